// weights_host_rgcn_main.cpp -- the stand-alone program of tests/test_weights_host_rgcn.py: csrc/gnnb_weights.h's image of an
// RGCNConv model (rgcn_relations: three tensors per layer, stacked into w_rgcn / b_rgcn) -- or of any other model through the
// builder's full argument list -- driven from files, built with a plain C++ compiler under the address and undefined-behaviour
// sanitizers.  No GPU, no HIP header.
//   weights_host_rgcn_main <job.txt> <in.bin> <out.bin> <out.txt>
// job.txt: conv_type num_layers in_dim hidden_dim out_dim skip edge_dim gat_heads tf_heads gated ggnn_steps rgcn_relations
// mlp_num_linear mlp_hidden mlp_out num_pools, then the number of input tensors and the length of each; in.bin: those tensors, raw fp32, back to back;
// out.bin: the image, raw fp32; out.txt: the layout, one "name offset" line per tensor the model has.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "gnnb_weights.h"

using namespace gnnb;

int main(int argc, char **argv)
{
    if (argc != 5)
        return 2;
    std::ifstream job(argv[1]);
    gnnb_model_desc d{};
    int edge_dim = 0, gat_heads = 0, tf_heads = 0, gated = 0, ggnn_steps = 0, rgcn_relations = 0;
    d.pna_delta = 1.0f;
    job >> d.conv_type >> d.num_layers >> d.in_dim >> d.hidden_dim >> d.out_dim >> d.skip >> edge_dim >> gat_heads >> tf_heads >> gated >>
        ggnn_steps >> rgcn_relations >> d.mlp_num_linear >> d.mlp_hidden >> d.mlp_out >> d.num_pools;
    size_t nt = 0;
    job >> nt;
    std::vector<std::vector<float>> t(nt);
    std::vector<const float *> p;
    FILE *in = fopen(argv[2], "rb");
    const int slots = rgcn_relations > 0 ? RGCN_PARAM_SLOTS
                      : ggnn_steps > 0 ? GGNN_PARAM_SLOTS
                      : gated         ? RG_PARAM_SLOTS
                      : tf_heads > 0  ? TF_PARAM_SLOTS + (edge_dim ? 1 : 0)
                      : gat_heads > 0 ? GAT_PARAM_SLOTS + (edge_dim ? 1 : 0)
                                      : conv_slots(d.conv_type) + (edge_dim ? 2 : 0);
    if (!job || !in || nt != (size_t)(slots * d.num_layers + 2 * d.mlp_num_linear))
        return 2;
    for (auto &v : t) {
        size_t n = 0;
        job >> n;
        v.resize(n);
        if (!job || fread(v.data(), sizeof(float), n, in) != n)
            return 2;
    }
    fclose(in);
    for (auto &v : t)
        p.push_back(v.data());

    const BuiltWeights b = build_weight_image(d, edge_dim, p.data(), gat_heads, tf_heads, gated != 0, 0, ggnn_steps, rgcn_relations);
    FILE *out = fopen(argv[3], "wb");
    if (!out || (!b.img.empty() && fwrite(b.img.data(), sizeof(float), b.img.size(), out) != b.img.size()))
        return 3;
    fclose(out);
    FILE *f = fopen(argv[4], "w");
    if (!f)
        return 3;
    auto line = [f](const std::string &name, size_t off) {
        if (off != NO_OFFSET)
            fprintf(f, "%s %zu\n", name.c_str(), off);
    };
    for (size_t l = 0; l < b.layout.conv.size(); l++) {
        const LayerOffsets &o = b.layout.conv[l];
        const std::string at = "conv" + std::to_string(l) + ".";
        line(at + "w0", o.w0), line(at + "b0", o.b0), line(at + "w1", o.w1), line(at + "b1", o.b1);
        line(at + "edge_w", o.edge_w), line(at + "edge_b", o.edge_b);
        line(at + "w_lr", o.w_lr), line(at + "b_lr", o.b_lr), line(at + "att", o.att), line(at + "gat_bias", o.gat_bias);
        line(at + "w_edge", o.w_edge);
        line(at + "w_qkvr", o.w_qkvr), line(at + "b_qkvr", o.b_qkvr);
        line(at + "w_qkvre", o.w_qkvre), line(at + "b_qkvre", o.b_qkvre);
        line(at + "w_kqvr", o.w_kqvr), line(at + "b_kqvr", o.b_kqvr);
        line(at + "w_ggc", o.w_ggc), line(at + "w_ggc_next", o.w_ggc_next), line(at + "b_ggc", o.b_ggc), line(at + "b_ih", o.b_ih);
        line(at + "w_rgcn", o.w_rgcn), line(at + "b_rgcn", o.b_rgcn);
        line(at + "w_cat", o.w_cat), line(at + "b_cat", o.b_cat), line(at + "w_cat_skip", o.w_cat_skip);
        line(at + "w_pre", o.w_pre), line(at + "b_pre", o.b_pre), line(at + "w_post", o.w_post), line(at + "b_post", o.b_post);
        line(at + "w_lin", o.w_lin), line(at + "b_lin", o.b_lin);
        line(at + "w_fold", o.w_fold), line(at + "b_fold", o.b_fold), line(at + "w_class", o.w_class), line(at + "b_class", o.b_class);
    }
    line("zf_w1f", b.layout.zf_w1f), line("gin_w", b.layout.gin_w), line("gin_b", b.layout.gin_b);
    for (size_t i = 0; i < b.layout.head_w.size(); i++)
        line("head" + std::to_string(i) + ".w", b.layout.head_w[i]), line("head" + std::to_string(i) + ".b", b.layout.head_b[i]);
    fclose(f);
    return 0;
}
