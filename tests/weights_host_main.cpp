// weights_host_main.cpp -- the stand-alone program of tests/test_weights_host.py: csrc/gnnb_weights.h driven from files, built
// with a plain C++ compiler under the address and undefined-behaviour sanitizers.  No GPU, no HIP header.
//   weights_host_main <job.txt> <in.bin> <out.bin> <out.txt>
// job.txt: the mode and its integers / floats, then the number of input tensors and the length of each; in.bin: those tensors,
// raw fp32, back to back; out.bin: the result, raw fp32; out.txt: the layout (mode `image`), one "name offset" line per
// tensor the model has.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "gnnb_weights.h"

using namespace gnnb;

static void write_floats(const char *path, const std::vector<float> &a, const std::vector<float> &b = {})
{
    FILE *f = fopen(path, "wb");
    if (!f)
        exit(3);
    for (const std::vector<float> *v : {&a, &b})
        if (!v->empty() && fwrite(v->data(), sizeof(float), v->size(), f) != v->size())
            exit(3);
    fclose(f);
}

int main(int argc, char **argv)
{
    if (argc != 5)
        return 2;
    std::ifstream job(argv[1]);
    std::string mode;
    job >> mode;
    gnnb_model_desc d{};
    int edge_dim = 0, K = 0, plus = 0;
    size_t fi = 0, fo = 0;
    float delta = 0.f;
    if (mode == "image" || mode == "gin_exec") {
        job >> d.conv_type >> d.num_layers >> d.in_dim >> d.hidden_dim >> d.out_dim >> d.skip >> d.fpx_w >> d.fpx_i >> d.pna_delta >> edge_dim >>
            d.mlp_num_linear >> d.mlp_hidden >> d.mlp_out >> d.num_pools;
    } else if (mode == "sage_cat") {
        job >> fo >> fi >> plus;
    } else if (mode == "zf") {
        job >> K >> d.out_dim;
    } else if (mode == "pna_fold") {
        job >> fi >> fo >> plus;
    } else if (mode == "pna_class") {
        job >> fi >> fo >> delta;
    } else {
        return 2;
    }
    size_t nt = 0;
    job >> nt;
    std::vector<std::vector<float>> t(nt);
    std::vector<const float *> p;
    FILE *in = fopen(argv[2], "rb");
    if (!job || !in)
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

    if (mode == "image") {
        const BuiltWeights b = build_weight_image(d, edge_dim, p.data());
        write_floats(argv[3], b.img);
        FILE *f = fopen(argv[4], "w");
        auto line = [f](const std::string &name, size_t off) {
            if (off != NO_OFFSET)
                fprintf(f, "%s %zu\n", name.c_str(), off);
        };
        for (size_t l = 0; l < b.layout.conv.size(); l++) {
            const LayerOffsets &o = b.layout.conv[l];
            const std::string at = "conv" + std::to_string(l) + ".";
            line(at + "w0", o.w0), line(at + "b0", o.b0), line(at + "w1", o.w1), line(at + "b1", o.b1);
            line(at + "edge_w", o.edge_w), line(at + "edge_b", o.edge_b);
            line(at + "w_cat", o.w_cat), line(at + "b_cat", o.b_cat), line(at + "w_cat_skip", o.w_cat_skip);
            line(at + "w_pre", o.w_pre), line(at + "b_pre", o.b_pre), line(at + "w_post", o.w_post), line(at + "b_post", o.b_post);
            line(at + "w_lin", o.w_lin), line(at + "b_lin", o.b_lin);
            line(at + "w_fold", o.w_fold), line(at + "b_fold", o.b_fold), line(at + "w_class", o.w_class), line(at + "b_class", o.b_class);
        }
        line("zf_w1f", b.layout.zf_w1f), line("gin_w", b.layout.gin_w), line("gin_b", b.layout.gin_b);
        for (size_t i = 0; i < b.layout.head_w.size(); i++)
            line("head" + std::to_string(i) + ".w", b.layout.head_w[i]), line("head" + std::to_string(i) + ".b", b.layout.head_b[i]);
        fclose(f);
    } else if (mode == "gin_exec") { // the GIN layers' four tensors each, as gnnb_model_create's image holds them
        WeightImage im(d);
        std::vector<LayerOffsets> off(d.num_layers);
        for (int l = 0; l < d.num_layers; l++)
            off[l] = push_conv_layer(im, d, l, p.data() + 4 * l, 0);
        const WeightBias g = gin_execution_order(d, im.img, off);
        write_floats(argv[3], g.w, g.b);
    } else if (mode == "sage_cat") {
        write_floats(argv[3], sage_cat_weights(p[0], p[1], fo, fi, plus != 0));
    } else if (mode == "zf") {
        write_floats(argv[3], zf_fragment_order(p[0], K, d.out_dim));
    } else if (mode == "pna_fold") { // {W_post, b_post, W_lin, b_lin}
        const WeightBias f = pna_fold_lin(p[0], p[1], p[2], p[3], fi, fo, plus != 0);
        write_floats(argv[3], f.w, f.b);
    } else { // pna_class: {W', b', W_pre, b_pre}
        const WeightBias c = pna_degree_class_weights(WeightBias{t[0], t[1]}, p[2], p[3], fi, fo, delta);
        write_floats(argv[3], c.w, c.b);
    }
    return 0;
}
