// gnnb_weights.h -- a model's weights as the forward reads them: the named slots of a conv layer (LayerSlots), the derived forms
// the kernels take (one helper each below) and build_weight_image, the ONE function that lays canonical and derived tensors out
// in the blob gnnb_model_create uploads.  Pure host arithmetic on the standard library and the C ABI's description: no HIP
// header in here, so that a plain C++ compiler builds it and tests/test_weights_host.py checks the layout, the permutations and
// the folded sums without a GPU.
// Reference: load_parameters once (gnnbuilder/templates/model.cpp.jinja:724-730).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "gnnb_hip.h"

namespace gnnb {

struct LayerDims {
    int fin, fout;
};

// canonical parameter tensors per conv layer (-1: unknown conv type)
inline int conv_slots(int conv)
{
    switch (conv) {
    case GNNB_CONV_GCN: return 2;
    case GNNB_CONV_GIN: return 4;
    case GNNB_CONV_SAGE: return 3;
    case GNNB_CONV_PNA: return 6;
    default: return -1;
    }
}

// gnnbuilder/models.py:519-549
inline LayerDims layer_dims(const gnnb_model_desc &d, int l)
{
    if (d.num_layers == 1)
        return {d.in_dim, d.out_dim};
    if (l == 0)
        return {d.in_dim, d.hidden_dim};
    if (l == d.num_layers - 1)
        return {d.hidden_dim, d.out_dim};
    return {d.hidden_dim, d.hidden_dim};
}

inline int gnn_out_width(const gnnb_model_desc &d) { return d.num_layers == 0 ? d.in_dim : d.out_dim; }

// gnnbuilder/models.py:398-415
inline void mlp_dims(const gnnb_model_desc &d, int i, int *din, int *dout)
{
    const int pooled = d.num_pools * gnn_out_width(d);
    *din = (i == 0) ? pooled : d.mlp_hidden;
    *dout = (i == d.mlp_num_linear - 1) ? d.mlp_out : d.mlp_hidden;
}

constexpr size_t NO_OFFSET = ~(size_t)0;
// what a slot holds when the layer has no such tensor: nullptr, or NO_OFFSET in the layout
template <typename T> constexpr T absent_slot() { return T(); }
template <> constexpr size_t absent_slot<size_t>() { return NO_OFFSET; }

// One conv layer's tensors in the blob, by name: T = const float * in a model (LayerWeights: device pointers), size_t in the
// layout build_weight_image returns (LayerOffsets: floats from the image's start).  A layer holds its conv type's members and
// leaves the others absent.  The C side's one statement of what follows the canonical order of include/gnnb_hip.h
// (gnnb_model_num_params) and models.py (canonical_param_names); in = the layer's input width, out = its output width; all
// row-major [out][in] as torch.nn.Linear.weight.  "canonical" = tensor k of the layer as the caller passed it.
//   GCN        w0 [out, in], b0 [out]               canonical 0, 1
//   GIN, GINE  w0 [out, in], b0 [out]               canonical 0, 1: the first linear (ReLU behind it; hidden = out, models.py:90)
//              w1 [out, out], b1 [out]              canonical 2, 3: the second linear
//              edge_w [in, edge_dim], edge_b [in]   canonical 4, 5 of a GINE model (gnnb_model::edge_dim > 0): conv.lin
//   GraphSAGE  w_cat [out, 2 in]                    derived: [Wl | Wr], canonical 0 and 2 side by side (sage_cat_weights)
//              b_cat [out]                          canonical 1: lin_l's bias (lin_r has none); goes with either w_cat form
//              w_cat_skip [out, 2 in]               derived: [Wl | Wr + I]; a skip middle layer with in == out, not under fpx
//   PNA        w_pre [in, 2 in], b_pre [in]         canonical 0, 1: the pre-NN; columns [0, in) act on the destination x_i
//              w_post [out, 13 in], b_post [out]    canonical 2, 3: the post-NN
//              w_lin [out, out], b_lin [out]        canonical 4, 5
//              w_fold [out, 13 in], b_fold [out]    derived: `lin` folded into the post-NN, + I on a skip middle layer with
//                                                   in == out (pna_fold_lin); not under fpx
//              w_class [16][out, 5 in], b_class [16][out]   derived: the degree-class form of w_fold (pna_degree_class_weights);
//                                                   where w_fold exists and out > 32
//   PNA + edges  (gnnb_model::edge_dim > 0, gnnb_pna_edge_model_create) PNA's slots with a three-block pre-NN, and
//              w_pre [in, 3 in]                     canonical 0: columns [2 in, 3 in) = W_c act on the encoded edge attributes
//              edge_w [in, edge_dim], edge_b [in]   derived from canonical 6, 7 (conv.edge_encoder): W_c W_enc and W_c b_enc
//                                                   (pna_edge_projection) -- what k_pna_edge_aggregate adds to q_i + p_j
//              no w_class / b_class: such a model does not take the degree-class form
//   GATv2      (gnnb_model::gat_heads > 0, gnnb_gat_model_create: a GCN description) none of GCN's slots, but
//              w_lr [2 out, in]                     derived: [W_l ; W_r], canonical 0 (conv.lin_l.weight) on top of canonical 2
//                                                   (conv.lin_r.weight) -- ONE GEMM gives [xl | xr] [N, 2 out] (gat_stack_rows)
//              b_lr [2 out]                         derived: [b_l ; b_r], canonical 1 and 3
//              att [out]                            canonical 4: conv.att [1, heads, out / heads], head-major
//              gat_bias [out]                       canonical 5: conv.bias, added behind the aggregate
//   GATv2 + edges  (gat_heads > 0 and edge_dim > 0, gnnb_gat_edge_model_create) GATv2's slots, and
//              w_edge [out, edge_dim]               canonical 6: conv.lin_edge.weight (no bias), raw -- what k_gatv2_edge_aggregate
//                                                   projects the edge attributes with, inside the score
//   GAT v1     (gnnb_model::gat1_heads > 0, gnnb_gatconv_model_create: a GCN description) none of GCN's slots, but
//              w_gat [out + roundup4(2 heads), in]  derived: [W ; A_src W ; A_dst W ; 0], canonical 0 (conv.lin.weight, no bias) on top
//                                                   of the folded score rows (gat_score_fold): row out + h = sum_c att_src[h, c] W[h C + c],
//                                                   row out + heads + h likewise with att_dst (canonical 1, 2: conv.att_src, conv.att_dst
//                                                   [1, heads, out / heads]); zero rows up to a multiple of 4 -- ONE GEMM gives
//                                                   [xl | s_src | s_dst | pad].  No GEMM bias
//              gat_bias [out]                       canonical 3: conv.bias, added behind the aggregate
//   GAT v1 + edges  (gat1_heads > 0 and edge_dim > 0, gnnb_gatconv_edge_model_create) GAT v1's slots -- w_gat is exactly the plain
//              model's, so the GEMM is unchanged -- and
//              a_edge [heads, roundup4(edge_dim)]   derived: row h = sum_c att_edge[h, c] W_e[h C + c, :] (gat_edge_fold), canonical 4
//                                                   (conv.att_edge [1, heads, out / heads]) folded into canonical 5
//                                                   (conv.lin_edge.weight [out, edge_dim], no bias); zero columns up to a multiple
//                                                   of 4 -- what k_gat_edge_aggregate forms an edge's score term with
//   TransformerConv  (gnnb_model::tf_heads > 0, gnnb_transformer_model_create: a GIN description) none of GIN's slots, but
//              w_qkvr [4 out, in]                   derived: [W_q ; W_k ; W_v ; W_skip], canonical 2 (conv.lin_query.weight), 0
//                                                   (conv.lin_key.weight), 4 (conv.lin_value.weight), 6 (conv.lin_skip.weight) on top
//                                                   of each other -- ONE GEMM gives [q | k | v | r] [N, 4 out] (stack_rows)
//              b_qkvr [4 out]                       derived: [b_q ; b_k ; b_v ; b_skip], canonical 3, 1, 5, 7
//   TransformerConv + edges  (tf_heads > 0 and edge_dim > 0, gnnb_transformer_edge_model_create) neither of TransformerConv's slots, but
//              w_qkvre [4 out + roundup4(heads edge_dim), in]   derived: [W_q ; W_k ; W_v ; W_skip ; W_qe ; 0], W_qe [heads edge_dim, in] =
//                                                   per head W_e[h]^T W_q[h] (transformer_edge_fold) -- ONE GEMM gives
//                                                   [q | k | v | r | qe] with qe_i[h] = W_e[h]^T q_i[h]; zero rows up to a multiple of 4
//              b_qkvre [4 out + roundup4(heads edge_dim)]       derived: [b_q ; b_k ; b_v ; b_skip ; W_e[h]^T b_q[h] ; 0]
//              w_edge [out, edge_dim]               canonical 8: conv.lin_edge.weight (no bias), raw -- what
//                                                   k_transformer_edge_aggregate applies to the weighted attribute sum in its epilogue
//   ResGatedGraphConv  (gnnb_model::gated, gnnb_resgated_model_create: a GIN description) none of GIN's slots, but
//              w_kqvr [4 out, in]                   derived: [W_k ; W_q ; W_v ; W_skip], canonical 0 (conv.lin_key.weight), 2
//                                                   (conv.lin_query.weight), 4 (conv.lin_value.weight), 6 (conv.lin_skip.weight) on top
//                                                   of each other -- ONE GEMM gives [k | q | v | r] [N, 4 out]; q and v are adjacent
//                                                   blocks, so a neighbour's q_j | v_j is ONE span of 2 out floats of its row
//              b_kqvr [4 out]                       derived: [b_k ; b_q ; b_v ; bias], canonical 1, 3, 5 and 7 (conv.bias): lin_skip has
//                                                   no bias, so the conv's own rides as the skip block's GEMM bias.  b_q is NOT
//                                                   folded into b_k: every block keeps the rounding of its own linear
//   ResGatedGraphConv + edges  (gated and edge_dim > 0, gnnb_resgated_edge_model_create) lin_key / lin_query / lin_value are
//              [out, in + edge_dim], the x columns first
//              w_kqvr [4 out, in]                   derived: [W_kx ; W_qx ; W_vx ; W_skip] -- the x column blocks, copied
//              b_kqvr [4 out]                       as above
//              w_gv_edge [2 out, edge_dim]          derived: [W_g ; W_v], W_g = W_ke + W_qe (the e column blocks of lin_key and
//                                                   lin_query: both enter the gate's argument; added in double, rounded once --
//                                                   resgated_edge_blocks), W_v = W_ve, copied -- what k_resgated_edge_aggregate adds
//                                                   per edge to the gate's argument and to the value
//   GatedGraphConv  (gnnb_model::ggnn_steps > 0, gnnb_ggnn_model_create: a GIN description) none of GIN's slots, but per (layer, step)
//              w_ggc [6 out, in]                    derived, step 0: [W_p[0][:, :in] ; weight_hh[:, :in]], W_p[t] = weight_ih weight[t]^T
//                                                   [3 out, out] (ggnn_fold: canonical 1, conv.rnn.weight_ih, folded into canonical 0,
//                                                   conv.weight [steps, out, out]) on top of canonical 2 (conv.rnn.weight_hh) -- ONE
//                                                   GEMM gives [p | gh] [N, 6 out].  Only the first `in` input columns: h_0 = [x | 0]
//              w_ggc_next [steps - 1][6 out, out]   derived, steps 1 ..: [W_p[t] ; weight_hh], each at ggnn_step_stride(out) floats
//              b_ggc [6 out]                        derived: [0 | bias_hh], canonical 4 -- the p block takes NO bias (it would be
//                                                   counted once per edge)
//              b_ih [3 out]                         canonical 3: conv.rnn.bias_ih, raw -- k_ggnn_aggregate adds it once per row
//   RGCNConv  (gnnb_model::rgcn_relations = R > 0, gnnb_rgcn_model_create: a GIN description) none of GIN's slots, but
//              w_rgcn [(R + 1) out, in]             derived: [weight[0]^T ; .. ; weight[R-1]^T ; root^T] -- canonical 0, conv.weight
//                                                   [R, in, out], and canonical 1, conv.root [in, out], both applied as x @ W: pure
//                                                   transposes into nn.Linear layout, no arithmetic (rgcn_stack) -- ONE GEMM gives
//                                                   [p_0 | .. | p_{R-1} | root] [N, (R + 1) out]
//              b_rgcn [(R + 1) out]                 derived: [0 | .. | 0 | bias], canonical 2 -- the relation blocks take NO bias
//                                                   (it would be counted once per edge)
// (GCN's pair has the names of GIN's first linear: the stack kernels and k_conv_rows take either through the same operands)
template <typename T> struct LayerSlots {
    T w0 = absent_slot<T>(), b0 = absent_slot<T>(), w1 = absent_slot<T>(), b1 = absent_slot<T>();
    T edge_w = absent_slot<T>(), edge_b = absent_slot<T>();
    T w_lr = absent_slot<T>(), b_lr = absent_slot<T>(), att = absent_slot<T>(), gat_bias = absent_slot<T>(), w_edge = absent_slot<T>();
    T w_gat = absent_slot<T>(), a_edge = absent_slot<T>();
    T w_qkvr = absent_slot<T>(), b_qkvr = absent_slot<T>();
    T w_qkvre = absent_slot<T>(), b_qkvre = absent_slot<T>();
    T w_kqvr = absent_slot<T>(), b_kqvr = absent_slot<T>(), w_gv_edge = absent_slot<T>();
    T w_ggc = absent_slot<T>(), w_ggc_next = absent_slot<T>(), b_ggc = absent_slot<T>(), b_ih = absent_slot<T>();
    T w_rgcn = absent_slot<T>(), b_rgcn = absent_slot<T>();
    T w_cat = absent_slot<T>(), b_cat = absent_slot<T>(), w_cat_skip = absent_slot<T>();
    T w_pre = absent_slot<T>(), b_pre = absent_slot<T>(), w_post = absent_slot<T>(), b_post = absent_slot<T>();
    T w_lin = absent_slot<T>(), b_lin = absent_slot<T>();
    T w_fold = absent_slot<T>(), b_fold = absent_slot<T>(), w_class = absent_slot<T>(), b_class = absent_slot<T>();

    // the same slots with f applied to each (offsets -> pointers)
    template <typename F> auto map(F f) const -> LayerSlots<decltype(f(w0))>
    {
        return {f(w0),    f(b0),    f(w1),     f(b1),     f(edge_w), f(edge_b), f(w_lr),   f(b_lr),    f(att),        f(gat_bias), f(w_edge), f(w_gat), f(a_edge), f(w_qkvr), f(b_qkvr), f(w_qkvre), f(b_qkvre), f(w_kqvr), f(b_kqvr), f(w_gv_edge), f(w_ggc), f(w_ggc_next), f(b_ggc), f(b_ih), f(w_rgcn), f(b_rgcn), f(w_cat),
                f(b_cat), f(w_cat_skip), f(w_pre), f(b_pre), f(w_post), f(b_post), f(w_lin), f(b_lin), f(w_fold), f(b_fold), f(w_class),
                f(b_class)};
    }
};
using LayerWeights = LayerSlots<const float *>;
using LayerOffsets = LayerSlots<size_t>;

// where everything sits in the image (floats from its start; NO_OFFSET: the model has no such tensor)
struct WeightLayout {
    std::vector<LayerOffsets> conv;
    size_t zf_w1f = NO_OFFSET;                    // gnnb_model::zf_w1f
    size_t gin_w = NO_OFFSET, gin_b = NO_OFFSET; // gnnb_model::gin_w, gin_b
    std::vector<size_t> head_w, head_b;
};

// host staging image of the blob: every tensor padded to a 16-byte boundary
struct WeightImage {
    std::vector<float> img;
    bool fpx;
    float q_inv, q_step, q_span, q_half;
    explicit WeightImage(const gnnb_model_desc &d)
        : fpx(d.fpx_w > 0), q_inv(fpx ? ldexpf(1.0f, d.fpx_w - d.fpx_i) : 1.0f), q_step(fpx ? ldexpf(1.0f, -(d.fpx_w - d.fpx_i)) : 1.0f),
          q_span(fpx ? ldexpf(1.0f, d.fpx_i) : 1.0f), q_half(fpx ? ldexpf(1.0f, d.fpx_i - 1) : 1.0f)
    {
    }
    size_t push(const float *src, size_t n) // -> offset of the tensor in the image
    {
        size_t off = img.size();
        img.insert(img.end(), src, src + n);
        if (fpx) // W_TYPE = ap_fixed<W, I>: the weights live on the grid (model.h.jinja:41-45)
            for (size_t i = off; i < off + n; i++) {
                float v = floorf(img[i] * q_inv) * q_step;
                img[i] = v - q_span * floorf((v + q_half) / q_span);
            }
        while (img.size() % 4)
            img.push_back(0.0f);
        return off;
    }
    size_t push(const std::vector<float> &v) { return push(v.data(), v.size()); }
};

struct WeightBias { // a derived matrix and the bias that goes with it
    std::vector<float> w, b;
};

// GraphSAGE: lin_l and lin_r fused into one [out, 2*in] matrix [Wl | Wr]; plus_identity: [Wl | Wr + I], the layer's skip
// connection folded into the root weights
inline std::vector<float> sage_cat_weights(const float *wl, const float *wr, size_t fo, size_t fi, bool plus_identity)
{
    std::vector<float> cat(fo * 2 * fi);
    for (size_t o = 0; o < fo; o++) {
        memcpy(&cat[o * 2 * fi], wl + o * fi, fi * sizeof(float));
        memcpy(&cat[o * 2 * fi + fi], wr + o * fi, fi * sizeof(float));
    }
    if (plus_identity)
        for (size_t o = 0; o < fo; o++)
            cat[o * 2 * fi + fi + o] += 1.0f;
    return cat;
}

// PNA: `lin` folded into the post-NN.  PNAConv applies them back to back with nothing in between
// (out = W_lin (W_post [x | S] + b_post) + b_lin, gnn_builder_lib.h:2081-2157), so
// W' = W_lin W_post [out, 13 F] and b' = W_lin b_post + b_lin (formed in double, rounded once) give the layer
// in ONE 13F-wide GEMM whose epilogue carries the skip operand and the activation: the out x out GEMM and the
// [N, out] hand-over between the two are gone (3 x ~55 us of a BASELINE config 4 step).  Not under the
// fixed-point emulation: the folded matrix is not on the weight grid.
inline WeightBias pna_fold_lin(const float *w_post, const float *b_post, const float *w_lin, const float *b_lin, size_t fi, size_t fo,
                               bool skip_fold)
{
    const size_t K13 = 13 * fi;
    std::vector<double> acc(K13);
    WeightBias f{std::vector<float>(fo * K13), std::vector<float>(fo)};
    for (size_t o = 0; o < fo; o++) {
        std::fill(acc.begin(), acc.end(), 0.0);
        double ab = (double)b_lin[o];
        for (size_t h = 0; h < fo; h++) {
            const double wl = (double)w_lin[o * fo + h];
            const float *wp = w_post + h * K13;
            for (size_t k = 0; k < K13; k++)
                acc[k] += wl * (double)wp[k];
            ab += wl * (double)b_post[h];
        }
        if (skip_fold)
            acc[o] += 1.0; // (+ I on the x segment: the skip connection)
        for (size_t k = 0; k < K13; k++)
            f.w[o * K13 + k] = (float)acc[k];
        f.b[o] = (float)ab;
    }
    return f;
}

// PNA, the degree-class form (gnnb_workspace_set_max_degree): for every in-degree c = 0 .. 15 the matrix
//   ( W'_x + S_c Wq | W'_1 + amp W'_2 + att W'_3 ),  [out, 5 F],   and the bias  b' + S_c bq,
// of the folded W' above (`folded`); amp / att as graph prep computes them (k_prep.hip: logf(d + 1) / delta and its
// reciprocal, d = max(c, 1)).  S_c = the max + min + mean column blocks of the class's A matrix: the
// destination's own pre-NN term q_i = Wq x_i + bq shifts max, min and mean of its messages by q_i and
// leaves std alone (gnn_builder_lib.h:1801-1850), so it is folded into x's weights too and the q GEMM is
// not run at all.  Class 0 (no messages: the four aggregates are 0, not q) carries no S term.
// wq = W_pre [F, 2F]: columns [0, F) act on the destination x_i (lib:1801-1802), bias bq
inline WeightBias pna_degree_class_weights(const WeightBias &folded, const float *wq, const float *bq, size_t fi, size_t fo, float pna_delta)
{
    const size_t K13 = 13 * fi, K5 = 5 * fi;
    WeightBias c5{std::vector<float>((size_t)GNNB_DEG_CLASSES * fo * K5), std::vector<float>((size_t)GNNB_DEG_CLASSES * fo)};
    std::vector<double> wa(4 * fi), sq(fi), sqw(fi);
    for (int c = 0; c < GNNB_DEG_CLASSES; c++) {
        const float lg = logf((float)std::max(c, 1) + 1.0f);
        const double amp = (double)(lg / pna_delta), att = (double)(pna_delta / lg);
        float *dst = &c5.w[(size_t)c * fo * K5];
        for (size_t o = 0; o < fo; o++) {
            const float *src = &folded.w[o * K13];
            for (size_t k = 0; k < 4 * fi; k++)
                wa[k] = (double)src[fi + k] + amp * (double)src[5 * fi + k] + att * (double)src[9 * fi + k];
            for (size_t k = 0; k < 4 * fi; k++)
                dst[o * K5 + fi + k] = (float)wa[k];
            double bsum = (double)folded.b[o];
            if (c > 0) {
                for (size_t k = 0; k < fi; k++)
                    sq[k] = wa[k] + wa[fi + k] + wa[2 * fi + k]; // S_c[o][k]: max + min + mean
                // (S_c Wq)[o][j] = sum_k S_c[o][k] Wq[k][j], k ascending from src[j] as before, but walked
                // along Wq's rows: the column walk (stride 2F) made a 1024-wide PNA layer's upload ~80 s
                for (size_t j = 0; j < fi; j++)
                    sqw[j] = (double)src[j];
                for (size_t k = 0; k < fi; k++) {
                    const double s = sq[k];
                    const float *wr = wq + k * 2 * fi;
                    for (size_t j = 0; j < fi; j++)
                        sqw[j] += s * (double)wr[j];
                }
                for (size_t j = 0; j < fi; j++)
                    dst[o * K5 + j] = (float)sqw[j];
                for (size_t k = 0; k < fi; k++)
                    bsum += sq[k] * (double)bq[k];
            } else {
                for (size_t j = 0; j < fi; j++)
                    dst[o * K5 + j] = src[j];
            }
            c5.b[(size_t)c * fo + o] = (float)bsum;
        }
    }
    return c5;
}

// PNA with edge features: the pre-NN is linear, so its third column block W_c = W_pre[:, 2F:3F] and the edge encoder collapse into
// ONE projection of the raw attributes, pre_nn([x_i | x_j | W_enc e + b_enc]) = (Wa x_i + b) + Wb x_j + (W_c W_enc) e + W_c b_enc:
//   w [F, edge_dim] = W_c W_enc,   b [F] = W_c b_enc      (formed in double, rounded once)
// w_pre [F, 3F], w_enc [F, edge_dim], b_enc [F]
inline WeightBias pna_edge_projection(const float *w_pre, const float *w_enc, const float *b_enc, size_t fi, size_t edge_dim)
{
    WeightBias e{std::vector<float>(fi * edge_dim), std::vector<float>(fi)};
    std::vector<double> acc(edge_dim);
    for (size_t o = 0; o < fi; o++) {
        const float *wc = w_pre + o * 3 * fi + 2 * fi;
        std::fill(acc.begin(), acc.end(), 0.0);
        double ab = 0.0;
        for (size_t h = 0; h < fi; h++) {
            const double c = (double)wc[h];
            for (size_t k = 0; k < edge_dim; k++)
                acc[k] += c * (double)w_enc[h * edge_dim + k];
            ab += c * (double)b_enc[h];
        }
        for (size_t k = 0; k < edge_dim; k++)
            e.w[o * edge_dim + k] = (float)acc[k];
        e.b[o] = (float)ab;
    }
    return e;
}

// k_gcn2_zf reads its 16-column slice of the last GCN layer's weight as MFMA B fragments: lane (li, lg) of the wave that
// owns slice s takes W[16 s + li][16 q + 4 lg .. + 3] for q = 0 .. K/16 - 1.  Straight from the [out][in] matrix that is
// 16 rows x 64 B per load instruction (half of every 128-B line unused, 32 MB of L2 traffic per launch over the chip);
// a second copy in fragment order -- float4 index ((s K/16 + q) 4 + lg) 16 + li -- makes every load instruction one
// contiguous KiB.  Rows past `out` are zero.  w1 [out_dim, K]
inline std::vector<float> zf_fragment_order(const float *w1, int K, int out_dim)
{
    const int KQ = K / 16, NS = (out_dim + 15) / 16;
    std::vector<float> frag((size_t)NS * 16 * K, 0.0f);
    for (int s = 0; s < NS; s++)
        for (int q = 0; q < KQ; q++)
            for (int lg = 0; lg < 4; lg++)
                for (int li = 0; li < 16; li++) {
                    const int n = 16 * s + li;
                    if (n >= out_dim)
                        continue;
                    for (int e = 0; e < 4; e++)
                        frag[((((size_t)s * KQ + q) * 4 + lg) * 16 + li) * 4 + e] = w1[(size_t)n * K + 16 * q + 4 * lg + e];
                }
    return frag;
}

// GIN stacks: every wide matrix once more in EXECUTION order at one hidden x hidden stride, zero-padded (gnnb_model::gin_w):
// index 0 = layer 0's second linear, 2l - 1 / 2l = layer l's first / second linear; the biases likewise.  Read from the
// image (conv_off: the layers' canonical tensors in it), so the copies are on the fixed-point grid when the originals are.
inline WeightBias gin_execution_order(const gnnb_model_desc &d, const std::vector<float> &img, const std::vector<LayerOffsets> &conv_off)
{
    const size_t h = d.hidden_dim, ho = d.out_dim;
    const int L = d.num_layers, nm = 2 * L - 1;
    WeightBias g{std::vector<float>((size_t)nm * h * h, 0.0f), std::vector<float>((size_t)nm * h, 0.0f)};
    auto put = [&](int idx, size_t off_w, size_t off_b, size_t rows, size_t cols) { // [rows, cols] -> top-left of slot idx
        for (size_t r = 0; r < rows; r++)
            memcpy(&g.w[(size_t)idx * h * h + r * h], &img[off_w + r * cols], cols * sizeof(float));
        memcpy(&g.b[(size_t)idx * h], &img[off_b], rows * sizeof(float));
    };
    put(0, conv_off[0].w1, conv_off[0].b1, L == 1 ? ho : h, L == 1 ? ho : h); // (layer 0's second linear)
    for (int l = 1; l < L; l++) {
        const size_t fo = l == L - 1 ? ho : h;
        put(2 * l - 1, conv_off[l].w0, conv_off[l].b0, fo, h); // Wa [fo, h]
        put(2 * l, conv_off[l].w1, conv_off[l].b1, fo, fo);     // Wb [fo, fo]
    }
    return g;
}

// GATv2: two tensors of `rows_each` rows of `cols` floats, the first on top of the second ([W_l ; W_r], and with cols = 1 [b_l ; b_r])
inline std::vector<float> gat_stack_rows(const float *top, const float *bottom, size_t rows_each, size_t cols)
{
    std::vector<float> s(2 * rows_each * cols);
    memcpy(s.data(), top, rows_each * cols * sizeof(float));
    memcpy(s.data() + rows_each * cols, bottom, rows_each * cols * sizeof(float));
    return s;
}

// TransformerConv: gat_stack_rows for n tensors, the first on top ([W_q ; W_k ; W_v ; W_skip], and with cols = 1 the biases)
inline std::vector<float> stack_rows(std::initializer_list<const float *> parts, size_t rows_each, size_t cols)
{
    std::vector<float> s(parts.size() * rows_each * cols);
    size_t at = 0;
    for (const float *p : parts) {
        memcpy(s.data() + at, p, rows_each * cols * sizeof(float));
        at += rows_each * cols;
    }
    return s;
}

// TransformerConv with edge features: the query's edge term as a linear function of x.  q_i[h] . (W_e[h] e) = (W_e[h]^T q_i[h]) . e,
// and q = W_q x + b_q, so qe_i[h * edge_dim + t] = (W_qe x_i + b_qe)[h * edge_dim + t] with
//   W_qe[h * edge_dim + t][:] = sum_c W_e[h C + c][t] * W_q[h C + c][:],   b_qe[h * edge_dim + t] = sum_c W_e[h C + c][t] * b_q[h C + c]
// (C = fo / heads; accumulated in double, c increasing, rounded once -- as pna_edge_projection), padded with zero rows to a multiple
// of 4 rows: w [roundup4(heads edge_dim), fi], b [roundup4(heads edge_dim)].  w_q [fo, fi], b_q [fo], w_e [fo, edge_dim]
inline size_t transformer_edge_qe_rows(size_t heads, size_t edge_dim) { return (heads * edge_dim + 3) / 4 * 4; }
inline WeightBias transformer_edge_fold(const float *w_q, const float *b_q, const float *w_e, size_t fi, size_t fo, size_t heads, size_t edge_dim)
{
    const size_t C = fo / heads, rows = transformer_edge_qe_rows(heads, edge_dim);
    WeightBias f{std::vector<float>(rows * fi, 0.0f), std::vector<float>(rows, 0.0f)};
    std::vector<double> acc(fi);
    for (size_t h = 0; h < heads; h++)
        for (size_t t = 0; t < edge_dim; t++) {
            std::fill(acc.begin(), acc.end(), 0.0);
            double ab = 0.0;
            for (size_t c = 0; c < C; c++) {
                const double e = (double)w_e[(h * C + c) * edge_dim + t];
                const float *wq = w_q + (h * C + c) * fi;
                for (size_t k = 0; k < fi; k++)
                    acc[k] += e * (double)wq[k];
                ab += e * (double)b_q[h * C + c];
            }
            for (size_t k = 0; k < fi; k++)
                f.w[(h * edge_dim + t) * fi + k] = (float)acc[k];
            f.b[h * edge_dim + t] = (float)ab;
        }
    return f;
}

// GAT v1: both per-node scores as linear functions of x.  s_src_j[h] = sum_c att_src[h, c] (W x_j)[h C + c] = (A_src W x_j)[h], so
//   w[fo + h][:] = sum_c att_src[h C + c] * W[h C + c][:],   w[fo + heads + h][:] = sum_c att_dst[h C + c] * W[h C + c][:]
// (C = fo / heads; accumulated in double, c increasing, rounded once -- as resgated_edge_blocks and transformer_edge_fold) under W's
// own fo rows, copied, and padded with zero rows to a multiple of 4 score rows: [fo + gat_score_rows(heads), fi].  w [fo, fi],
// att_src / att_dst [fo] head-major
inline size_t gat_score_rows(size_t heads) { return (2 * heads + 3) / 4 * 4; }
inline std::vector<float> gat_score_fold(const float *w, const float *att_src, const float *att_dst, size_t fi, size_t fo, size_t heads)
{
    const size_t C = fo / heads;
    std::vector<float> f((fo + gat_score_rows(heads)) * fi, 0.0f);
    memcpy(f.data(), w, fo * fi * sizeof(float));
    std::vector<double> acc(fi);
    for (size_t side = 0; side < 2; side++)
        for (size_t h = 0; h < heads; h++) {
            const float *att = side ? att_dst : att_src;
            std::fill(acc.begin(), acc.end(), 0.0);
            for (size_t c = 0; c < C; c++) {
                const double a = (double)att[h * C + c];
                const float *wr = w + (h * C + c) * fi;
                for (size_t k = 0; k < fi; k++)
                    acc[k] += a * (double)wr[k];
            }
            for (size_t k = 0; k < fi; k++)
                f[(fo + side * heads + h) * fi + k] = (float)acc[k];
        }
    return f;
}

// GAT v1 with edge features: the edge term of the score as a linear function of the edge attribute.  a_edge[h] . (W_e e)[h C ..] =
// (A_edge W_e)[h, :] . e, so
//   f[h][:] = sum_c att_edge[h C + c] * W_e[h C + c][:]
// (accumulated in double, c increasing, rounded once -- as gat_score_fold) at row stride gat_edge_cols(edge_dim), the pad columns
// zero: [heads, roundup4(edge_dim)].  w_edge [fo, edge_dim], att_edge [fo] head-major
inline size_t gat_edge_cols(size_t edge_dim) { return (edge_dim + 3) / 4 * 4; }
inline std::vector<float> gat_edge_fold(const float *w_edge, const float *att_edge, size_t edge_dim, size_t fo, size_t heads)
{
    const size_t C = fo / heads, ld = gat_edge_cols(edge_dim);
    std::vector<float> f(heads * ld, 0.0f);
    std::vector<double> acc(edge_dim);
    for (size_t h = 0; h < heads; h++) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (size_t c = 0; c < C; c++) {
            const double a = (double)att_edge[h * C + c];
            const float *wr = w_edge + (h * C + c) * edge_dim;
            for (size_t k = 0; k < edge_dim; k++)
                acc[k] += a * (double)wr[k];
        }
        for (size_t k = 0; k < edge_dim; k++)
            f[h * ld + k] = (float)acc[k];
    }
    return f;
}

// ResGatedGraphConv with edge features: a linear's [fo, fi + edge_dim] weight (x columns first) split.  x_cols: its [fo, fi] block
inline std::vector<float> resgated_x_cols(const float *w, size_t fi, size_t fo, size_t edge_dim)
{
    std::vector<float> x(fo * fi);
    for (size_t c = 0; c < fo; c++)
        memcpy(&x[c * fi], w + c * (fi + edge_dim), fi * sizeof(float));
    return x;
}
// ... and [W_g ; W_v] [2 fo, edge_dim]: W_g[c][t] = W_ke[c][t] + W_qe[c][t] in double, rounded once (the gate's argument takes
// lin_key's and lin_query's edge terms, both of the same e_ij); W_v = W_ve, copied
inline std::vector<float> resgated_edge_blocks(const float *w_key, const float *w_query, const float *w_value, size_t fi, size_t fo, size_t edge_dim)
{
    std::vector<float> gv(2 * fo * edge_dim);
    const size_t ld = fi + edge_dim;
    for (size_t c = 0; c < fo; c++)
        for (size_t t = 0; t < edge_dim; t++) {
            gv[c * edge_dim + t] = (float)((double)w_key[c * ld + fi + t] + (double)w_query[c * ld + fi + t]);
            gv[(fo + c) * edge_dim + t] = w_value[c * ld + fi + t];
        }
    return gv;
}

// GatedGraphConv: the message weight folded into the GRU's input weight.  m_i = sum_j h_j weight[t] (a plain matmul) and
// gi = m weight_ih^T, so gi_i = sum_j h_j (weight[t] weight_ih^T) = sum_j W_p[t] h_j in nn.Linear layout with
//   W_p[t][g][k] = sum_c weight_ih[g][c] * weight[t][k][c]          [3 fo, fo]
// (accumulated in double, c increasing, rounded once -- as gat_score_fold) on top of weight_hh, both cut to their first `cols` input
// columns: [6 fo, cols].  cols = the layer's input width at step 0 (h_0 = [x | 0]: the zero padding costs no flops), fo behind it.
// weight_t [fo, fo] = weight[t], w_ih / w_hh [3 fo, fo]
inline std::vector<float> ggnn_fold(const float *weight_t, const float *w_ih, const float *w_hh, size_t fo, size_t cols)
{
    std::vector<float> f(6 * fo * cols);
    for (size_t g = 0; g < 3 * fo; g++)
        for (size_t k = 0; k < cols; k++) {
            double acc = 0.0;
            for (size_t c = 0; c < fo; c++)
                acc += (double)w_ih[g * fo + c] * (double)weight_t[k * fo + c];
            f[g * cols + k] = (float)acc;
        }
    for (size_t g = 0; g < 3 * fo; g++)
        memcpy(&f[(3 * fo + g) * cols], w_hh + g * fo, cols * sizeof(float));
    return f;
}
// floats between the [6 fo, fo] matrices of steps 1 .. (whole 16-byte pieces, as every tensor of the image)
inline size_t ggnn_step_stride(size_t fo) { return (6 * fo * fo + 3) / 4 * 4; }

// RGCNConv: the R relation weights and the root weight, each [fi, fo] and applied as x @ W, stacked in nn.Linear layout:
// [(R + 1) fo, fi], block r = weight[r]^T, block R = root^T.  Pure transposes: every float of the result is a float of the input
inline std::vector<float> rgcn_stack(const float *weight, const float *root, size_t relations, size_t fi, size_t fo)
{
    std::vector<float> w((relations + 1) * fo * fi);
    for (size_t r = 0; r <= relations; r++) {
        const float *src = r < relations ? weight + r * fi * fo : root;
        for (size_t o = 0; o < fo; o++)
            for (size_t k = 0; k < fi; k++)
                w[(r * fo + o) * fi + k] = src[k * fo + o];
    }
    return w;
}

constexpr int GAT_PARAM_SLOTS = 6; // a GATv2 layer's canonical tensors (gnnb_gat.h); one more with edge features (gnnb_gat_edge.h)
constexpr int TF_PARAM_SLOTS = 8;  // a TransformerConv layer's canonical tensors (gnnb_transformer.h); one more with edge features
                                   // (gnnb_transformer_edge.h)
constexpr int RG_PARAM_SLOTS = 8;  // a ResGatedGraphConv layer's canonical tensors (gnnb_resgated.h)
constexpr int GGNN_PARAM_SLOTS = 5; // a GatedGraphConv layer's canonical tensors (gnnb_ggnn.h)
constexpr int GGNN_MAX_STEPS = 8;
constexpr int RGCN_PARAM_SLOTS = 3; // an RGCNConv layer's canonical tensors (gnnb_rgcn.h)
constexpr int GAT1_PARAM_SLOTS = 4; // a GAT v1 layer's canonical tensors (gnnb_gatconv.h); two more with edge features (gnnb_gatconv_edge.h)

// One conv layer's canonical tensors p[] (in the order of include/gnnb_hip.h; an edge model's two behind GIN's four / PNA's six; a
// GATv2 model's six in gnnb_gat.h's order, lin_edge's weight behind them when it has edge features) and the derived forms its conv type has, pushed in the order of LayerSlots' comment ->
// their offsets in the image
inline LayerOffsets push_conv_layer(WeightImage &im, const gnnb_model_desc &d, int l, const float *const *p, int edge_dim, int gat_heads = 0,
                                    int tf_heads = 0, bool gated = false, int gat1_heads = 0, int ggnn_steps = 0, int rgcn_relations = 0)
{
    const LayerDims ld = layer_dims(d, l);
    const size_t fi = ld.fin, fo = ld.fout;
    if (rgcn_relations > 0) { // (a GIN description whose layers are RGCNConv's; canonical order: weight, root, bias)
        LayerOffsets g;
        g.w_rgcn = im.push(rgcn_stack(p[0], p[1], (size_t)rgcn_relations, fi, fo));
        std::vector<float> b(((size_t)rgcn_relations + 1) * fo, 0.0f);
        memcpy(&b[(size_t)rgcn_relations * fo], p[2], fo * sizeof(float));
        g.b_rgcn = im.push(b);
        return g;
    }
    if (ggnn_steps > 0) { // (a GIN description whose layers are GatedGraphConv's; canonical order: weight, rnn.weight_ih, rnn.weight_hh,
                          // rnn.bias_ih, rnn.bias_hh; fi <= fo by gnnb_ggnn_model_create's check)
        LayerOffsets g;
        g.w_ggc = im.push(ggnn_fold(p[0], p[1], p[2], fo, fi));
        if (ggnn_steps > 1) {
            std::vector<float> next((size_t)(ggnn_steps - 1) * ggnn_step_stride(fo), 0.0f);
            for (int t = 1; t < ggnn_steps; t++) {
                const std::vector<float> f = ggnn_fold(p[0] + (size_t)t * fo * fo, p[1], p[2], fo, fo);
                memcpy(&next[(size_t)(t - 1) * ggnn_step_stride(fo)], f.data(), f.size() * sizeof(float));
            }
            g.w_ggc_next = im.push(next);
        }
        std::vector<float> b(6 * fo, 0.0f);
        memcpy(&b[3 * fo], p[4], 3 * fo * sizeof(float));
        g.b_ggc = im.push(b);
        g.b_ih = im.push(p[3], 3 * fo);
        return g;
    }
    if (gat1_heads > 0) { // (a GCN description whose layers are GAT v1's; canonical order: lin.weight, att_src, att_dst, bias)
        LayerOffsets g;
        g.w_gat = im.push(gat_score_fold(p[0], p[1], p[2], fi, fo, (size_t)gat1_heads));
        g.gat_bias = im.push(p[3], fo);
        if (edge_dim > 0) // (... with edge features, gnnb_gatconv_edge.h: att_edge and lin_edge.weight behind the four)
            g.a_edge = im.push(gat_edge_fold(p[5], p[4], (size_t)edge_dim, fo, (size_t)gat1_heads));
        return g;
    }
    if (gated) { // (a GIN description whose layers are ResGatedGraphConv's; canonical order: key, query, value, skip weight, conv.bias)
        LayerOffsets g;
        if (edge_dim > 0) { // (... with edge features, gnnb_resgated_edge.h: the same eight, key / query / value [fo, fi + edge_dim])
            const size_t ed = (size_t)edge_dim;
            const std::vector<float> kx = resgated_x_cols(p[0], fi, fo, ed), qx = resgated_x_cols(p[2], fi, fo, ed),
                                     vx = resgated_x_cols(p[4], fi, fo, ed);
            g.w_kqvr = im.push(stack_rows({kx.data(), qx.data(), vx.data(), p[6]}, fo, fi));
            g.b_kqvr = im.push(stack_rows({p[1], p[3], p[5], p[7]}, fo, 1));
            g.w_gv_edge = im.push(resgated_edge_blocks(p[0], p[2], p[4], fi, fo, ed));
            return g;
        }
        g.w_kqvr = im.push(stack_rows({p[0], p[2], p[4], p[6]}, fo, fi));
        g.b_kqvr = im.push(stack_rows({p[1], p[3], p[5], p[7]}, fo, 1));
        return g;
    }
    if (tf_heads > 0 && edge_dim > 0) { // (... with edge features: lin_edge's weight behind the eight; the folded query block)
        LayerOffsets g;
        const WeightBias qe = transformer_edge_fold(p[2], p[3], p[8], fi, fo, (size_t)tf_heads, (size_t)edge_dim);
        std::vector<float> w = stack_rows({p[2], p[0], p[4], p[6]}, fo, fi), b = stack_rows({p[3], p[1], p[5], p[7]}, fo, 1);
        w.insert(w.end(), qe.w.begin(), qe.w.end());
        b.insert(b.end(), qe.b.begin(), qe.b.end());
        g.w_qkvre = im.push(w);
        g.b_qkvre = im.push(b);
        g.w_edge = im.push(p[8], fo * (size_t)edge_dim);
        return g;
    }
    if (tf_heads > 0) { // (a GIN description whose layers are TransformerConv's; canonical order: key, query, value, skip)
        LayerOffsets g;
        g.w_qkvr = im.push(stack_rows({p[2], p[0], p[4], p[6]}, fo, fi));
        g.b_qkvr = im.push(stack_rows({p[3], p[1], p[5], p[7]}, fo, 1));
        return g;
    }
    if (gat_heads > 0) { // (a GCN description whose layers are GATv2's)
        LayerOffsets g;
        g.w_lr = im.push(gat_stack_rows(p[0], p[2], fo, fi));
        g.b_lr = im.push(gat_stack_rows(p[1], p[3], fo, 1));
        g.att = im.push(p[4], fo);
        g.gat_bias = im.push(p[5], fo);
        if (edge_dim > 0)
            g.w_edge = im.push(p[6], fo * (size_t)edge_dim);
        return g;
    }
    // the layer's skip connection (middle layers: y = conv(x) + x, models.py:562-564) where x itself is an operand of
    // the layer's GEMM (GraphSAGE's root term, PNA's x segment): folded into that operand's weights as + I, so that the
    // [N, out] skip operand is not read again in the epilogue (45 of 293 us of a 128-wide PNA layer's GEMM went there:
    // 32-byte pieces of 128-byte lines)
    const bool skip_fold = d.skip && l != 0 && l != d.num_layers - 1 && fi == fo && !im.fpx;
    LayerOffsets off;
    switch (d.conv_type) {
    case GNNB_CONV_GCN:
        off.w0 = im.push(p[0], fo * fi);
        off.b0 = im.push(p[1], fo);
        break;
    case GNNB_CONV_GIN: // hidden = out_channels (models.py:90)
        off.w0 = im.push(p[0], fo * fi);
        off.b0 = im.push(p[1], fo);
        off.w1 = im.push(p[2], fo * fo);
        off.b1 = im.push(p[3], fo);
        if (edge_dim > 0) {
            off.edge_w = im.push(p[4], fi * (size_t)edge_dim);
            off.edge_b = im.push(p[5], fi);
        }
        break;
    case GNNB_CONV_SAGE: // {Wl, bl, Wr}
        off.w_cat = im.push(sage_cat_weights(p[0], p[2], fo, fi, false));
        off.b_cat = im.push(p[1], fo);
        if (skip_fold)
            off.w_cat_skip = im.push(sage_cat_weights(p[0], p[2], fo, fi, true));
        break;
    case GNNB_CONV_PNA:
        off.w_pre = im.push(p[0], fi * (edge_dim > 0 ? 3 : 2) * fi);
        off.b_pre = im.push(p[1], fi);
        off.w_post = im.push(p[2], fo * 13 * fi);
        off.b_post = im.push(p[3], fo);
        off.w_lin = im.push(p[4], fo * fo);
        off.b_lin = im.push(p[5], fo);
        if (!im.fpx) {
            const WeightBias folded = pna_fold_lin(p[2], p[3], p[4], p[5], fi, fo, skip_fold);
            off.w_fold = im.push(folded.w);
            off.b_fold = im.push(folded.b);
            if (edge_dim > 0) { // (behind a three-block pre-NN: p[6], p[7] = conv.edge_encoder; no degree-class form)
                const WeightBias proj = pna_edge_projection(p[0], p[6], p[7], fi, (size_t)edge_dim);
                off.edge_w = im.push(proj.w);
                off.edge_b = im.push(proj.b);
            } else if (fo > 32) { // (any input width: whole 32-wide chunks take k_linear_dma's row-class mode, others the generic kernel's)
                const WeightBias classes = pna_degree_class_weights(folded, p[0], p[1], fi, fo, d.pna_delta);
                off.w_class = im.push(classes.w);
                off.b_class = im.push(classes.b);
            }
        }
        break;
    }
    return off;
}

struct BuiltWeights {
    std::vector<float> img;
    WeightLayout layout;
};

// The blob of a validated description (gnnb_model_create's checks have passed; edge_dim > 0: a GINE or PNA edge model) from the caller's
// tensors in canonical order, and where everything is in it.  Blob order: conv layers (canonical + derived tensors), k_gcn2_zf's
// fragment copy, the GIN stack's copies, the head.  gat_heads > 0: a GATv2 model (a GCN description, six tensors per layer; no
// fragment copy -- it takes no stack kernel); with edge_dim > 0 besides, GATv2 with edge features (seven tensors per layer).
// tf_heads > 0: a TransformerConv model (a GIN description, eight tensors per layer; no execution-order copy -- no stack kernel);
// with edge_dim > 0 besides, TransformerConv with edge features (nine tensors per layer).  gated: a ResGatedGraphConv model (a GIN
// description, eight tensors per layer; no execution-order copy either); with edge_dim > 0 besides, ResGatedGraphConv with edge
// features (the same eight, three of them [out, in + edge_dim]).  gat1_heads > 0: a GAT v1 model (a GCN description, four tensors
// per layer; no fragment copy -- it takes no stack kernel); with edge_dim > 0 besides, GAT v1 with edge features (six tensors per
// layer).  ggnn_steps > 0: a GatedGraphConv model (a GIN description, five tensors per layer; no execution-order copy).
// rgcn_relations > 0: an RGCNConv model (a GIN description, three tensors per layer; no execution-order copy).
inline BuiltWeights build_weight_image(const gnnb_model_desc &d, int edge_dim, const float *const *host_params, int gat_heads = 0,
                                       int tf_heads = 0, bool gated = false, int gat1_heads = 0, int ggnn_steps = 0, int rgcn_relations = 0)
{
    WeightImage im(d);
    WeightLayout lo;
    lo.conv.resize(d.num_layers);
    const int slots = rgcn_relations > 0 ? RGCN_PARAM_SLOTS
                      : ggnn_steps > 0 ? GGNN_PARAM_SLOTS
                      : gat1_heads > 0 ? GAT1_PARAM_SLOTS + (edge_dim ? 2 : 0)
                      : gated         ? RG_PARAM_SLOTS
                      : tf_heads > 0  ? TF_PARAM_SLOTS + (edge_dim ? 1 : 0)
                      : gat_heads > 0 ? GAT_PARAM_SLOTS + (edge_dim ? 1 : 0)
                                      : conv_slots(d.conv_type) + (edge_dim ? 2 : 0);
    int pi = 0;
    for (int l = 0; l < d.num_layers; l++, pi += slots)
        lo.conv[l] = push_conv_layer(im, d, l, host_params + pi, edge_dim, gat_heads, tf_heads, gated, gat1_heads, ggnn_steps, rgcn_relations);
    const bool have_w1f = gat_heads == 0 && gat1_heads == 0 && d.conv_type == GNNB_CONV_GCN && d.num_layers == 2 && d.hidden_dim % 16 == 0 && d.hidden_dim <= 128 && d.out_dim <= 128;
    if (have_w1f) // (from the image copy: already on the fixed-point grid when fpx is set; push() quantising again is harmless -- the grid is idempotent)
        lo.zf_w1f = im.push(zf_fragment_order(&im.img[lo.conv[1].w0], d.hidden_dim, d.out_dim));
    // (a GINE model, a TransformerConv model, a ResGatedGraphConv model, a GatedGraphConv model, an RGCNConv model take no stack
    // kernel: no execution-order copy)
    const bool have_gin = edge_dim == 0 && tf_heads == 0 && !gated && ggnn_steps == 0 && rgcn_relations == 0 && d.conv_type == GNNB_CONV_GIN && d.num_layers >= 2 && (d.hidden_dim == 32 || d.hidden_dim == 64 || d.hidden_dim == 128) &&
                          d.out_dim <= d.hidden_dim && d.out_dim % 4 == 0;
    if (have_gin) {
        const WeightBias g = gin_execution_order(d, im.img, lo.conv);
        lo.gin_w = im.push(g.w);
        lo.gin_b = im.push(g.b);
    }
    for (int i = 0; i < d.mlp_num_linear; i++, pi += 2) {
        int din, dout;
        mlp_dims(d, i, &din, &dout);
        lo.head_w.push_back(im.push(host_params[pi], (size_t)din * dout));
        lo.head_b.push_back(im.push(host_params[pi + 1], (size_t)dout));
    }
    return {std::move(im.img), std::move(lo)};
}

} // namespace gnnb
