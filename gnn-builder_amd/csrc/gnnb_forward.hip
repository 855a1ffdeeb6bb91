// gnnb_forward.hip -- the forward of libgnnb_hip.so: WHICH kernels of k_*.hip a forward runs, in which order and on which
// stream.  Host only, no kernels.  (gnnb_runtime.hip: errors, options, workspace, graph prep, the stage entry points;
// gnnb_ingest.hip: the PyG mini-batch entries, which end in forward_batched_tail.)
//
// Sequencing follows the reference's generated top (gnnbuilder/templates/model.cpp.jinja):
//   compute_gnn_head (:151-359)                -> the stack kernels, or per layer: k_aggregate + k_linear (+skip +act fused)
//   compute_global_graph_pooling (:413-449)    -> k_global_pool, or the epilogue of the last layer's GEMM
//   compute_mlp_head (:454-530)                -> the readout kernels, or a k_linear chain
// Every choice is a LADDER of rungs: a rung is a launcher that may decline (hipErrorNotSupported: nothing launched), and then
// the next rung is tried.  One conv layer is one function (gcn_layer .. pna_layer), the readout behind the layers one ladder
// (readout_layerwise); a new form is one function and one GNNB_RUNG line.
#include <cstring>
#include <vector>

#include "gnnb_host.h"

using namespace gnnb;

// One rung: the launcher ran -- GNNB_OK; it launched nothing and the next form is tried -- DECLINED (hipErrorNotSupported); or
// it failed -- GNNB_ERR_HIP, with "<what> launch failed: ..." as the error text.  DECLINED is no gnnb_status (those are <= 0).
enum { DECLINED = 1 };
static int attempt(hipError_t he, const char *what)
{
    if (he == hipSuccess)
        return GNNB_OK;
    if (he == hipErrorNotSupported)
        return DECLINED;
    return fail(GNNB_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(he));
}
// ... in a ladder: whatever the rung did ends the enclosing function, unless it declined
#define GNNB_RUNG(expr)                                                                           \
    do {                                                                                          \
        const int _rung = (expr);                                                                 \
        if (_rung != DECLINED)                                                                    \
            return _rung;                                                                         \
    } while (0)

// one plain GEMM; sk: the calling workspace's stream-K scratch, nullptr: the stand-alone entry's (per (device, stream))
static int linear1(const StreamK *sk, const float *a, int lda, int k, const float *w, int ldw, const float *bias, const float *skip,
                   float *y, int M, int N, int act, void *stream)
{
    gnnb_gemm_seg seg = {a, nullptr, lda, k};
    return linear_segs(sk, &seg, 1, w, ldw, bias, skip, y, M, N, act, stream);
}

// fixed-point emulation only: put a finished tensor on the model's ap_fixed<W, I> grid
static int quantize(const gnnb_model_desc &d, float *buf, size_t n, void *stream)
{
    if (d.fpx_w <= 0)
        return GNNB_OK;
    GNNB_HIP_TRY(launch_quantize(buf, buf, n, d.fpx_w, d.fpx_i, (hipStream_t)stream));
    return GNNB_OK;
}

// global pooling in the epilogue of the last conv layer's GEMM: into ws->pooled, by the model's pools
static PoolEpilogue pool_epilogue(const gnnb_workspace *ws, const gnnb_model_desc &d)
{
    PoolEpilogue pe;
    pe.node_graph = ws->t.node_graph;
    pe.graph_ptr = ws->t.graph_ptr;
    pe.pooled = ws->pooled;
    pe.part = ws->pool_part;
    pe.num_graphs = ws->t.num_graphs;
    pe.np = d.num_pools;
    for (int k = 0; k < 3; k++)
        pe.pools[k] = k < d.num_pools ? d.pools[k] : 0;
    return pe;
}

// Middle layers of a GCN stack for the fused kernel: every one hidden -> hidden, weights / biases at one constant
// stride in the model blob (it is laid out layer by layer, so they are -- checked, not assumed).  nl = 0: not eligible.
static G2Deep gcn_stack_middle_layers(const gnnb_model *model)
{
    const gnnb_model_desc &d = model->desc;
    G2Deep g;
    g.nl = 0;
    const int L = d.num_layers;
    // a GINE model: no stack kernel forms the edge term; a GATv2 model, a GAT v1 model, a TransformerConv model: none forms
    // attention; a ResGatedGraphConv model: none forms the gate; a GatedGraphConv model: none forms the GRU cell; an RGCNConv
    // model: none selects a weight by relation
    if (model->edge_dim || model->gat_heads || model->gat1_heads || model->tf_heads || model->gated || model->ggnn_steps || model->rgcn_relations)
        return g;
    if (d.conv_type == GNNB_CONV_GIN && L >= 2 && L <= GNNB_MAX_LAYERS && model->gin_w && model->gin_b) {
        // (the execution-order copy made at upload: one stride by construction, the last layer padded to hidden x hidden)
        g.wmid = model->gin_w;
        g.bmid = model->gin_b;
        g.mid_stride = (long)d.hidden_dim * d.hidden_dim;
        g.bmid_stride = (long)d.hidden_dim;
        g.gin = 1;
        g.eps = d.gin_eps;
        g.skip = d.skip ? 1 : 0;
        g.nl = L;
        return g;
    }
    if (d.conv_type != GNNB_CONV_GCN || L < 2 || L > GNNB_MAX_LAYERS)
        return g;
    if (L > 2) {
        g.wmid = model->conv[1].w0;
        g.bmid = model->conv[1].b0;
        if (L > 3) {
            g.mid_stride = (long)(model->conv[2].w0 - model->conv[1].w0);
            g.bmid_stride = (long)(model->conv[2].b0 - model->conv[1].b0);
        }
        for (int l = 1; l + 1 < L; l++)
            if (model->conv[l].w0 != g.wmid + (long)(l - 1) * g.mid_stride || model->conv[l].b0 != g.bmid + (long)(l - 1) * g.bmid_stride)
                return g;
    }
    g.skip = d.skip ? 1 : 0;
    g.nl = L;
    return g;
}

// What every layer loop decides in front of a layer's kernels.  Ping-pong: layer l writes ws->act[which], never the buffer it
// reads.  Skip connection: on middle layers only (models.py:562-564); fused into the GEMM epilogue.
struct LayerIO {
    float *nxt;
    const float *skip;
};
static LayerIO layer_io(const gnnb_model_desc &d, gnnb_workspace *ws, int l, const float *cur, int &which)
{
    if ((const float *)ws->act[which] == cur)
        which ^= 1;
    const LayerIO io = {ws->act[which], (d.skip && l != 0 && l != d.num_layers - 1) ? cur : nullptr};
    which ^= 1; // (the next layer's)
    return io;
}

// One conv layer of run_conv_layers on the node rows [row_lo, row_lo + M) of the prepared batch: filled by its loop, read by
// the four layer functions.  Aggregations index the batch-global buffers (sources are batch-global ids) and walk the tiles
// from tv.tile_lo; the GEMMs take the row range as a pointer offset (rows()).
struct LayerCtx {
    const gnnb_model *model;
    gnnb_workspace *ws;
    void *stream;
    int row_lo, M;
    bool whole;        // row_lo == 0: the forms that take the whole batch only may run
    BatchTables tv;    // ws->t from the row range's first tile
    const StreamK *sk; // this workspace's stream-K scratch (unlike the stand-alone gnnb_linear's)
    bool fpx;
    bool *pooled;      // non-null: the caller accepts ws->pooled in place of the last layer's output; set by try_pooling_gemm
    bool *mean_ready;  // GraphSAGE: ws->agg already holds mean_j of this layer's input rows (k_sage_first_mean, the layer before)
    const float *edge_attr; // GINE: the batch's [E, edge_dim] edge attributes in COO row order (nullptr: a model without)
    int l, fi, fo;
    bool last;
    const float *cur;  // the layer's input [N, fi] ...
    float *nxt;        // ... and output [N, fo]
    const float *skip; // cur on a middle layer of a model with skip connections
    bool skip_fold;    // (GraphSAGE / PNA: the derived weights of such a layer (w_cat_skip, w_fold, w_class) carry the skip connection as + I on x's own weights: gnnb_model_create)

    hipStream_t hs() const { return (hipStream_t)stream; }
    // the row range of a [N, width] matrix
    const float *rows(const float *p, int width) const { return p ? p + (size_t)row_lo * width : p; }
    float *rows(float *p, int width) const { return p ? p + (size_t)row_lo * width : p; }
    // the layer's GEMMs over the row range, on the workspace's scratch: y[M, N] = act(segments . w^T + bias + skip_rows)
    int linear(const gnnb_gemm_seg *segs, int num_segs, const float *w, int ldw, const float *bias, const float *skip_rows, float *y, int N, int act) const
    {
        return linear_segs(sk, segs, num_segs, w, ldw, bias, skip_rows, y, M, N, act, stream);
    }
    int linear1(const float *a, int k, const float *w, int ldw, const float *bias, const float *skip_rows, float *y, int N, int act) const
    {
        return ::linear1(sk, a, k, k, w, ldw, bias, skip_rows, y, M, N, act, stream);
    }
    int aggregate(int kind, const float *x, const float *selfq, float *out, int w, float eps) const
    {
        if (M <= 0)
            return GNNB_OK;
        if (kind == GNNB_AGG_GCN) {
            const int rc = ensure_gcoef(ws, stream);
            if (rc != GNNB_OK)
                return rc;
        }
        GNNB_HIP_TRY(launch_aggregate(tv, kind, x, selfq, out, w, eps, hs()));
        return GNNB_OK;
    }
};

// A rung of GraphSAGE's and PNA's LAST layer in a whole-batch run: global pooling in the epilogue of the layer's GEMM -- its
// [N, out] output is never written and the separate pooling pass (a full read of it) disappears (reference: compute_gnn_head's
// last layer + compute_global_graph_pooling, templates/model.cpp.jinja:151-449).  Declines when the caller wants the node
// matrix, and when the GEMM shape has no such epilogue.
static int try_pooling_gemm(const LayerCtx &c, const gnnb_gemm_seg *segs, int num_segs, const float *w, int ldw, const float *bias)
{
    if (!(c.pooled && c.whole && c.last && !c.fpx && options().fuse_pool && c.ws->t.node_graph && c.ws->pool_part))
        return DECLINED;
    const gnnb_model_desc &d = c.model->desc;
    GemmArgs g;
    int rc = build_gemm(g, segs, num_segs, w, ldw);
    if (rc != GNNB_OK)
        return rc;
    const PoolEpilogue pe = pool_epilogue(c.ws, d);
    rc = attempt(launch_linear(g, w, ldw, bias, nullptr, c.nxt, c.M, c.fo, d.activation, c.hs(), &pe), "pooling GEMM");
    if (rc != GNNB_OK)
        return rc;
    GNNB_HIP_TRY(launch_pool_combine(pe, c.M, c.fo, c.hs()));
    *c.pooled = true;
    return GNNB_OK;
}

static int gcn_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo;
    int rc;
    // aggregate at the input width, then transform (the reference's order, lib:1346-1379)
    if (c.whole && options().fuse_narrow && fi <= 32)
        GNNB_RUNG(attempt(launch_conv_gather(c.ws->t, GNNB_AGG_GCN, 0.f, c.cur, fi, fi, p.w0, fi, p.b0, c.skip, c.nxt, fo, d.activation, c.hs()),
                          "fused narrow conv"));
    if ((rc = c.aggregate(GNNB_AGG_GCN, c.cur, nullptr, c.ws->agg, fi, 0.f)))
        return rc;
    return c.linear1(c.rows(c.ws->agg, fi), fi, p.w0, fi, p.b0, c.rows(c.skip, fi), c.rows(c.nxt, fo), fo, d.activation);
}

// GATv2 (gnnb_gat.h; a GCN description with heads beside it): ONE GEMM x -> [xl | xr] [N, 2 fo] on the stacked weight [W_l ; W_r] in
// the model's math mode, then ONE k_gatv2_aggregate launch -- scores, softmax and weighted sum in one pass over the edges, with
// the bias, the skip term and the activation in its epilogue (no GEMM follows the aggregate here).  None of the fused rungs
static int gat_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo;
    float *lr = c.ws->tmp0;
    int rc;
    if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_lr, fi, p.b_lr, nullptr, c.rows(lr, 2 * fo), 2 * fo, GNNB_ACT_NONE)))
        return rc;
    // (always the whole batch: such a model takes no stack kernel, so no large segment runs beside one)
    if (c.M > 0 && c.model->edge_dim) // with edge features (gnnb_gat_edge.h): lin_edge's projection of the batch's edge attributes, inside the score
        GNNB_HIP_TRY(launch_gatv2_edge_aggregate(c.tv, lr, 2 * fo, lr + fo, 2 * fo, p.att, p.gat_bias, c.skip, d.activation, c.model->gat_heads,
                                                 c.model->gat_slope, c.edge_attr, c.model->edge_dim, p.w_edge, c.model->edge_dim, c.nxt, fo,
                                                 c.hs()));
    else if (c.M > 0)
        GNNB_HIP_TRY(launch_gatv2_aggregate(c.tv, lr, 2 * fo, lr + fo, 2 * fo, p.att, p.gat_bias, c.skip, d.activation, c.model->gat_heads,
                                            c.model->gat_slope, c.nxt, fo, c.hs()));
    return GNNB_OK;
}

// GAT v1 (gnnb_gatconv.h; a GCN description with heads beside it): ONE GEMM x -> [xl | s_src | s_dst | pad] [N, fo + roundup4(2 heads)]
// on w_gat = [W ; A_src W ; A_dst W ; 0] in the model's math mode, without a bias -- both per-node scores are linear in x, so att is
// folded into the weight at upload and they cost 2 heads more output columns --, then ONE k_gat_aggregate launch: leaky_relu of the
// sum of two scalars per (edge, head), softmax and weighted sum in one pass over the edges, with the bias, the skip term and the
// activation in its epilogue.  None of the fused rungs
static int gat1_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo, heads = c.model->gat1_heads;
    const int ld = fo + (int)gat_score_rows(heads);
    float *xs = c.ws->tmp0;
    int rc;
    if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_gat, fi, nullptr, nullptr, c.rows(xs, ld), ld, GNNB_ACT_NONE)))
        return rc;
    if (c.M > 0 && c.model->edge_dim) // with edge features (gnnb_gatconv_edge.h): the same GEMM; the batch's edge attributes enter the
                                      // score through the layer's folded a_edge [heads, roundup4(edge_dim)], d FMAs per (edge, head)
        GNNB_HIP_TRY(launch_gat_edge_aggregate(c.tv, xs, ld, xs + fo, ld, xs + fo + heads, ld, p.gat_bias, c.skip, d.activation, heads,
                                               c.model->gat_slope, c.edge_attr, c.model->edge_dim, p.a_edge,
                                               (int)gat_edge_cols(c.model->edge_dim), c.nxt, fo, c.hs()));
    else if (c.M > 0) // (always the whole batch: such a model takes no stack kernel, so no large segment runs beside one)
        GNNB_HIP_TRY(launch_gat_aggregate(c.tv, xs, ld, xs + fo, ld, xs + fo + heads, ld, p.gat_bias, c.skip, d.activation, heads,
                                          c.model->gat_slope, c.nxt, fo, c.hs()));
    return GNNB_OK;
}

// TransformerConv (gnnb_transformer.h; a GIN description with heads beside it, so the tables keep explicit (v, v) edges): ONE GEMM
// x -> [q | k | v | r] [N, 4 fo] on the stacked weight [W_q ; W_k ; W_v ; W_skip] in the model's math mode (the GEMM launch plan
// tiles N: 4 fo up to 1024 is one launch), then ONE k_transformer_aggregate launch -- dot-product scores, softmax and the weighted
// sum of the value rows in one pass over the edges, with the root term, the skip term and the activation in its epilogue.  None of
// the fused rungs.
// With edge features (gnnb_transformer_edge.h): the GEMM's weight carries the folded block W_qe behind the four, so the ONE GEMM
// gives x -> [q | k | v | r | qe] [N, ld], ld = 4 fo + roundup4(heads edge_dim) (at most 1024 + 128 columns: still one launch,
// the plan tiles N and walks the column tiles of any width), and the ONE launch is k_transformer_edge_aggregate, which takes qe
// beside q and lin_edge's raw weight for its epilogue
static int transformer_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo, heads = c.model->tf_heads;
    float *qkvr = c.ws->tmp0;
    int rc;
    if (const int ed = c.model->edge_dim) {
        const int ld = 4 * fo + (int)transformer_edge_qe_rows(heads, ed);
        if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_qkvre, fi, p.b_qkvre, nullptr, c.rows(qkvr, ld), ld, GNNB_ACT_NONE)))
            return rc;
        const float scale = 1.0f / std::sqrt((float)(fo / heads));
        if (c.M > 0)
            GNNB_HIP_TRY(launch_transformer_edge_aggregate(c.tv, qkvr, ld, qkvr + fo, ld, qkvr + 2 * fo, ld, qkvr + 4 * fo, ld, qkvr + 3 * fo, ld,
                                                           c.skip, d.activation, heads, scale, c.edge_attr, ed, p.w_edge, ed, c.nxt, fo, c.hs()));
        return GNNB_OK;
    }
    if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_qkvr, fi, p.b_qkvr, nullptr, c.rows(qkvr, 4 * fo), 4 * fo, GNNB_ACT_NONE)))
        return rc;
    const float scale = 1.0f / std::sqrt((float)(fo / heads)); // (once on the host: the kernel multiplies each score by it)
    if (c.M > 0) // (always the whole batch: such a model takes no stack kernel, so no large segment runs beside one)
        GNNB_HIP_TRY(launch_transformer_aggregate(c.tv, qkvr, 4 * fo, qkvr + fo, 4 * fo, qkvr + 2 * fo, 4 * fo, qkvr + 3 * fo, 4 * fo, c.skip,
                                                  d.activation, heads, scale, c.nxt, fo, c.hs()));
    return GNNB_OK;
}

// ResGatedGraphConv (gnnb_resgated.h; a GIN description with the "gated" mark beside it, so the tables keep explicit (v, v) edges):
// ONE GEMM x -> [k | q | v | r] [N, 4 fo] on the stacked weight [W_k ; W_q ; W_v ; W_skip] in the model's math mode (conv.bias
// rides as the skip block's GEMM bias), then ONE k_resgated_aggregate launch -- the per-column sigmoid gate and the gated sum of
// the value rows in one pass over the edges, with the root term, the skip term and the activation in its epilogue.  None of the
// fused rungs.  With edge features (gnnb_resgated_edge.h): the same GEMM on the x column blocks, then ONE
// k_resgated_edge_aggregate launch, which forms both edge terms from the batch's edge attributes and w_gv_edge = [W_g ; W_v]
static int resgated_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo;
    float *kqvr = c.ws->tmp0;
    int rc;
    if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_kqvr, fi, p.b_kqvr, nullptr, c.rows(kqvr, 4 * fo), 4 * fo, GNNB_ACT_NONE)))
        return rc;
    if (const int ed = c.model->edge_dim) {
        if (c.M > 0)
            GNNB_HIP_TRY(launch_resgated_edge_aggregate(c.tv, kqvr, 4 * fo, kqvr + fo, 4 * fo, kqvr + 2 * fo, 4 * fo, kqvr + 3 * fo, 4 * fo, c.skip,
                                                        d.activation, c.edge_attr, ed, p.w_gv_edge, ed, p.w_gv_edge + (size_t)fo * ed, ed, c.nxt,
                                                        fo, c.hs()));
        return GNNB_OK;
    }
    if (c.M > 0) // (always the whole batch: such a model takes no stack kernel, so no large segment runs beside one)
        GNNB_HIP_TRY(launch_resgated_aggregate(c.tv, kqvr, 4 * fo, kqvr + fo, 4 * fo, kqvr + 2 * fo, 4 * fo, kqvr + 3 * fo, 4 * fo, c.skip,
                                               d.activation, c.nxt, fo, c.hs()));
    return GNNB_OK;
}

// GatedGraphConv (gnnb_ggnn.h; a GIN description with `steps` beside it, so the tables keep explicit (v, v) edges): steps x (ONE GEMM
// h -> [p | gh] [N, 6 fo] on [W_p[t] ; weight_hh] with the bias [0 | bias_hh] in the model's math mode -- the message weight is
// folded into the GRU's input weight at upload --, then ONE k_ggnn_aggregate launch: the sum of the neighbours' p rows and the whole
// GRU cell in one pass over the edges).  Step 0 reads the layer's input at K = fi (h_0 = [x | 0]: the kernel takes h's columns from
// fi on as 0); the inner steps write the two [N, fo] state buffers in ws->tmp1 in turn, without skip term or activation; the last
// step writes the layer's output with both in its epilogue.  None of the fused rungs
static int ggnn_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo, steps = c.model->ggnn_steps;
    float *pg = c.ws->tmp0;
    // (tmp0 and tmp1 are [max_nodes, >= GGNN_TMP_BLOCKS fo], gnnb_host.h: room for [p | gh] and for both state buffers)
    float *state[2] = {c.ws->tmp1, c.ws->tmp1 + ggnn_state_offset((size_t)c.ws->t.num_nodes, (size_t)fo)};
    const float *h = c.cur;
    int hw = fi, rc;
    for (int t = 0; t < steps; t++) {
        const bool last = t == steps - 1;
        const float *w = t == 0 ? p.w_ggc : p.w_ggc_next + (size_t)(t - 1) * ggnn_step_stride(fo);
        if ((rc = c.linear1(c.rows(h, hw), hw, w, hw, p.b_ggc, nullptr, c.rows(pg, 6 * fo), 6 * fo, GNNB_ACT_NONE)))
            return rc;
        float *o = last ? c.nxt : state[t & 1];
        if (c.M > 0) // (always the whole batch: such a model takes no stack kernel, so no large segment runs beside one)
            GNNB_HIP_TRY(launch_ggnn_aggregate(c.tv, pg, 6 * fo, pg + 3 * fo, 6 * fo, h, hw, hw, p.b_ih, last ? c.skip : nullptr,
                                               last ? d.activation : GNNB_ACT_NONE, o, fo, c.hs()));
        h = o, hw = fo;
    }
    return GNNB_OK;
}

// RGCNConv (gnnb_rgcn.h; a GIN description with `relations` beside it, so the tables keep explicit (v, v) edges): ONE GEMM
// x -> [p_0 | .. | p_{R-1} | root] [N, (R + 1) fo] on w_rgcn with the bias [0 | .. | 0 | bias] in the model's math mode -- the
// per-relation transform is the GEMM's, the message is linear --, then ONE k_rgcn_aggregate launch on the slot records the _types
// forward built into ws->rgcn_rec: one gathered row-width per edge, the skip term and the activation in its epilogue.  None of
// the fused rungs
static int rgcn_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo, R = c.model->rgcn_relations, ld = rgcn_tmp_blocks(R) * fo;
    float *pr = c.ws->tmp0; // ([max_nodes, >= (R + 1) fo]: gnnb_workspace_create)
    int rc;
    if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_rgcn, fi, p.b_rgcn, nullptr, c.rows(pr, ld), ld, GNNB_ACT_NONE)))
        return rc;
    if (c.M > 0) // (always the whole batch: such a model takes no stack kernel, so no large segment runs beside one)
        GNNB_HIP_TRY(launch_rgcn_aggregate(c.tv, c.ws->rgcn_rec, pr, ld, R, pr + (size_t)R * fo, ld, c.skip, d.activation, c.nxt, fo, c.hs()));
    return GNNB_OK;
}

// GIN's first linear + ReLU on the eps-weighted sum -> ws->tmp0
static int gin_hidden(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo;
    int rc;
    if (c.model->edge_dim) {
        // GINE: the same layer with relu(x_j + W_e e_ij + b_e) as the message -- k_gine_aggregate forms the edge term on chip
        // (edge_w [fi, edge_dim], edge_b); none of the fused rungs, everything behind the aggregate is GIN's
        if (c.M > 0)
            GNNB_HIP_TRY(launch_gine_aggregate(c.tv, c.cur, c.edge_attr, c.model->edge_dim, p.edge_w, c.model->edge_dim, p.edge_b, c.ws->agg, fi,
                                               d.gin_eps, c.hs()));
        return c.linear1(c.rows(c.ws->agg, fi), fi, p.w0, fi, p.b0, nullptr, c.rows(c.ws->tmp0, fo), fo, GNNB_ACT_RELU);
    }
    if (c.whole && options().fuse_narrow && fi <= 32)
        GNNB_RUNG(attempt(launch_conv_gather(c.ws->t, GNNB_AGG_SUM, d.gin_eps, c.cur, fi, fi, p.w0, fi, p.b0, nullptr, c.ws->tmp0, fo, GNNB_ACT_RELU, c.hs()),
                          "fused narrow conv"));
    if ((rc = c.aggregate(GNNB_AGG_SUM, c.cur, nullptr, c.ws->agg, fi, d.gin_eps)))
        return rc;
    return c.linear1(c.rows(c.ws->agg, fi), fi, p.w0, fi, p.b0, nullptr, c.rows(c.ws->tmp0, fo), fo, GNNB_ACT_RELU);
}

static int gin_layer(const LayerCtx &c)
{
    const LayerWeights &p = c.model->conv[c.l];
    const int fo = c.fo;
    int rc;
    if ((rc = gin_hidden(c)))
        return rc;
    return c.linear1(c.rows(c.ws->tmp0, fo), fo, p.w1, fo, p.b1, c.rows(c.skip, fo), c.rows(c.nxt, fo), fo, c.model->desc.activation);
}

static int sage_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo;
    int rc;
    const bool narrow = c.whole && options().fuse_narrow && 2 * fi <= 32;
    if (narrow && !c.last && c.skip == nullptr && !c.fpx) {
        // narrow input AND a layer behind it: the stage's output rows stay in LDS and the next layer's mean aggregate is
        // taken from there -- its aggregate kernel (a full read and write of [N, fo]) is not run
        rc = attempt(launch_sage_first_mean(c.ws->t, c.cur, fi, p.w_cat, 2 * fi, p.b_cat, c.nxt, c.ws->agg, fo, d.activation, c.hs()), "first-layer + mean");
        if (rc == GNNB_OK)
            *c.mean_ready = true;
        GNNB_RUNG(rc);
    }
    if (narrow) // narrow input: [mean_j x_j | x_i] is produced inside the GEMM's A stage (K = 2 F_in)
        GNNB_RUNG(attempt(launch_conv_gather(c.ws->t, GNNB_AGG_MEAN, 0.f, c.cur, fi, 2 * fi, p.w_cat, 2 * fi, p.b_cat, c.skip, c.nxt, fo, d.activation, c.hs(), fi),
                          "fused narrow conv"));
    if (!*c.mean_ready && (rc = c.aggregate(GNNB_AGG_MEAN, c.cur, nullptr, c.ws->agg, fi, 0.f)))
        return rc;
    *c.mean_ready = false;
    gnnb_gemm_seg segs[2] = {{c.rows(c.ws->agg, fi), nullptr, fi, fi}, {c.rows(c.cur, fi), nullptr, fi, fi}};
    GNNB_RUNG(try_pooling_gemm(c, segs, 2, p.w_cat, 2 * fi, p.b_cat));
    if (c.skip_fold && p.w_cat_skip && options().fold_skip) // ([Wl | Wr + I])
        return c.linear(segs, 2, p.w_cat_skip, 2 * fi, p.b_cat, nullptr, c.rows(c.nxt, fo), fo, d.activation);
    return c.linear(segs, 2, p.w_cat, 2 * fi, p.b_cat, c.rows(c.skip, fi), c.rows(c.nxt, fo), fo, d.activation);
}

// PNA: the source half p = x . Wb^T and its aggregate -> ws->agg: in one kernel, p on chip, where the degree-class form (no
// destination term) and the max_graph_nodes promise (whole graphs in a stage) allow; else GEMM -> [N, F] -> aggregate
static int pna_source_aggregate(const LayerCtx &c, bool classes)
{
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi;
    float *q = c.ws->tmp0, *pp = c.ws->tmp1;
    int rc;
    if (classes)
        GNNB_RUNG(attempt(launch_pna_pagg(c.ws->t, c.cur, fi, p.w_pre + fi, 2 * fi, c.ws->agg, c.hs()), "PNA product + aggregate"));
    if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_pre + fi, 2 * fi, nullptr, nullptr, c.rows(pp, fi), fi, GNNB_ACT_NONE)))
        return rc;
    return c.aggregate(GNNB_AGG_PNA, pp, classes ? nullptr : q, c.ws->agg, fi, 0.f);
}

static int pna_layer(const LayerCtx &c)
{
    const gnnb_model_desc &d = c.model->desc;
    gnnb_workspace *const ws = c.ws;
    const LayerWeights &p = c.model->conv[c.l];
    const int fi = c.fi, fo = c.fo;
    const int edge_dim = c.model->edge_dim;
    const int ldpre = (edge_dim ? 3 : 2) * fi; // w_pre's row stride: [Wa | Wb], and | Wc of a model with edge features behind them
    int rc;
    // a narrow input (the first layer): the whole layer in one kernel, whole graphs staged in LDS (k_pna_first.hip)
    if (!edge_dim && c.whole && fi <= 12 && c.skip == nullptr && !c.fpx && p.w_fold && options().pna_fold_lin && ws->prep_delta == d.pna_delta)
        GNNB_RUNG(attempt(launch_pna_first(ws->t, c.cur, fi, p.w_pre, p.b_pre, p.w_fold, 13 * fi, p.b_fold, c.nxt, fo, d.activation, c.hs()), "narrow PNA layer"));
    // h_ij = Wpre [x_i || x_j] + b  ==  (Wpre[:, :F] x_i + b) + Wpre[:, F:] x_j
    float *q = ws->tmp0;
    // degree-class form (gnnb_workspace_set_max_degree; decided here: it folds the destination's pre-NN term into x's
    // class weights, so q is not computed and the aggregate runs without a destination term)
    // (the row-class GEMM addresses a row of its operands as a 32-bit byte offset on the operand's base, row * 16 fi
    // for the aggregate: the form applies while that stays below 2^32 -- 2^21 rows at fi = 128, 2^20 at fi = 256; larger
    // batches take the general form below, decided here, before anything of the layer is enqueued)
    const bool classes = !edge_dim && p.w_class && options().pna_fold_lin && options().pna_classes && c.whole && ws->deg_ready && c.M > 0 && !c.fpx &&
                         ws->deg_delta == d.pna_delta && fo > 32 && (uint64_t)c.M * 16 * fi + 512 <= 0xffffffffull;
    if (!classes && (rc = c.linear1(c.rows(c.cur, fi), fi, p.w_pre, ldpre, p.b_pre, nullptr, c.rows(q, fi), fi, GNNB_ACT_NONE)))
        return rc;
    if (edge_dim) {
        // PNA with edge features: h_ij = q_i + p_j + (W_e e_ij + b_e) -- the p GEMM, then k_pna_edge_aggregate forms the edge term on
        // chip (edge_w = Wc W_enc [fi, edge_dim], edge_b = Wc b_enc: gnnb_weights.h); none of the fused rungs, no class form;
        // everything behind the aggregate is PNA's
        float *pp = ws->tmp1;
        if ((rc = c.linear1(c.rows(c.cur, fi), fi, p.w_pre + fi, ldpre, nullptr, nullptr, c.rows(pp, fi), fi, GNNB_ACT_NONE)))
            return rc;
        if (c.M > 0)
            GNNB_HIP_TRY(launch_pna_edge_aggregate(c.tv, pp, q, c.edge_attr, edge_dim, p.edge_w, edge_dim, p.edge_b, ws->agg, fi, c.hs()));
    } else if ((rc = pna_source_aggregate(c, classes)))
        return rc;
    if (classes) {
        // degree-class form (gnnb_workspace_set_max_degree): [x | A] . W_class^T over the class-sorted rows, written to
        // the rows' own places; skip + activation in the epilogue (the last layer pools in the pass behind)
        gnnb_gemm_seg s2[2] = {{c.cur, nullptr, fi, fi}, {ws->agg, nullptr, 4 * fi, 4 * fi}};
        GemmArgs g;
        if ((rc = build_gemm(g, s2, 2, p.w_class, 5 * fi)))
            return rc;
        RowClasses rcl;
        rcl.perm = ws->deg_perm;
        rcl.tile_cls = ws->deg_tile_cls;
        rcl.w_stride = (long)fo * 5 * fi;
        rcl.bias_stride = fo;
        hipError_t he = launch_linear(g, p.w_class, 5 * fi, p.b_class, c.skip_fold ? nullptr : c.skip, c.nxt, ws->deg_max_tiles * 128, fo, d.activation,
                                      c.hs(), nullptr, &rcl, c.sk);
        if (he == hipSuccess)
            return GNNB_OK;
        // (no way back from here: the aggregate above ran without the destination term)
        return fail(GNNB_ERR_HIP, "degree-class GEMM launch failed: %s", hipGetErrorString(he));
    }
    // [x | A | amp.A | att.A] . Wpost^T without materialising the 13F concat
    gnnb_gemm_seg segs[4] = {{c.rows(c.cur, fi), nullptr, fi, fi},
                             {c.rows(ws->agg, 4 * fi), nullptr, 4 * fi, 4 * fi},
                             {c.rows(ws->agg, 4 * fi), ws->t.amp + c.row_lo, 4 * fi, 4 * fi},
                             {c.rows(ws->agg, 4 * fi), ws->t.att + c.row_lo, 4 * fi, 4 * fi}};
    if (p.w_fold && options().pna_fold_lin) {
        // `lin` folded into the post-NN at upload (gnnb_model_create): one GEMM, skip + activation in its epilogue;
        // the last layer of a whole-batch run pools there too (as GraphSAGE's; PNA's own condition: the pooling epilogue
        // takes no skip operand, and this GEMM would carry one)
        if (c.skip == nullptr)
            GNNB_RUNG(try_pooling_gemm(c, segs, 4, p.w_fold, 13 * fi, p.b_fold));
        return c.linear(segs, 4, p.w_fold, 13 * fi, p.b_fold, c.skip_fold ? nullptr : c.rows(c.skip, fo), c.rows(c.nxt, fo), fo, d.activation);
    }
    float *hid = ws->tmp0; // q is dead after the aggregate
    if ((rc = c.linear(segs, 4, p.w_post, 13 * fi, p.b_post, nullptr, c.rows(hid, fo), fo, GNNB_ACT_NONE)))
        return rc;
    return c.linear1(c.rows(hid, fo), fo, p.w_lin, fo, p.b_lin, c.rows(c.skip, fo), c.rows(c.nxt, fo), fo, d.activation);
}

// The conv layers one by one (gather-aggregate + GEMM kernels) on the node rows [row_lo, N) of the prepared batch:
// row_lo = 0 is the whole batch; row_lo > 0 the caller's large segment (gnnb_workspace_set_large_segment), whose first
// node tile is tile_lo.  *out_cur = the last layer's output matrix ([N, width], rows below row_lo untouched) -- unless
// pooled_in_epilogue is given and comes back true: the last layer's GEMM pooled into ws->pooled and wrote no node matrix.
// edge_attr: a GINE model's edge attributes (nullptr: a model without).
static int run_conv_layers(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr, int row_lo, int tile_lo,
                           const float **out_cur, void *stream, bool *pooled_in_epilogue = nullptr)
{
    if (pooled_in_epilogue)
        *pooled_in_epilogue = false;
    const gnnb_model_desc &d = model->desc;
    bool mean_ready = false;
    LayerCtx c = {model, ws, stream, row_lo, ws->t.num_nodes - row_lo, row_lo == 0, ws->t, ws->sk.part ? &ws->sk : nullptr, d.fpx_w > 0,
                  pooled_in_epilogue, &mean_ready, edge_attr};
    c.tv.tile_lo = tile_lo;
    c.cur = x_dev;
    int which = 0;
    for (c.l = 0; c.l < d.num_layers; c.l++) {
        const LayerDims ld = layer_dims(d, c.l);
        const LayerIO io = layer_io(d, ws, c.l, c.cur, which);
        c.fi = ld.fin;
        c.fo = ld.fout;
        c.last = c.l == d.num_layers - 1;
        c.nxt = io.nxt;
        c.skip = io.skip;
        c.skip_fold = c.skip != nullptr && c.fi == c.fo && !c.fpx;
        int rc = GNNB_OK;
        switch (d.conv_type) {
        case GNNB_CONV_GCN: rc = model->gat_heads ? gat_layer(c) : model->gat1_heads ? gat1_layer(c) : gcn_layer(c); break;
        case GNNB_CONV_GIN:
            rc = model->tf_heads ? transformer_layer(c) : model->gated ? resgated_layer(c) : model->ggnn_steps ? ggnn_layer(c)
                 : model->rgcn_relations                                                                                 ? rgcn_layer(c)
                                                                                                                         : gin_layer(c);
            break;
        case GNNB_CONV_SAGE: rc = sage_layer(c); break;
        case GNNB_CONV_PNA: rc = pna_layer(c); break;
        }
        if (rc != GNNB_OK)
            return rc;
        if ((rc = quantize(d, c.rows(c.nxt, c.fo), (size_t)c.M * c.fo, stream)))
            return rc;
        c.cur = c.nxt;
    }
    *out_cur = c.cur;
    return GNNB_OK;
}

// The large segment of the PREPARED batch: what graph prep validated against the batch and baked into its tables (t.promise_graphs,
// t.large_n, t.large_e; the device check behind flag 16), NOT the workspace's current setting -- gnnb_workspace_set_large_segment
// between a graph prep and its prepared forward names the segment of the NEXT prep, and everything below this line reads the
// split from here.  -1: the batch was prepared without one.
static int prepared_large_g(const gnnb_workspace *ws) { return ws->t.large_n >= 0 ? ws->t.promise_graphs : -1; }

// global pooling of the large segment's graphs [large_g, B) from the node matrix `cur` into their rows of ws->pooled
static hipError_t pool_large_segment(const gnnb_model *model, gnnb_workspace *ws, const float *cur, hipStream_t s)
{
    const gnnb_model_desc &d = model->desc;
    const int gw = gnn_out_width(d), large_g = prepared_large_g(ws);
    return launch_global_pool(cur, ws->t.graph_ptr + large_g, ws->t.num_graphs - large_g, gw, d.pools, d.num_pools,
                              ws->pooled + (size_t)large_g * d.num_pools * gw, s);
}

// The large segment through the small-footprint per-layer kernel (k_conv_rows) + pooling, all on stream `s`; fills
// ws->pooled rows [large_g, B).  hipErrorNotSupported (nothing launched) when a layer does not suit that kernel.
static hipError_t large_segment_small(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, hipStream_t s)
{
    const gnnb_model_desc &d = model->desc;
    if (d.conv_type != GNNB_CONV_GCN && d.conv_type != GNNB_CONV_GIN)
        return hipErrorNotSupported;
    for (int l = 0; l < d.num_layers; l++) {
        const LayerDims ld = layer_dims(d, l);
        if (ld.fin > 128 || ld.fout > 128)
            return hipErrorNotSupported;
    }
    if ((d.in_dim & 3) == 0 && (((uintptr_t)x_dev) & 15))
        return hipErrorNotSupported;
    const float *cur = x_dev;
    int which = 0;
    for (int l = 0; l < d.num_layers; l++) {
        const LayerDims ld = layer_dims(d, l);
        const LayerWeights &p = model->conv[l];
        const LayerIO io = layer_io(d, ws, l, cur, which);
        hipError_t he = launch_conv_rows(ws->t, d.conv_type, cur, ld.fin, p.w0, p.b0, p.w1, p.b1, // (GCN: no second linear)
                                         ld.fout, io.skip, io.nxt, ws->t.large_n, d.activation, d.gin_eps, s);
        if (he != hipSuccess)
            return he; // (NotSupported can only come from the first layer's checks above: nothing is half done)
        cur = io.nxt;
    }
    return pool_large_segment(model, ws, cur, s);
}

// The batch tables restricted to the graphs the max_graph_nodes promise covers: everything, or -- with a large segment --
// graphs [0, large_g) = nodes [0, large_n) = edges [0, large_e).  The stack kernels clamp every table entry to these
// counts, so a tile that begins in the small segment ends at its last node.  (The prepared batch's segment: graph prep calls this
// behind the lines that bake it, where it is the workspace's setting.)
BatchTables gnnb::small_segment(const gnnb_workspace *ws)
{
    BatchTables t = ws->t;
    const int large_g = prepared_large_g(ws);
    if (large_g >= 0 && large_g < t.num_graphs) {
        t.num_graphs = large_g;
        t.num_nodes = ws->t.large_n;
        t.num_edges = ws->t.large_e;
        t.num_tiles = (t.num_nodes + t.tile_rows - 1) / t.tile_rows;
    }
    return t;
}

// The LDS-resident conv stack + pooling for this model on the prepared batch -> ws->pooled.  hipErrorNotSupported when
// no stack kernel takes the model / batch (the caller runs layer by layer); *path says which kernel ran.
// head_out != nullptr: the stack kernel may run the MLP head on the graphs of `t` as well (k_gcn2_zf does when the head's
// activation is the conv stack's and its shape suits: *head_fused); out rows [0, t.num_graphs) are then complete
static hipError_t launch_conv_stack(const gnnb_model *model, gnnb_workspace *ws, const BatchTables &t, const float *x_dev,
                                    const G2Deep &deep, hipStream_t s, int *path, float *head_out = nullptr, bool *head_fused = nullptr)
{
    const gnnb_model_desc &d = model->desc;
    const int L = d.num_layers;
    hipError_t he = hipErrorNotSupported;
    if (head_fused)
        *head_fused = false;
    if (!deep.gin && L == 2) { // two GCN layers, fp32: the transform-first form with 96-row stages (k_stack_zf.h)
        const bool offer = head_out != nullptr && model->head_dev != nullptr && d.mlp_num_linear <= 8 && d.mlp_activation == d.activation;
        const HeadArgs head = model_head_args(model);
        he = launch_gcn2_zf(t, x_dev, d.in_dim, model->conv[0].w0, model->conv[0].b0, d.hidden_dim, model->conv[1].w0,
                            model->conv[1].b0, d.out_dim, d.activation, d.pools, d.num_pools, ws->pooled, s, model->zf_w1f,
                            offer ? &head : nullptr, offer ? model->head_dev : nullptr, offer ? head_out : nullptr, head_fused);
    }
    *path = GNNB_PATH_STACK_ZF;
    if (he == hipErrorNotSupported) {
        *path = GNNB_PATH_STACK;
        he = launch_gcn2_fused(t, x_dev, d.in_dim, model->conv[0].w0, model->conv[0].b0, d.hidden_dim,
                               model->conv[L - 1].w0, model->conv[L - 1].b0, d.out_dim, d.activation, d.pools,
                               d.num_pools, ws->pooled, s, deep);
    }
    return he;
}

// The head as a plain GEMM chain (a head too large for the readout kernels; the fixed-point emulation, each layer's output put
// on the grid).  On the stand-alone GEMM scratch: the head's GEMMs never use the workspace's stream-K scratch.
static int run_head_chain(const gnnb_model *model, gnnb_workspace *ws, int g0, float *out_dev, void *stream)
{
    const gnnb_model_desc &d = model->desc;
    const int M = ws->t.num_graphs - g0;
    const float *h = ws->pooled + (size_t)g0 * d.num_pools * gnn_out_width(d);
    for (int i = 0; i < d.mlp_num_linear; i++) {
        int din, dout, rc;
        mlp_dims(d, i, &din, &dout);
        const bool last = (i == d.mlp_num_linear - 1);
        float *y = last ? out_dev + (size_t)g0 * d.mlp_out : ws->mlp[i & 1];
        if ((rc = linear1(nullptr, h, din, din, model->head_w[i], din, model->head_b[i], nullptr, y, M, dout,
                          last ? GNNB_ACT_NONE : d.mlp_activation, stream)))
            return rc;
        if ((rc = quantize(d, y, (size_t)M * dout, stream)))
            return rc;
        h = y;
    }
    return GNNB_OK;
}

// The readout of graphs [g0, B) from a complete ws->pooled: in one launch, else the GEMM chain (no fixed-point emulation on
// this route).  what: the error text's name of the launch.
static int readout_from_pooled(const gnnb_model *model, gnnb_workspace *ws, int g0, float *out_dev, void *stream, const char *what = "readout")
{
    const gnnb_model_desc &d = model->desc;
    const int gw = gnn_out_width(d);
    GNNB_RUNG(attempt(launch_readout_pooled(ws->pooled + (size_t)g0 * d.num_pools * gw, ws->t.num_graphs - g0, gw, model_head_args(model), d.mlp_activation,
                                            out_dev + (size_t)g0 * d.mlp_out, (hipStream_t)stream), what));
    return run_head_chain(model, ws, g0, out_dev, stream);
}

// the pooling pass over the node matrix `cur`, unless ws->pooled is complete already; it is afterwards
static int ensure_pooled(const gnnb_model *model, gnnb_workspace *ws, const float *cur, bool *pooled, void *stream)
{
    const gnnb_model_desc &d = model->desc;
    if (*pooled)
        return GNNB_OK;
    const int rc = gnnb_global_pool(ws, cur, gnn_out_width(d), d.pools, d.num_pools, ws->pooled, stream);
    *pooled = rc == GNNB_OK;
    return rc;
}

// The readout behind run_conv_layers on the whole batch, as one ladder.  pooled: ws->pooled is complete (the last layer's
// GEMM pooled in its epilogue); else `cur` is the node matrix.
static int readout_layerwise(const gnnb_model *model, gnnb_workspace *ws, const float *cur, bool pooled, float *out_dev, void *stream)
{
    const gnnb_model_desc &d = model->desc;
    const int gw = gnn_out_width(d), B = ws->t.num_graphs;
    int rc;
    // the one-launch readouts: fp32 (the emulation quantises between the head's layers), a head a HeadArgs holds
    if (d.fpx_w <= 0 && d.mlp_num_linear <= 8) {
        if (pooled) // the readout takes ws->pooled as the stack path does
            return readout_from_pooled(model, ws, 0, out_dev, stream);
        if (options().head_split) {
            // pooling pass (HBM-bound, every CU) + the small readout on the pooled matrix: neither needs the
            // 119 KB of LDS of the one-launch form, so both share CUs with other batches' kernels
            if ((rc = ensure_pooled(model, ws, cur, &pooled, stream)))
                return rc;
            return readout_from_pooled(model, ws, 0, out_dev, stream, "fused readout");
        }
        // pooling + whole MLP head in one launch when the head fits LDS
        GNNB_RUNG(attempt(launch_readout_fused(cur, ws->t.graph_ptr, B, gw, d.pools, d.num_pools, model_head_args(model), d.mlp_activation, out_dev,
                                               (hipStream_t)stream), "fused readout"));
        if (readout_small_enabled()) {
            // The head's weights do not fit LDS (SAGE d = 256 with three pools: 768 x 64 floats): pooling pass, then
            // the small readout that takes its weights from L2 as MFMA operands -- one launch over B / 16 workgroups
            // instead of a chain of GEMMs with M = B rows (64 workgroups of the 128-row tile at B = 8192: 51 us)
            if ((rc = ensure_pooled(model, ws, cur, &pooled, stream)))
                return rc;
            return readout_from_pooled(model, ws, 0, out_dev, stream);
        }
    }
    // pooling pass, the pooled matrix on the fixed-point grid (fp32: nothing), GEMM chain
    if ((rc = ensure_pooled(model, ws, cur, &pooled, stream)))
        return rc;
    if ((rc = quantize(d, ws->pooled, (size_t)B * d.num_pools * gw, stream)))
        return rc;
    return run_head_chain(model, ws, 0, out_dev, stream);
}

// The side stream and its fork / join events, only for large_fork = 1 (the default, 2, never uses them): created on first
// use -- all three or none; a partial failure destroys what was created and the large segment stays on the caller's stream.
static bool ensure_side_stream(gnnb_workspace *ws)
{
    if (ws->side)
        return true;
    hipStream_t st = nullptr;
    hipEvent_t ef = nullptr, ej = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&ef, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&ej, hipEventDisableTiming) == hipSuccess) {
        ws->side = st;
        ws->ev_fork = ef;
        ws->ev_join = ej;
        return true;
    }
    (void)hipGetLastError();
    if (ej)
        (void)hipEventDestroy(ej);
    if (ef)
        (void)hipEventDestroy(ef);
    if (st)
        (void)hipStreamDestroy(st);
    return false;
}

// The whole GCN / GIN stack (two or more layers) + pooling in one persistent kernel on the graphs the promise covers, then the
// MLP head.  With a large segment (graphs the promise does not cover, ordered last by the caller) the stack runs on the graphs
// in front of it and the large ones go layer by layer into the same pooled matrix: one oversized molecule no longer sends the
// whole batch down the layer-by-layer path.  DECLINED: no stack kernel takes the model / batch.
static int forward_stack(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, float *out_dev, const G2Deep &deep, void *stream)
{
    const int B = ws->t.num_graphs, large_g = prepared_large_g(ws), large_n = ws->t.large_n;
    const bool seg = large_g >= 0 && large_g < B;
    int rc;
    // The large segment first, FORKED: its kernels are built to run beside the stack kernel (k_conv_rows.hip), so they
    // go on the workspace's side stream behind an event on the caller's stream and are joined in front of the readout.
    // (Capturable: the side stream joins a capture through the event and is joined back.)
    bool forked = false, side_forked = false;
    if (seg && options().large_fork == 1 && ensure_side_stream(ws)) {
        GNNB_HIP_TRY(hipEventRecord(ws->ev_fork, (hipStream_t)stream));
        GNNB_HIP_TRY(hipStreamWaitEvent(ws->side, ws->ev_fork, 0));
        side_forked = true;
        hipError_t hl = large_segment_small(model, ws, x_dev, ws->side);
        // (joined whether or not anything ran on the side stream -- also in front of the error return: a side stream
        // left forked would invalidate a capture in progress)
        const hipError_t hj = hipEventRecord(ws->ev_join, ws->side);
        if (hj != hipSuccess || (hl != hipSuccess && hl != hipErrorNotSupported)) {
            if (hj == hipSuccess)
                (void)hipStreamWaitEvent((hipStream_t)stream, ws->ev_join, 0);
            return fail(GNNB_ERR_HIP, "large-segment launch failed: %s", hipGetErrorString(hl != hipSuccess ? hl : hj));
        }
        forked = hl == hipSuccess;
    }
    bool head_fused = false;
    hipError_t he = launch_conv_stack(model, ws, small_segment(ws), x_dev, deep, (hipStream_t)stream, &ws->last_path, out_dev, &head_fused);
    if (side_forked)
        GNNB_HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ws->ev_join, 0));
    if (he != hipSuccess)
        return attempt(he, "fused GCN stack"); // (DECLINED: the whole batch layer by layer)
    if (seg && !forked && options().large_fork == 2) { // the small kernels on the caller's stream, behind the stack
        hipError_t hl = large_segment_small(model, ws, x_dev, (hipStream_t)stream);
        if (hl != hipSuccess && hl != hipErrorNotSupported)
            return fail(GNNB_ERR_HIP, "large-segment launch failed: %s", hipGetErrorString(hl));
        forked = hl == hipSuccess;
    }
    if (seg && !forked) { // the general layer-by-layer kernels on the large segment's rows
        const float *lcur = nullptr;
        // (no edge attributes: a GINE model never comes here -- gcn_stack_middle_layers)
        if ((rc = run_conv_layers(model, ws, x_dev, nullptr, large_n, large_n / ws->t.tile_rows, &lcur, stream)))
            return rc;
        GNNB_HIP_TRY(pool_large_segment(model, ws, lcur, (hipStream_t)stream));
    }
    if (seg)
        ws->last_path |= GNNB_PATH_LARGE_LAYERWISE;
    // (the stack kernel ran the head on its own graphs: what is left are the graphs of the large segment, if any)
    const int hg0 = head_fused ? (seg ? large_g : B) : 0;
    if (hg0 >= B)
        return GNNB_OK;
    return readout_from_pooled(model, ws, hg0, out_dev, stream);
}

static int forward_prepared_body(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr, float *out_dev,
                                 void *stream)
{
    if (!model || !ws || !x_dev || !out_dev)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward");
    if (!ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    if (memcmp(&model->desc, &ws->desc, sizeof(gnnb_model_desc)) != 0 || model->edge_dim != ws->edge_dim ||
        model->gat_heads != ws->gat_heads || model->gat_slope != ws->gat_slope || model->gat1_heads != ws->gat1_heads ||
        model->tf_heads != ws->tf_heads || model->gated != ws->gated ||
        model->ggnn_steps != ws->ggnn_steps || model->rgcn_relations != ws->rgcn_relations)
        return fail(GNNB_ERR_INVALID, "workspace was created for a different model");
    const gnnb_model_desc &d = model->desc;
    const int N = ws->t.num_nodes, B = ws->t.num_graphs;
    int rc;
    const bool fpx = d.fpx_w > 0;
    if (fpx) { // the input features enter as F_TYPE values: a quantised copy (the caller's buffer is not written)
        GNNB_HIP_TRY(launch_quantize(x_dev, ws->act[1], (size_t)N * d.in_dim, d.fpx_w, d.fpx_i, (hipStream_t)stream));
        x_dev = ws->act[1]; // (the layer loop never writes the buffer it reads)
    }

    // (large_g = 0: every graph is large -> layer by layer)
    const G2Deep deep = gcn_stack_middle_layers(model);
    if (!fpx && deep.nl >= 2 && d.mlp_num_linear <= 8 && !(prepared_large_g(ws) == 0 && B > 0))
        GNNB_RUNG(forward_stack(model, ws, x_dev, out_dev, deep, stream));

    ws->last_path = GNNB_PATH_LAYERWISE;
    const float *cur = nullptr;
    bool pooled = false;
    if ((rc = run_conv_layers(model, ws, x_dev, edge_attr, 0, 0, &cur, stream, &pooled)))
        return rc;
    return readout_layerwise(model, ws, cur, pooled, out_dev, stream);
}

// gnnb_forward_prepared and gnnb_forward_prepared_edges behind their checks; edge_attr: the latter's (nullptr: a model without)
static int forward_prepared(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr, float *out_dev, void *stream)
{
    // every launch below runs in the MODEL's math mode; the reduced modes' kernels flag this workspace
    MathScope math_scope(model ? model->desc.math : -1, ws ? ws->t.err : nullptr, ws ? ws->t.err_host_dev : nullptr);
    int rc = forward_prepared_body(model, ws, x_dev, edge_attr, out_dev, stream);
    if (rc != GNNB_OK)
        return rc;
    // output_activation(dim=-1) over every graph's output row (models.py:572-573)
    if (model->desc.output_activation != GNNB_OUT_NONE)
        GNNB_HIP_TRY(launch_output_activation(out_dev, ws->t.num_graphs, model->desc.mlp_out, model->desc.output_activation,
                                              (hipStream_t)stream));
    return GNNB_OK;
}

// a GINE model, its own workspace, and edge attributes for a batch of num_edges edges
static int check_edge_forward(const gnnb_model *model, const gnnb_workspace *ws, const float *edge_attr_dev, int num_edges, const char *entry)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to %s", entry);
    if (const int rc = refuse_rgcn_model(model, ws, entry, strstr(entry, "prepared") ? "gnnb_forward_prepared_types" : "gnnb_forward_batched_types"))
        return rc;
    if (!model->edge_dim)
        return fail(GNNB_ERR_INVALID, "%s takes a model of gnnb_edge_model_create; this one has no edge weights", entry);
    if (model->edge_dim != ws->edge_dim)
        return fail(GNNB_ERR_INVALID, "workspace was created for a different model");
    if (num_edges > 0 && !edge_attr_dev)
        return fail(GNNB_ERR_INVALID, "%s: edge_attr_dev is NULL for a batch of %d edges", entry, num_edges);
    return GNNB_OK;
}

// The one tail of gnnb_forward_batched, gnnb_forward_batched_edges and the three gnnb_forward_pyg* (gnnb_ingest.hip), each behind its
// own checks: graph prep -- without the lazy flag report where the entry's ingest has made it -- then the prepared forward.
int gnnb::forward_batched_tail(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev, const int32_t *coo_dev,
                               const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                               float *out_dev, void *stream, bool ingest_reported)
{
    if (const int rc = graph_prep_impl(ws, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, model->desc.pna_delta, stream,
                                       nullptr, ingest_reported))
        return rc;
    return forward_prepared(model, ws, x_dev, edge_attr_dev, out_dev, stream);
}

// an RGCNConv model, its own workspace, and edge types for a batch of num_edges edges
static int check_types_forward(const gnnb_model *model, const gnnb_workspace *ws, const int32_t *edge_type_dev, int num_edges, const char *entry)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to %s", entry);
    if (!model->rgcn_relations)
        return fail(GNNB_ERR_INVALID, "%s takes a model of gnnb_rgcn_model_create; this one has no relations", entry);
    if (model->rgcn_relations != ws->rgcn_relations || !ws->rgcn_rec)
        return fail(GNNB_ERR_INVALID, "workspace was created for a different model");
    if (num_edges > 0 && !edge_type_dev)
        return fail(GNNB_ERR_INVALID, "%s: edge_type_dev is NULL for a batch of %d edges", entry, num_edges);
    return GNNB_OK;
}

// the slot records of the prepared batch into the workspace's own allocation, then the prepared forward (rgcn_layer reads them)
static int forward_prepared_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int32_t *edge_type_dev, float *out_dev,
                                  void *stream)
{
    if (!x_dev || !out_dev)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward");
    if (!ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    GNNB_HIP_TRY(launch_rgcn_slots(ws->t, edge_type_dev, model->rgcn_relations, ws->rgcn_rec, (hipStream_t)stream));
    return forward_prepared(model, ws, x_dev, nullptr, out_dev, stream);
}

int gnnb::forward_batched_types_tail(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int32_t *edge_type_dev,
                                     const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs,
                                     int num_nodes, int num_edges, float *out_dev, void *stream, bool ingest_reported)
{
    if (const int rc = check_types_forward(model, ws, edge_type_dev, num_edges, "gnnb_forward_batched_types"))
        return rc;
    if (const int rc = graph_prep_impl(ws, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, model->desc.pna_delta, stream,
                                       nullptr, ingest_reported))
        return rc;
    return forward_prepared_types(model, ws, x_dev, edge_type_dev, out_dev, stream);
}

extern "C" {

int gnnb_forward_prepared_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int32_t *edge_type_dev, float *out_dev,
                                void *stream)
{
    if (const int rc = check_types_forward(model, ws, edge_type_dev, ws && ws->prepared ? ws->t.num_edges : 0, "gnnb_forward_prepared_types"))
        return rc;
    return forward_prepared_types(model, ws, x_dev, edge_type_dev, out_dev, stream);
}

int gnnb_forward_batched_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int32_t *edge_type_dev,
                               const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs, int num_nodes,
                               int num_edges, float *out_dev, void *stream)
{
    return forward_batched_types_tail(model, ws, x_dev, edge_type_dev, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, out_dev,
                                      stream, false);
}

int gnnb_forward_prepared(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev,
                          float *out_dev, void *stream)
{
    if (const int rc = refuse_edge_model(model, ws, "gnnb_forward_prepared", "gnnb_forward_prepared_edges"))
        return rc;
    if (const int rc = refuse_rgcn_model(model, ws, "gnnb_forward_prepared", "gnnb_forward_prepared_types"))
        return rc;
    return forward_prepared(model, ws, x_dev, nullptr, out_dev, stream);
}

int gnnb_forward_prepared_edges(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev,
                                float *out_dev, void *stream)
{
    if (const int rc = check_edge_forward(model, ws, edge_attr_dev, ws && ws->prepared ? ws->t.num_edges : 0, "gnnb_forward_prepared_edges"))
        return rc;
    return forward_prepared(model, ws, x_dev, edge_attr_dev, out_dev, stream);
}

int gnnb_forward_batched_edges(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev,
                               const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs,
                               int num_nodes, int num_edges, float *out_dev, void *stream)
{
    if (const int rc = check_edge_forward(model, ws, edge_attr_dev, num_edges, "gnnb_forward_batched_edges"))
        return rc;
    return forward_batched_tail(model, ws, x_dev, edge_attr_dev, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, out_dev, stream,
                                false);
}

int gnnb_forward_batched(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev,
                         const int32_t *coo_dev, const int32_t *node_ptr_dev,
                         const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                         float *out_dev, void *stream)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_batched");
    if (const int erc = refuse_edge_model(model, ws, "gnnb_forward_batched", "gnnb_forward_batched_edges"))
        return erc;
    if (const int erc = refuse_rgcn_model(model, ws, "gnnb_forward_batched", "gnnb_forward_batched_types"))
        return erc;
    return forward_batched_tail(model, ws, x_dev, nullptr, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, out_dev, stream, false);
}

// gnnb_forward_prepared(model, ws, ...) followed by gnnb_graph_prep(ws_next, ...) on the same stream -- with the prep of ws_next
// run INSIDE the forward's readout kernel where that exists (k_head_small, GUEST: extra workgroups): the software-pipelined form
// of gnnb_forward_batched for a stream of batches over two alternating workspaces.
int gnnb_forward_prepared_prep_next(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, float *out_dev,
                                    gnnb_workspace *ws_next, const int32_t *coo_dev, const int32_t *node_ptr_dev,
                                    const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges, void *stream)
{
    if (!model || !ws || !ws_next)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_prepared_prep_next");
    if (const int erc = refuse_edge_model(model, ws, "gnnb_forward_prepared_prep_next", "gnnb_forward_prepared_edges and gnnb_graph_prep"))
        return erc;
    if (const int erc = refuse_edge_model(nullptr, ws_next, "gnnb_forward_prepared_prep_next", "gnnb_forward_prepared_edges and gnnb_graph_prep"))
        return erc;
    if (const int erc = refuse_rgcn_model(model, ws, "gnnb_forward_prepared_prep_next", "gnnb_forward_prepared_types and gnnb_graph_prep"))
        return erc;
    if (const int erc = refuse_rgcn_model(nullptr, ws_next, "gnnb_forward_prepared_prep_next", "gnnb_forward_prepared_types and gnnb_graph_prep"))
        return erc;
    if (ws == ws_next)
        return fail(GNNB_ERR_INVALID, "gnnb_forward_prepared_prep_next: the next batch needs a workspace of its own (the forward reads "
                                      "the tables the prep writes)");
    if (!ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    if (!guest_prep_eligible(ws_next, num_nodes)) {
        const int rc = gnnb_forward_prepared(model, ws, x_dev, out_dev, stream);
        if (rc != GNNB_OK)
            return rc;
        return gnnb_graph_prep(ws_next, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, model->desc.pna_delta, stream);
    }
    PrepParams pp;
    int rc = graph_prep_impl(ws_next, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, model->desc.pna_delta, stream, &pp, false);
    if (rc != GNNB_OK)
        return rc; // (nothing was enqueued)
    ws_next->prepared = false; // (until its prep is enqueued)
    GuestPrep offer{&pp, false};
    struct Offer { // (the slot never outlives this call)
        GuestPrep *prev;
        explicit Offer(GuestPrep *g) : prev(guest_prep_slot()) { guest_prep_slot() = g; }
        ~Offer() { guest_prep_slot() = prev; }
    };
    {
        Offer scope(&offer);
        rc = gnnb_forward_prepared(model, ws, x_dev, out_dev, stream);
    }
    if (rc != GNNB_OK && !offer.taken)
        return rc; // (ws_next stays unprepared)
    if (!offer.taken) // the forward ran another readout than the one that hosts a prep: the prep as a launch of its own
        GNNB_HIP_TRY(launch_graph_prep(pp, (hipStream_t)stream));
    ws_next->prepared = true;
    return rc;
}

int gnnb_forward_batched_host(const gnnb_model *model, gnnb_workspace *ws, const float *x,
                              const int32_t *coo, const int32_t *node_ptr, const int32_t *edge_ptr,
                              int num_graphs, int num_nodes, int num_edges, float *out)
{
    if (!model || !ws || !x || !node_ptr || !edge_ptr || !out || (num_edges > 0 && !coo))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_batched_host");
    if (const int erc = refuse_edge_model(model, ws, "gnnb_forward_batched_host", "gnnb_forward_batched_edges on device buffers"))
        return erc;
    if (const int erc = refuse_rgcn_model(model, ws, "gnnb_forward_batched_host", "gnnb_forward_batched_types on device buffers"))
        return erc;
    if (const int crc = check_batch_sizes(ws, num_graphs, num_nodes, num_edges))
        return crc;
    const gnnb_model_desc &d = model->desc;
    // staging buffers live in the workspace, sized once for its capacities: the reference's <name>_top is called once
    // per graph (model_tb.cpp.jinja:189-205), and a hipMalloc / hipFree pair per call would dominate it
    const size_t cx = arena_up((size_t)ws->max_nodes * d.in_dim * 4), cc = arena_up((size_t)std::max(ws->max_edges, 1) * 8),
                 cp = arena_up(((size_t)ws->max_graphs + 1) * 4), co = arena_up((size_t)ws->max_graphs * d.mlp_out * 4);
    if (!ws->stage) {
        GNNB_HIP_TRY(hipMalloc((void **)&ws->stage, cx + cc + 2 * cp + co));
        ws->stage_bytes = cx + cc + 2 * cp + co;
    }
    float *dx = (float *)ws->stage;
    int32_t *dc = (int32_t *)(ws->stage + cx);
    int32_t *dn = (int32_t *)(ws->stage + cx + cc);
    int32_t *de = (int32_t *)(ws->stage + cx + cc + cp);
    float *dout = (float *)(ws->stage + cx + cc + 2 * cp);
    const size_t bx = (size_t)num_nodes * d.in_dim * 4, bc = (size_t)num_edges * 8,
                 bp = ((size_t)num_graphs + 1) * 4, bo = (size_t)num_graphs * d.mlp_out * 4;
    hipStream_t s0 = nullptr;
    if (bx)
        GNNB_HIP_TRY(hipMemcpyAsync(dx, x, bx, hipMemcpyHostToDevice, s0));
    if (bc)
        GNNB_HIP_TRY(hipMemcpyAsync(dc, coo, bc, hipMemcpyHostToDevice, s0));
    GNNB_HIP_TRY(hipMemcpyAsync(dn, node_ptr, bp, hipMemcpyHostToDevice, s0));
    GNNB_HIP_TRY(hipMemcpyAsync(de, edge_ptr, bp, hipMemcpyHostToDevice, s0));
    int rc = gnnb_forward_batched(model, ws, dx, dc, dn, de, num_graphs, num_nodes, num_edges, dout, nullptr);
    if (rc == GNNB_OK && bo)
        GNNB_HIP_TRY(hipMemcpyAsync(out, dout, bo, hipMemcpyDeviceToHost, s0));
    if (rc == GNNB_OK)
        rc = gnnb_workspace_check(ws, nullptr); // one synchronisation: the validation word and `out` are both back
    else
        (void)hipStreamSynchronize(s0);
    return rc;
}

int gnnb_gcn_stack_timed(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, int iters,
                         void *stream, float *out_us_per_launch)
{
    if (!model || !ws || !x_dev || iters < 1 || !out_us_per_launch)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_gcn_stack_timed");
    if (const int erc = refuse_edge_model(model, ws, "gnnb_gcn_stack_timed", "gnnb_forward_prepared_edges: it runs layer by layer"))
        return erc;
    if (const int erc = refuse_rgcn_model(model, ws, "gnnb_gcn_stack_timed", "gnnb_forward_prepared_types: it runs layer by layer"))
        return erc;
    MathScope math_scope(model->desc.math, ws->t.err, ws->t.err_host_dev);
    if (!ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    const G2Deep deep = gcn_stack_middle_layers(model);
    if (deep.nl < 2)
        return fail(GNNB_ERR_INVALID, "the fused stack exists for GCN / GIN models of two or more layers");
    // (as the forward launches it: with the MLP head inside where k_gcn2_zf takes it; its output goes to a workspace buffer)
    bool head_fused = false;
    return timed_loop((hipStream_t)stream, 3, iters, [&](int) {
        const int rc = attempt(launch_conv_stack(model, ws, small_segment(ws), x_dev, deep, (hipStream_t)stream, &ws->last_path, ws->mlp[0], &head_fused),
                               "fused GCN stack");
        return rc == DECLINED ? fail(GNNB_ERR_INVALID, "fused stack not eligible (shape, or no max_graph_nodes promise)") : rc;
    }, out_us_per_launch);
}

} // extern "C"
