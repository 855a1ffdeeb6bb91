// gnnb_runtime.hip -- host side of libgnnb_hip.so: errors and options, the workspace handle, graph prep and its plan, the
// stage entry points of the C ABI declared in include/gnnb_hip.h, gnnb_edge.h and gnnb_pna_edge.h (gnnb_aggregate, gnnb_linear, gnnb_global_pool
// ...), the timed loops and the utilities.  The forward -- which kernels run, in which order -- is gnnb_forward.hip; the PyG
// mini-batch entries (ingest, ordered ingest, edge attributes) and the workspace's add-on allocations are gnnb_ingest.hip.
//
// graph prep follows the reference's generated top (gnnbuilder/templates/model.cpp.jinja):
//   compute_degree/neighbor_tables (:737-758)  -> k_graph_prep, once per batch, shared by all layers
// There is no CPU fallback: every entry point fails with GNNB_ERR_NO_DEVICE / GNNB_ERR_HIP when
// the GPU path cannot run.
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gnnb_host.h"

namespace gnnb {

static thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// an option's default: the environment variable GNNB_<NAME> (atoi, not validated) or the table's
static int option_default(const char *name, int dflt)
{
    char var[64] = "GNNB_";
    size_t n = strlen(var);
    for (const char *c = name; *c && n + 1 < sizeof(var); c++)
        var[n++] = (char)toupper((unsigned char)*c);
    var[n] = 0;
    const char *v = getenv(var);
    return (v && *v) ? atoi(v) : dflt;
}

Options &options()
{
#define GNNB_OPTION_DEFAULT(name, dflt, accepts) option_default(#name, dflt),
    static Options o = {GNNB_OPTIONS(GNNB_OPTION_DEFAULT)};
#undef GNNB_OPTION_DEFAULT
    return o;
}

int refuse_edge_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->edge_dim) || (ws && ws->edge_dim))
        return fail(GNNB_ERR_INVALID, "%s: a GINE model (gnnb_edge_model_create) needs its edge attributes: call %s (gnnb_edge.h)", entry, use);
    return GNNB_OK;
}

int refuse_gat_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->gat_heads) || (ws && ws->gat_heads))
        return fail(GNNB_ERR_INVALID, "%s: a GATv2 model (gnnb_gat_model_create) runs layer by layer and is not served here: call %s (gnnb_gat.h)",
                    entry, use);
    return GNNB_OK;
}

int refuse_gatconv_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->gat1_heads) || (ws && ws->gat1_heads))
        return fail(GNNB_ERR_INVALID, "%s: a GAT model (gnnb_gatconv_model_create) runs layer by layer and is not served here: call %s "
                                      "(gnnb_gatconv.h)", entry, use);
    return GNNB_OK;
}

int refuse_transformer_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->tf_heads) || (ws && ws->tf_heads))
        return fail(GNNB_ERR_INVALID, "%s: a TransformerConv model (gnnb_transformer_model_create) runs layer by layer and is not served here: "
                                      "call %s (gnnb_transformer.h)", entry, use);
    return GNNB_OK;
}

int refuse_resgated_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->gated) || (ws && ws->gated))
        return fail(GNNB_ERR_INVALID, "%s: a ResGatedGraphConv model (gnnb_resgated_model_create) runs layer by layer and is not served here: "
                                      "call %s (gnnb_resgated.h)", entry, use);
    return GNNB_OK;
}

int refuse_ggnn_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->ggnn_steps) || (ws && ws->ggnn_steps))
        return fail(GNNB_ERR_INVALID, "%s: a GatedGraphConv model (gnnb_ggnn_model_create) runs layer by layer and is not served here: "
                                      "call %s (gnnb_ggnn.h)", entry, use);
    return GNNB_OK;
}

int refuse_rgcn_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use)
{
    if ((model && model->rgcn_relations) || (ws && ws->rgcn_relations))
        return fail(GNNB_ERR_INVALID, "%s: an RGCNConv model (gnnb_rgcn_model_create) needs the batch's edge types and is not served here: "
                                      "call %s (gnnb_rgcn.h)", entry, use);
    return GNNB_OK;
}

static thread_local int tl_math = -1; // >= 0: the calling thread is inside an entry point of a model with its own math mode
static thread_local FlagWord tl_flag = {nullptr, nullptr};
int launch_math() { return tl_math >= 0 ? tl_math : (int)options().math; }
static thread_local GuestPrep *tl_guest = nullptr;
GuestPrep *&guest_prep_slot() { return tl_guest; }
FlagWord launch_flag_word() { return tl_flag; }
MathScope::MathScope(int model_math, int32_t *err, int32_t *err_host) : prev(tl_math), prev_flag(tl_flag)
{
    if (model_math >= 0)
        tl_math = model_math;
    if (err)
        tl_flag = FlagWord{err, err_host};
}
MathScope::~MathScope()
{
    tl_math = prev;
    tl_flag = prev_flag;
}

} // namespace gnnb

using namespace gnnb;

// ---------------------------------------------------------------------------------------
extern "C" {

int gnnb_version(void) { return GNNB_VERSION; }

const char *gnnb_last_error(void) { return g_last_error.c_str(); }

int gnnb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int gnnb_stream_sync(void *stream)
{
    GNNB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_set_option(const char *name, int value)
{
    Options &o = options();
    if (!name)
        return fail(GNNB_ERR_INVALID, "null option name");
    const int v = value;
#define GNNB_OPTION_SET(opt, dflt, accepts)                                                        \
    if (!strcmp(name, #opt) && (accepts)) {                                                        \
        o.opt = v;                                                                                 \
        return GNNB_OK;                                                                            \
    }
    GNNB_OPTIONS(GNNB_OPTION_SET)
#undef GNNB_OPTION_SET
    return fail(GNNB_ERR_INVALID, "unknown option or bad value: %s=%d", name, value);
}

// ---------------------------------------------------------------------------------------
int gnnb_workspace_create(const gnnb_model *model, int max_graphs, int max_nodes, int max_edges,
                          gnnb_workspace **out_ws)
{
    if (!out_ws)
        return fail(GNNB_ERR_INVALID, "null out_ws");
    *out_ws = nullptr;
    if (!model)
        return fail(GNNB_ERR_INVALID, "null model");
    if (max_graphs < 1 || max_nodes < 1 || max_edges < 0)
        return fail(GNNB_ERR_INVALID, "workspace capacities must be positive");
    const gnnb_model_desc &d = model->desc;

    int maxw = d.in_dim, aggw = 4, tmpw = 4;
    for (int l = 0; l < d.num_layers; l++) {
        const LayerDims ld = layer_dims(d, l);
        maxw = std::max(maxw, std::max(ld.fin, ld.fout));
        aggw = std::max(aggw, d.conv_type == GNNB_CONV_PNA ? 4 * ld.fin : ld.fin);
    }
    tmpw = std::max(tmpw, maxw);
    if (model->gat_heads) // a GATv2 layer's GEMM writes [xl | xr] [N, 2 out] into tmp0
        for (int l = 0; l < d.num_layers; l++)
            tmpw = std::max(tmpw, 2 * layer_dims(d, l).fout);
    if (model->gat1_heads) // a GAT v1 layer's GEMM writes [xl | s_src | s_dst | pad] [N, out + roundup4(2 heads)] into tmp0
        for (int l = 0; l < d.num_layers; l++)
            tmpw = std::max(tmpw, layer_dims(d, l).fout + (int)gat_score_rows(model->gat1_heads));
    if (model->tf_heads) // a TransformerConv layer's GEMM writes [q | k | v | r] [N, 4 out] into tmp0
        for (int l = 0; l < d.num_layers; l++)
            tmpw = std::max(tmpw, 4 * layer_dims(d, l).fout + // (with edge features: [.. | qe], padded to whole 16-byte pieces)
                                      (model->edge_dim ? (int)transformer_edge_qe_rows(model->tf_heads, model->edge_dim) : 0));
    if (model->gated) // a ResGatedGraphConv layer's GEMM writes [k | q | v | r] [N, 4 out] into tmp0
        for (int l = 0; l < d.num_layers; l++)
            tmpw = std::max(tmpw, 4 * layer_dims(d, l).fout);
    if (model->ggnn_steps) // a GatedGraphConv step's GEMM writes [p | gh] [N, 6 out] into tmp0; tmp1 holds the two [N, out] state buffers
        for (int l = 0; l < d.num_layers; l++)
            tmpw = std::max(tmpw, GGNN_TMP_BLOCKS * layer_dims(d, l).fout); // (gnnb_host.h: what ggnn_layer carves from them)
    if (model->rgcn_relations) // an RGCNConv layer's GEMM writes [p_0 | .. | p_{R-1} | root] [N, (R + 1) out] into tmp0
        for (int l = 0; l < d.num_layers; l++)
            tmpw = std::max(tmpw, rgcn_tmp_blocks(model->rgcn_relations) * layer_dims(d, l).fout); // (gnnb_host.h)
    // the widest GEMM K of the conv layers: from 1024 on k_linear_dma may cut its tiles along K (stream-K) and needs a scratch,
    // which belongs to the workspace -- forwards of different workspaces never share one, whatever streams or graphs run them
    int max_k = 0;
    for (int l = 0; l < d.num_layers; l++) {
        const LayerDims ld = layer_dims(d, l);
        max_k = std::max(max_k, d.conv_type == GNNB_CONV_PNA ? 13 * ld.fin : d.conv_type == GNNB_CONV_SAGE ? 2 * ld.fin : std::max(ld.fin, ld.fout));
    }
    const bool want_sk = max_k >= 1024;
    // (the stage-cut planner's tables: opt-in -- carved only for workspaces created while the option is on; a workspace created
    // without them keeps equal tile counts whatever the option says later: round-5 advisor finding)
    const bool want_plan = options().stage_cut && (d.conv_type == GNNB_CONV_GCN || d.conv_type == GNNB_CONV_GIN) && d.num_layers >= 2 &&
                           model->gat_heads == 0 && model->gat1_heads == 0 && model->tf_heads == 0 && model->gated == 0 && model->ggnn_steps == 0 && model->rgcn_relations == 0; // (a GATv2 model,
                                            // a GAT v1 model, a TransformerConv model, a ResGatedGraphConv model, a GatedGraphConv model, an RGCNConv model take no stack kernel: no stage plan)
    const int pooledw = d.num_pools * gnn_out_width(d);
    const int mlpw = std::max(d.mlp_hidden, d.mlp_out);
    const int min_tile_rows = 4;
    const size_t max_tiles = (size_t)max_nodes / min_tile_rows + 2;

    gnnb_workspace *ws = new gnnb_workspace();
    ws->desc = d;
    ws->edge_dim = model->edge_dim;
    ws->gat_heads = model->gat_heads;
    ws->gat_slope = model->gat_slope;
    ws->gat1_heads = model->gat1_heads;
    ws->tf_heads = model->tf_heads;
    ws->gated = model->gated;
    ws->ggnn_steps = model->ggnn_steps;
    ws->rgcn_relations = model->rgcn_relations;
    ws->max_graphs = max_graphs;
    ws->max_nodes = max_nodes;
    ws->max_edges = max_edges;
    (void)hipGetDevice(&ws->device);

    const size_t N = max_nodes, E = std::max(max_edges, 1), B = max_graphs;
    // (models whose last conv layer ends in the large-K segmented GEMM -- GraphSAGE -- pool in that GEMM's epilogue: a
    // node -> graph table and the buffer for the pieces of graphs that cross 32-row blocks)
    const bool pool_epi = (d.conv_type == GNNB_CONV_SAGE || d.conv_type == GNNB_CONV_PNA) && d.num_layers >= 1 && d.fpx_w <= 0;
    const bool pna = d.conv_type == GNNB_CONV_PNA;
    const size_t deg_tiles = (N + 127) / 128 + GNNB_DEG_CLASSES + 1;
    // THE list of the blob's arrays, in their order in it: run once without a base for the size, once on the blob (an array the
    // workspace does not want takes nothing and reads nullptr)
    char *sk_base = nullptr;
    auto place = [&](Arena a) {
        BatchTables &t = ws->t;
        t.row_ptr = a.take<int32_t>(N + 1);
        t.col = a.take<int32_t>(E);
        t.eid = a.take<int32_t>(E);
        t.node_rec = a.take<int4>(2 * N);
        t.dinv = a.take<float>(N);
        t.amp = a.take<float>(N);
        t.att = a.take<float>(N);
        t.gcoef = a.take<float4>(N);
        t.tile_first = a.take<int32_t>(max_tiles + 1);
        t.tile_edge = a.take<int32_t>(max_tiles + 1);
        t.graph_ptr = a.take<int32_t>(B + 1);
        t.tile_graph = a.take<int32_t>(max_tiles + 1);
        t.err = a.take<int32_t>(1);
        t.agg_cut = a.take<int4>(4096 + 1);
        t.stage_cut = a.take<int32_t>(1024 + 2);
        ws->plan_scratch = want_plan ? a.take<int32_t>((size_t)stage_cut_levels((int)max_tiles) * (max_tiles + 1)) : nullptr;
        ws->deg_work = pna ? a.take<int32_t>(1024 * 16) : nullptr;
        ws->deg_perm = pna ? a.take<int32_t>(deg_tiles * 128) : nullptr;
        ws->deg_tile_cls = pna ? a.take<int32_t>(deg_tiles) : nullptr;
        t.node_graph = pool_epi ? a.take<int32_t>(N) : nullptr;
        ws->pool_part = pool_epi ? a.take<float2>(((N + 31) / 32) * 2 * (size_t)gnn_out_width(d)) : nullptr;
        ws->act[0] = a.take<float>(N * maxw);
        ws->act[1] = a.take<float>(N * maxw);
        ws->agg = a.take<float>(N * aggw);
        ws->tmp0 = a.take<float>(N * tmpw);
        ws->tmp1 = a.take<float>(N * tmpw);
        ws->pooled = a.take<float>(B * pooledw);
        ws->mlp[0] = a.take<float>(B * mlpw);
        ws->mlp[1] = a.take<float>(B * mlpw);
        sk_base = want_sk ? a.take<char>(stream_k_scratch_bytes()) : nullptr;
        ws->rgcn_rec = ws->rgcn_relations ? a.take<RgcnSlot>(E) : nullptr; // (last: every other workspace's layout is what it was)
        return a.off;
    };
    ws->bytes = place(Arena{nullptr});
    hipError_t e = hipMalloc((void **)&ws->blob, ws->bytes);
    if (e != hipSuccess) {
        const size_t bytes = ws->bytes;
        delete ws;
        return fail(GNNB_ERR_HIP, "workspace allocation of %zu bytes failed: %s", bytes,
                    hipGetErrorString(e));
    }
    (void)place(Arena{ws->blob});
    ws->t.agg_cut_n = 0;
    ws->t.stage_cut_n = 0;
    ws->t.stage_cut_cap = 1024;
    (void)hipMemset(ws->t.err, 0, sizeof(int32_t));
    if (want_sk) {
        ws->sk = stream_k_scratch_at(sk_base);
        // arrival counters zero (as every launch leaves them), guard pattern behind them.  Synchronous memsets, not the null
        // stream + a synchronise: that would join -- and could disturb a capture in progress on -- every blocking stream of the
        // process (round-5 advisor finding)
        (void)stream_k_scratch_init_sync(sk_base);
    }
    // best effort: without the mapped word only gnnb_workspace_check reports a malformed batch
    ws->t.err_host_dev = nullptr;
    if (hipHostMalloc((void **)&ws->err_host, 64, hipHostMallocMapped) == hipSuccess && ws->err_host) {
        *ws->err_host = 0;
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, ws->err_host, 0) == hipSuccess)
            ws->t.err_host_dev = (int32_t *)dp;
    } else {
        ws->err_host = nullptr;
        (void)hipGetLastError();
    }
    *out_ws = ws;
    return GNNB_OK;
}

void gnnb_workspace_destroy(gnnb_workspace *ws)
{
    if (!ws)
        return;
    if (ws->blob)
        (void)hipFree(ws->blob);
    if (ws->ingest_blob)
        (void)hipFree(ws->ingest_blob);
    if (ws->order_blob)
        (void)hipFree(ws->order_blob);
    if (ws->edge_blob)
        (void)hipFree(ws->edge_blob);
    if (ws->type_blob)
        (void)hipFree(ws->type_blob);
    if (ws->order_triple)
        (void)hipHostFree(ws->order_triple);
    if (ws->stage)
        (void)hipFree(ws->stage);
    if (ws->err_host)
        (void)hipHostFree(ws->err_host);
    if (ws->ev_fork)
        (void)hipEventDestroy(ws->ev_fork);
    if (ws->ev_join)
        (void)hipEventDestroy(ws->ev_join);
    if (ws->side)
        (void)hipStreamDestroy(ws->side);
    delete ws;
}

size_t gnnb_workspace_bytes(const gnnb_workspace *ws) { return ws ? ws->bytes : 0; }

int gnnb_workspace_last_path(const gnnb_workspace *ws) { return ws ? ws->last_path : GNNB_PATH_NONE; }

int gnnb_workspace_set_large_segment(gnnb_workspace *ws, int first_graph, int first_node, int first_edge)
{
    if (!ws)
        return fail(GNNB_ERR_INVALID, "null workspace");
    if (first_graph < 0) { // no large segment
        ws->large_g = ws->large_n = ws->large_e = -1;
        return GNNB_OK;
    }
    if (first_node < 0 || first_edge < 0)
        return fail(GNNB_ERR_INVALID, "the large segment needs the node and edge offsets of its first graph");
    ws->large_g = first_graph;
    ws->large_n = first_node;
    ws->large_e = first_edge;
    return GNNB_OK;
}

int gnnb_workspace_set_max_graph_nodes(gnnb_workspace *ws, int n)
{
    if (!ws || n < 0)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_workspace_set_max_graph_nodes");
    ws->max_graph_nodes = n;
    return GNNB_OK;
}

int gnnb_workspace_set_max_degree(gnnb_workspace *ws, int d)
{
    if (!ws || d < 0)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_workspace_set_max_degree");
    ws->max_degree = d;
    return GNNB_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------------
// (C++ linkage from here to gnnb_graph_prep: the gnnb:: functions below are what gnnb_forward.hip and gnnb_ingest.hip take from this
// unit, gnnb_host.h)
// The prep plan: what graph prep has to know about a workspace, each question answered in ONE place.  All of it is a handful
// of integer tests on the workspace and the options: nothing here allocates or looks anything up.

// A GCN / GIN model of two or more layers under a max_graph_nodes promise, with the stack kernels on: the batch (its small
// segment) is meant for the LDS-resident stack kernels, so the node tiles are sized for their stages
static bool stack_promised(const gnnb_workspace *ws)
{
    const gnnb_model_desc &d = ws->desc;
    // (a GINE model's workspace, a GATv2 model's, a GAT v1 model's, a TransformerConv model's, a ResGatedGraphConv model's, a
    // GatedGraphConv model's, an RGCNConv model's: never -- their layers take no stack kernel, whatever the promise)
    return options().fuse_gcn2 && (d.conv_type == GNNB_CONV_GCN || d.conv_type == GNNB_CONV_GIN) && d.num_layers >= 2 && ws->max_graph_nodes > 0 &&
           ws->edge_dim == 0 && ws->gat_heads == 0 && ws->gat1_heads == 0 && ws->tf_heads == 0 && ws->gated == 0 && ws->ggnn_steps == 0 && ws->rgcn_relations == 0;
}

// ... and the WHOLE batch is expected there: no large segment, no fixed-point emulation.  Such a batch needs neither the
// row-balanced aggregate ranges nor the GCN coefficient table.  (One predicate for three sites that used to spell it out: the
// two that ask about the coefficient table are inside conv_type == GCN, where "GCN or GIN" adds nothing; the one that asks
// about the aggregate ranges ANDs large_g < 0 beside it -- !(P && large_g < 0) && large_g < 0 == !P && large_g < 0 -- so the
// truth tables coincide.)
static bool stack_expected(const gnnb_workspace *ws) { return stack_promised(ws) && ws->large_g < 0 && ws->desc.fpx_w <= 0; }

// Which stack kernel a promised batch gets and how many rows its stages hold: a 2-layer fp32 GCN stack runs k_gcn2_zf (96- or
// 176-row stages), everything else k_gcn2_fused (64 rows; 48 in the bf16x6 mode, which only the 2-layer GCN form has)
struct StackKernel {
    bool zf, bf6;
    int stage_rows;
};
static StackKernel promised_stack_kernel(const gnnb_workspace *ws)
{
    const gnnb_model_desc &d = ws->desc;
    const bool gcn2 = d.conv_type == GNNB_CONV_GCN && d.num_layers == 2;
    StackKernel k;
    k.zf = gcn2 && options().fuse_zf;
    k.bf6 = !k.zf && launch_math() && gcn2;
    k.stage_rows = k.zf ? zf_stage_rows(d.in_dim) : k.bf6 ? GNNB_G2_STAGE_ROWS_BF6 : GNNB_G2_STAGE_ROWS;
    return k;
}

// PNA under a degree promise: graph prep sorts the rows into degree classes behind the tables
static bool wants_degree_classes(const gnnb_workspace *ws)
{
    return ws->desc.conv_type == GNNB_CONV_PNA && ws->max_degree > 0 && ws->max_degree <= GNNB_DEG_MAX && options().pna_classes && ws->deg_perm &&
           ws->large_g < 0 && ws->desc.fpx_w <= 0 && ws->edge_dim == 0; // (PNA with edge features takes no class form)
}

// The stage-cut planner MAY run behind the tables: the option is on and the workspace was created with its scratch.  (Coarse on
// purpose: it is asked before tile counts exist.  What graph_prep_impl launches under is this AND the conditions at the site.)
static bool may_plan_stage_cuts(const gnnb_workspace *ws) { return options().stage_cut && ws->plan_scratch; }

// GCN: the coefficient table is produced behind the tables unless the whole batch is expected on the stack kernels
// (a GATv2 or GAT v1 workspace is a GCN description whose layers never read the table: not produced there; gnnb_aggregate(GNNB_AGG_GCN)
// as a stage entry on such a workspace produces it lazily, ensure_gcoef)
static bool wants_gcoef_at_prep(const gnnb_workspace *ws)
{
    return ws->desc.conv_type == GNNB_CONV_GCN && ws->gat_heads == 0 && ws->gat1_heads == 0 && !stack_expected(ws);
}

// Can this workspace's graph prep run as a guest of the forward's readout kernel (k_head_small's extra workgroups)?  The molecule
// path (promise <= 64 nodes) of a batch that needs NOTHING launched behind its tables: no stage cuts, no degree classes, no
// coefficient table -- the same predicates graph_prep_impl launches those under.
bool gnnb::guest_prep_eligible(const gnnb_workspace *ws, int num_nodes)
{
    if (!options().guest_prep || ws->max_graph_nodes <= 0 || ws->max_graph_nodes > 64 || ws->large_g >= 0 || num_nodes <= 0)
        return false;
    // (the row-balanced aggregate ranges are part of the prep kernel itself: nothing behind it)
    return !may_plan_stage_cuts(ws) && !wants_degree_classes(ws) && !wants_gcoef_at_prep(ws);
}

// Lazy detection: a batch prepared (or ingested) EARLIER on this workspace was flagged on the device (edge leaving its graph,
// broken ptr arrays, broken max_graph_nodes promise, malformed PyG mini-batch) and nobody called gnnb_workspace_check since.  Read
// from a host-mapped word without synchronising: it reports what has already run, never the batch being enqueued now.
int gnnb::report_earlier_flags(gnnb_workspace *ws, void *stream)
{
    if (!ws->err_host || *(volatile int32_t *)ws->err_host == 0)
        return GNNB_OK;
    const int32_t seen = *(volatile int32_t *)ws->err_host;
    *(volatile int32_t *)ws->err_host = 0;
    // reported now: the device word is cleared as well (in stream order), or a later gnnb_workspace_check would blame
    // a good batch for it
    (void)hipMemsetAsync(ws->t.err, 0, sizeof(int32_t), (hipStream_t)stream);
    if (seen == GNNB_FLAG_RANGE)
        return fail(GNNB_ERR_RANGE, "an earlier forward on this workspace met a non-finite value in a reduced-precision math mode "
                                    "(fp16's range exceeded: its results were unspecified); run the model with math = 0");
    return fail(GNNB_ERR_GRAPH, "an earlier batch on this workspace was flagged as malformed (its results were "
                                "unspecified); gnnb_workspace_check reports and clears the flags");
}

// a batch of these sizes against the workspace's capacities
int gnnb::check_batch_sizes(const gnnb_workspace *ws, int num_graphs, int num_nodes, int num_edges)
{
    if (num_graphs < 0 || num_nodes < 0 || num_edges < 0)
        return fail(GNNB_ERR_INVALID, "negative batch size");
    if (num_graphs > ws->max_graphs || num_nodes > ws->max_nodes || num_edges > ws->max_edges)
        return fail(GNNB_ERR_CAPACITY, "batch (%d graphs, %d nodes, %d edges) exceeds workspace (%d, %d, %d)", num_graphs, num_nodes,
                    num_edges, ws->max_graphs, ws->max_nodes, ws->max_edges);
    return GNNB_OK;
}

// defer != nullptr (and guest_prep_eligible): everything gnnb_graph_prep does EXCEPT the launch -- *defer receives the kernel's arguments
int gnnb::graph_prep_impl(gnnb_workspace *ws, const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev,
                          int num_graphs, int num_nodes, int num_edges, float pna_delta, void *stream, PrepParams *defer, bool ingest_reported)
{
    if (!ws || !node_ptr_dev || !edge_ptr_dev || (num_edges > 0 && !coo_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_graph_prep");
    MathScope math_scope(ws->desc.math); // (the tile granularity depends on which stack kernel the mode selects)
    if (const int rc = check_batch_sizes(ws, num_graphs, num_nodes, num_edges))
        return rc;
    if (!ingest_reported) // (else: the same call has looked already, in front of its ingest -- gnnb_host.h)
        if (const int rc = report_earlier_flags(ws, stream))
            return rc;
    if (ws->large_g >= 0 && (ws->large_g > num_graphs || ws->large_n > num_nodes || ws->large_e > num_edges))
        return fail(GNNB_ERR_INVALID, "large segment (graph %d, node %d, edge %d) lies outside the batch (%d, %d, %d)",
                    ws->large_g, ws->large_n, ws->large_e, num_graphs, num_nodes, num_edges);
    BatchTables &t = ws->t;
    t.promise_graphs = ws->large_g >= 0 ? ws->large_g : num_graphs; // the promise covers graphs [0, promise_graphs)
    t.large_n = ws->large_g >= 0 ? ws->large_n : -1; // (checked against node_ptr / edge_ptr on the device: flag 16)
    t.large_e = ws->large_g >= 0 ? ws->large_e : -1;
    t.tile_lo = 0;
    t.node_ptr = node_ptr_dev;
    t.num_graphs = num_graphs;
    t.num_nodes = num_nodes;
    t.num_edges = num_edges;
    t.max_graph_nodes_hint = ws->max_graph_nodes;
    t.tile_rows = std::max((int)options().tile_rows, 4);
    // A 2-layer GCN with a promise takes the fused stack only if a whole tile (tile_rows - 1 + largest graph) fits
    // one 64-row stage (48 in the bf16x6 mode): for graphs of 50..61 nodes finer tiles (8, 4) keep that path open
    if (stack_promised(ws)) {
        const StackKernel k = promised_stack_kernel(ws);
        while (t.tile_rows > 4 && ws->max_graph_nodes + t.tile_rows - 1 > k.stage_rows)
            t.tile_rows >>= 1;
        // very large batches: coarser tiles (while a tile still fits a stage) keep the per-workgroup tile table in LDS
        const long tile_cap = k.zf ? gcn2_zf_tile_capacity(ws->desc.in_dim) : gcn2_fused_tile_capacity();
        while ((num_nodes + t.tile_rows - 1) / t.tile_rows > tile_cap && ws->max_graph_nodes + 2 * t.tile_rows - 1 <= k.stage_rows)
            t.tile_rows <<= 1;
    }
    t.num_tiles = (num_nodes + t.tile_rows - 1) / t.tile_rows;
    // row-balanced ranges for the gather-aggregate kernels (one per workgroup of the ring kernel's grid on this device):
    // not for a batch that is expected on the stack kernels entirely (their graph prep is on the pipeline's critical path
    // and pays for every instruction), not with a large segment (its aggregates walk a tile sub-range)
    {
        const int rings = aggregate_ring_grid();
        t.agg_cut_n = (options().agg_balance && !stack_expected(ws) && ws->large_g < 0 && rings <= 4096 && (rings & (rings - 1)) == 0 &&
                       t.num_tiles >= rings) ? rings : 0;
    }
    if (!(pna_delta > 0.0f))
        pna_delta = 1.0f;
    // the degree scalers (amp / att) are only read by PNA layers: a model-bound workspace of another conv type
    // skips their computation and their 8 B/node of writes (delta <= 0 tells the kernel)
    const float prep_delta = ws->desc.conv_type == GNNB_CONV_PNA ? pna_delta : -1.0f;
    // GCN: an explicit self-loop edge is not entered into the tables (PyG's gcn_norm replaces the self loops of the
    // input by exactly one per node; the reference C++ would count it on top of its own self term, see gnnb_hip.h)
    const int drop_self = ws->desc.conv_type == GNNB_CONV_GCN ? 1 : 0;
    const bool deferred = defer && guest_prep_eligible(ws, num_nodes);
    if (deferred)
        *defer = make_prep_params(coo_dev, node_ptr_dev, edge_ptr_dev, t, prep_delta, drop_self);
    else {
        if (defer)
            return fail(GNNB_ERR_INVALID, "graph prep deferred for a workspace that is not eligible");
        GNNB_HIP_TRY(launch_graph_prep(make_prep_params(coo_dev, node_ptr_dev, edge_ptr_dev, t, prep_delta, drop_self), (hipStream_t)stream));
    }
    ws->prepared = true;
    ws->prep_delta = prep_delta > 0.0f ? prep_delta : 0.0f;
    if (deferred) { // (eligible = nothing below would be launched: the tables do not exist yet)
        t.stage_cut_n = 0;
        ws->gcoef_ready = false;
        ws->deg_ready = false;
        return GNNB_OK;
    }
    // the conv-stack kernel's workgroup runs as whole stages of the global greedy stage list (k_plan.hip), right behind the tables
    // on the prep stream: for the batches that k_gcn2_fused takes (GIN stacks, GCN stacks deeper than two layers, the bf16x6 mode)
    t.stage_cut_n = 0;
    if (may_plan_stage_cuts(ws) && stack_promised(ws) && ws->desc.fpx_w <= 0 && num_nodes > 0) { // (the scratch exists for GCN / GIN stacks only)
        const StackKernel k = promised_stack_kernel(ws);
        const BatchTables ts = small_segment(ws);
        const int grid = gcn2_fused_grid(ts.num_tiles);
        if (!k.zf && ws->max_graph_nodes + t.tile_rows - 1 <= k.stage_rows && grid <= t.stage_cut_cap && ts.num_tiles > 0) {
            GNNB_HIP_TRY(launch_stage_cut(t.tile_first, ts.num_tiles, ts.num_nodes, k.stage_rows, grid, gcn2_fused_tile_window(), ws->plan_scratch,
                                          t.stage_cut, (hipStream_t)stream));
            t.stage_cut_n = grid;
        }
    }
    ws->gcoef_ready = false;
    // PNA under a degree promise: the rows sorted into degree classes, right behind the tables on the prep stream
    ws->deg_ready = false;
    if (wants_degree_classes(ws)) {
        ws->deg_max_tiles = (num_nodes + 127) / 128 + GNNB_DEG_CLASSES;
        GNNB_HIP_TRY(launch_degree_classes(t, ws->max_degree, ws->deg_work, ws->deg_perm, ws->deg_tile_cls, ws->deg_max_tiles,
                                           (hipStream_t)stream));
        ws->deg_ready = num_nodes > 0; // (an empty batch has no class tables: launch_degree_classes returns before it writes any)
        ws->deg_delta = pna_delta;
    }
    // The GCN coefficient table (dinv_i dinv_j of the four inline sources; read by every layer-wise GCN aggregate) is
    // produced HERE, on the prep stream right behind the tables, whenever the batch can run layer by layer -- so that a
    // forward captured into a hipGraph contains no lazily launched table kernel and aggregates on other streams that are
    // ordered against the prep see a finished table.  Only a workspace whose whole batch is expected on the LDS-resident
    // stack kernels (promise set, no large segment) skips it; should that forward fall back after all, ensure_gcoef
    // launches the table kernel in front of the first aggregate (the one lazy case left).
    if (wants_gcoef_at_prep(ws) && num_nodes > 0) {
        GNNB_HIP_TRY(launch_gcn_coef(ws->t, (hipStream_t)stream));
        ws->gcoef_ready = true;
    }
    return GNNB_OK;
}

// the GCN coefficient table of the prepared batch, once per batch, in front of the first layer-wise GCN aggregate
int gnnb::ensure_gcoef(gnnb_workspace *ws, void *stream)
{
    if (ws->gcoef_ready)
        return GNNB_OK;
    GNNB_HIP_TRY(launch_gcn_coef(ws->t, (hipStream_t)stream));
    ws->gcoef_ready = true;
    return GNNB_OK;
}

// rows: M of the call (0: nothing is read, so an empty operand may come without an address -- torch gives none)
int gnnb::build_gemm(GemmArgs &g, const gnnb_gemm_seg *segs, int num_segs, const float *w, int ldw, int rows)
{
    if (num_segs < 1 || num_segs > 4 || !segs)
        return fail(GNNB_ERR_INVALID, "gnnb_linear takes 1..4 segments");
    memset(&g, 0, sizeof(g));
    g.nseg = num_segs;
    int koff = 0;
    g.cpre[0] = 0;
    for (int s = 0; s < 4; s++) {
        if (s < num_segs) {
            if ((!segs[s].a_dev && rows > 0) || segs[s].k < 1 || segs[s].lda < segs[s].k)
                return fail(GNNB_ERR_INVALID, "bad GEMM segment %d", s);
            g.a[s] = segs[s].a_dev;
            g.rs[s] = segs[s].rowscale_dev;
            g.lda[s] = segs[s].lda;
            g.k[s] = segs[s].k;
            g.koff[s] = koff;
            g.avec[s] = (segs[s].k % 4 == 0) && (segs[s].lda % 4 == 0) && (((uintptr_t)segs[s].a_dev & 15) == 0);
            g.wvec[s] = (segs[s].k % 4 == 0) && (ldw % 4 == 0) && (koff % 4 == 0) && (((uintptr_t)w & 15) == 0);
            g.cpre[s + 1] = g.cpre[s] + (segs[s].k + 31) / 32;
            koff += segs[s].k;
        } else {
            g.cpre[s + 1] = g.cpre[s];
        }
    }
    if (koff > ldw)
        return fail(GNNB_ERR_INVALID, "segments span %d columns but ldw = %d", koff, ldw);
    return GNNB_OK;
}

// sk_owned: the calling workspace's stream-K scratch (nullptr: the standalone entry -- one per (device, stream), never under capture)
int gnnb::linear_segs(const StreamK *sk_owned, const gnnb_gemm_seg *segs, int num_segs, const float *w_dev, int ldw,
                      const float *bias_dev, const float *skip_dev, float *y_dev, int M, int N, int act, void *stream)
{
    if (!w_dev || (!y_dev && M > 0) || M < 0 || N < 1)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_linear");
    if (act < 0 || act > GNNB_ACT_NONE)
        return fail(GNNB_ERR_INVALID, "unknown activation %d", act);
    GemmArgs g;
    int rc = build_gemm(g, segs, num_segs, w_dev, ldw, M);
    if (rc != GNNB_OK)
        return rc;
    GNNB_HIP_TRY(launch_linear(g, w_dev, ldw, bias_dev, skip_dev, y_dev, M, N, act, (hipStream_t)stream, nullptr, nullptr, sk_owned));
    return GNNB_OK;
}

extern "C" {

int gnnb_graph_prep(gnnb_workspace *ws, const int32_t *coo_dev, const int32_t *node_ptr_dev,
                    const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                    float pna_delta, void *stream)
{
    return graph_prep_impl(ws, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, pna_delta, stream, nullptr, false);
}

int gnnb_workspace_check(gnnb_workspace *ws, void *stream)
{
    if (!ws || (!ws->prepared && !ws->ingested))
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    int32_t err = 0;
    GNNB_HIP_TRY(hipMemcpyAsync(&err, ws->t.err, sizeof(err), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GNNB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (err != 0) {
        (void)hipMemsetAsync(ws->t.err, 0, sizeof(int32_t), (hipStream_t)stream); // reset on read
        (void)hipStreamSynchronize((hipStream_t)stream);
    }
    if (ws->err_host)
        *(volatile int32_t *)ws->err_host = 0;
    static_assert(GNNB_FLAG_PTR_ENDS == 1 && GNNB_FLAG_PTR_ORDER == 2 && GNNB_FLAG_EDGE == 4 && GNNB_FLAG_GRAPH_NODES == 8 &&
                      GNNB_FLAG_LARGE_SEGMENT == 16 && GNNB_FLAG_DEGREE == 32 && GNNB_FLAG_RANGE == 64 && GNNB_FLAG_INGEST == 128 && GNNB_FLAG_EDGE_TYPE == 256,
                  "the message below names the bits by value");
    if (err & ~GNNB_FLAG_RANGE)
        return fail(GNNB_ERR_GRAPH, "malformed batch (flags 0x%x): 1/2 ptr arrays not monotone/complete, 4 an edge leaves "
                                    "its graph, 8 a graph exceeds the max_graph_nodes promise, 16 the large-segment offsets "
                                    "disagree with node_ptr / edge_ptr, 32 a node exceeds the max_degree promise, 64 a reduced-precision "
                                    "kernel produced a non-finite value, 128 gnnb_ingest_pyg: endpoint outside [0, N), edge between two "
                                    "graphs, or broken batch / ptr, 256 an edge type outside [0, relations) of an RGCNConv model", err);
    if (err & GNNB_FLAG_RANGE)
        return fail(GNNB_ERR_RANGE, "a reduced-precision math mode (bf16x3 / f16x3) produced a non-finite value since the last check: an "
                                    "activation or a weight beyond fp16's range (65504), or non-finite inputs; the results of that forward "
                                    "are unspecified -- run the model with math = 0 (flag 0x40)");
    return GNNB_OK;
}

// CSR slots no row owns (edges dropped by graph prep -- explicit self loops on a GCN workspace -- leave a gap at the end of
// their graph's segment, whose slots hold stale data) read -1 in the host copies
static int mark_unused_slots(gnnb_workspace *ws, int32_t *slots, hipStream_t s)
{
    const int N = ws->t.num_nodes, E = ws->t.num_edges;
    if (!slots || E <= 0)
        return GNNB_OK;
    std::vector<int32_t> rec((size_t)std::max(N, 1) * 8);
    if (N > 0)
        GNNB_HIP_TRY(hipMemcpyAsync(rec.data(), ws->t.node_rec, (size_t)N * 32, hipMemcpyDeviceToHost, s));
    GNNB_HIP_TRY(hipStreamSynchronize(s));
    std::vector<char> used((size_t)E, 0);
    for (int v = 0; v < N; v++) {
        const long start = rec[(size_t)v * 8], deg = rec[(size_t)v * 8 + 1];
        for (long k = std::max(start, 0L); k < std::min(start + deg, (long)E); k++)
            used[(size_t)k] = 1;
    }
    for (int k = 0; k < E; k++)
        if (!used[(size_t)k])
            slots[k] = -1;
    return GNNB_OK;
}

int gnnb_graph_tables_to_host(gnnb_workspace *ws, int32_t *row_ptr, int32_t *col, int32_t *in_deg,
                              void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    hipStream_t s = (hipStream_t)stream;
    const int N = ws->t.num_nodes, E = ws->t.num_edges;
    std::vector<int32_t> rec(in_deg ? (size_t)N * 8 : 0); // node records {start, degree, j0, j1}{j2, j3, -, -}
    if (row_ptr)
        GNNB_HIP_TRY(hipMemcpyAsync(row_ptr, ws->t.row_ptr, ((size_t)N + 1) * 4, hipMemcpyDeviceToHost, s));
    if (in_deg && N > 0)
        GNNB_HIP_TRY(hipMemcpyAsync(rec.data(), ws->t.node_rec, (size_t)N * 32, hipMemcpyDeviceToHost, s));
    if (col && E > 0)
        GNNB_HIP_TRY(hipMemcpyAsync(col, ws->t.col, (size_t)E * 4, hipMemcpyDeviceToHost, s));
    GNNB_HIP_TRY(hipStreamSynchronize(s));
    if (in_deg)
        for (int i = 0; i < N; i++)
            in_deg[i] = rec[(size_t)i * 8 + 1];
    return mark_unused_slots(ws, col, s);
}

int gnnb_edge_index_table_to_host(gnnb_workspace *ws, int32_t *edge_index_table, void *stream)
{
    if (!ws || !ws->prepared || !edge_index_table)
        return fail(GNNB_ERR_INVALID, "gnnb_edge_index_table_to_host needs a prepared batch and an output array");
    if (ws->t.num_edges > 0)
        GNNB_HIP_TRY(hipMemcpyAsync(edge_index_table, ws->t.eid, (size_t)ws->t.num_edges * 4, hipMemcpyDeviceToHost,
                                    (hipStream_t)stream));
    GNNB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return mark_unused_slots(ws, edge_index_table, (hipStream_t)stream);
}

int gnnb_aggregate_edges(gnnb_workspace *ws, const float *x_dev, const float *edge_term_dev, float *out_dev,
                         int width, float eps, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_edges needs a prepared batch (gnnb_graph_prep)");
    if (!x_dev || !out_dev || width < 1 || (ws->t.num_edges > 0 && !edge_term_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_edges");
    GNNB_HIP_TRY(launch_aggregate_edges(ws->t, x_dev, edge_term_dev, out_dev, width, eps, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_edges_fused(gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev, int edge_dim, const float *we_dev, int ldwe,
                               const float *be_dev, float *out_dev, int width, float eps, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_edges_fused needs a prepared batch (gnnb_graph_prep)");
    if (!x_dev || !out_dev || !we_dev || !be_dev || width < 1 || edge_dim < 1 || edge_dim > 16 || ldwe < edge_dim ||
        (ws->t.num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_edges_fused (edge_dim 1 .. 16, ldwe >= edge_dim)");
    GNNB_HIP_TRY(launch_gine_aggregate(ws->t, x_dev, edge_attr_dev, edge_dim, we_dev, ldwe, be_dev, out_dev, width, eps, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_pna_edges(gnnb_workspace *ws, const float *p_dev, const float *q_dev, const float *edge_attr_dev, int edge_dim,
                             const float *we_dev, int ldwe, const float *be_dev, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_pna_edges needs a prepared batch (gnnb_graph_prep)");
    if (!p_dev || !out_dev || !we_dev || !be_dev || width < 1 || edge_dim < 1 || edge_dim > 16 || ldwe < edge_dim ||
        (ws->t.num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_pna_edges (edge_dim 1 .. 16, ldwe >= edge_dim)");
    GNNB_HIP_TRY(launch_pna_edge_aggregate(ws->t, p_dev, q_dev, edge_attr_dev, edge_dim, we_dev, ldwe, be_dev, out_dev, width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_gatv2(gnnb_workspace *ws, const float *xl_dev, int ldl, const float *xr_dev, int ldr, const float *att_dev,
                         const float *bias_dev, const float *skip_dev, int act, int heads, float negative_slope, float *out_dev, int width,
                         void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gatv2 needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type != GNNB_CONV_GCN) // (only there are the tables free of (v, v) edges: the kernel adds the self term)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gatv2 takes the prepared batch of a GCN workspace (or a GATv2 model's): graph prep drops "
                                      "explicit self loops there, the kernel adds the one self term");
    if (!xl_dev || !xr_dev || !att_dev || !out_dev || heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH ||
        width % heads != 0 || ldl < width || ldr < width || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE || !std::isfinite(negative_slope))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_gatv2 (heads 1 .. %d dividing width 1 .. %d, ldl and ldr >= width, a "
                                      "gnnb_act, a finite negative_slope)", GAT_MAX_HEADS, GAT_MAX_WIDTH);
    GNNB_HIP_TRY(launch_gatv2_aggregate(ws->t, xl_dev, ldl, xr_dev, ldr, att_dev, bias_dev, skip_dev, act, heads, negative_slope, out_dev, width,
                                        (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_gat(gnnb_workspace *ws, const float *xl_dev, int ldl, const float *ssrc_dev, int lds, const float *sdst_dev, int ldd,
                       const float *bias_dev, const float *skip_dev, int act, int heads, float negative_slope, float *out_dev, int width,
                       void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gat needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type != GNNB_CONV_GCN) // (only there are the tables free of (v, v) edges: the kernel adds the self term)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gat takes the prepared batch of a GCN workspace (or a GAT model's): graph prep drops "
                                      "explicit self loops there, the kernel adds the one self term");
    if (!xl_dev || !ssrc_dev || !sdst_dev || !out_dev || heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH ||
        width % heads != 0 || ldl < width || lds < heads || ldd < heads || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE ||
        !std::isfinite(negative_slope))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_gat (heads 1 .. %d dividing width 1 .. %d, ldl >= width, lds and ldd >= "
                                      "heads, a gnnb_act, a finite negative_slope)", GAT_MAX_HEADS, GAT_MAX_WIDTH);
    GNNB_HIP_TRY(launch_gat_aggregate(ws->t, xl_dev, ldl, ssrc_dev, lds, sdst_dev, ldd, bias_dev, skip_dev, act, heads, negative_slope, out_dev,
                                      width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_gat_edges(gnnb_workspace *ws, const float *xl_dev, int ldl, const float *ssrc_dev, int lds, const float *sdst_dev, int ldd,
                             const float *bias_dev, const float *skip_dev, int act, int heads, float negative_slope, const float *edge_attr_dev,
                             int edge_dim, const float *ae_dev, int ldae, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gat_edges needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type != GNNB_CONV_GCN) // (only there are the tables free of (v, v) edges: the kernel adds the self term)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gat_edges takes the prepared batch of a GCN workspace (or a GAT model's): graph prep drops "
                                      "explicit self loops there, the kernel adds the one self term");
    if (!xl_dev || !ssrc_dev || !sdst_dev || !out_dev || heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH ||
        width % heads != 0 || ldl < width || lds < heads || ldd < heads || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE ||
        !std::isfinite(negative_slope))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_gat_edges (heads 1 .. %d dividing width 1 .. %d, ldl >= width, lds and "
                                      "ldd >= heads, a gnnb_act, a finite negative_slope)", GAT_MAX_HEADS, GAT_MAX_WIDTH);
    if (!ae_dev || edge_dim < 1 || edge_dim > 16 || ldae < edge_dim || (ws->t.num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_gat_edges (ae, edge_dim 1 .. 16, ldae >= edge_dim, edge_attr for a batch "
                                      "with edges)");
    GNNB_HIP_TRY(launch_gat_edge_aggregate(ws->t, xl_dev, ldl, ssrc_dev, lds, sdst_dev, ldd, bias_dev, skip_dev, act, heads, negative_slope,
                                           edge_attr_dev, edge_dim, ae_dev, ldae, out_dev, width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_gatv2_edges(gnnb_workspace *ws, const float *xl_dev, int ldl, const float *xr_dev, int ldr, const float *att_dev,
                               const float *bias_dev, const float *skip_dev, int act, int heads, float negative_slope, const float *edge_attr_dev,
                               int edge_dim, const float *we_dev, int ldwe, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gatv2_edges needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type != GNNB_CONV_GCN) // (only there are the tables free of (v, v) edges: the kernel adds the self term)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_gatv2_edges takes the prepared batch of a GCN workspace (or a GATv2 model's): graph prep "
                                      "drops explicit self loops there, the kernel adds the one self term");
    if (!xl_dev || !xr_dev || !att_dev || !out_dev || heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH ||
        width % heads != 0 || ldl < width || ldr < width || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE || !std::isfinite(negative_slope))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_gatv2_edges (heads 1 .. %d dividing width 1 .. %d, ldl and ldr >= width, a "
                                      "gnnb_act, a finite negative_slope)", GAT_MAX_HEADS, GAT_MAX_WIDTH);
    if (!we_dev || edge_dim < 1 || edge_dim > 16 || ldwe < edge_dim || (ws->t.num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_gatv2_edges (edge_dim 1 .. 16, ldwe >= edge_dim, edge_attr for a batch "
                                      "with edges)");
    GNNB_HIP_TRY(launch_gatv2_edge_aggregate(ws->t, xl_dev, ldl, xr_dev, ldr, att_dev, bias_dev, skip_dev, act, heads, negative_slope, edge_attr_dev,
                                             edge_dim, we_dev, ldwe, out_dev, width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_transformer(gnnb_workspace *ws, const float *q_dev, int ldq, const float *k_dev, int ldk, const float *v_dev, int ldv,
                               const float *root_dev, int ldr, const float *skip_dev, int act, int heads, float scale, float *out_dev, int width,
                               void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_transformer needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN) // (a GCN model's, a GATv2 model's with or without edge features)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_transformer takes a prepared batch whose tables keep explicit self loops: graph prep "
                                      "drops the (v, v) edges on a workspace of a GCN description (a GCN or GATv2 model's), and this layer "
                                      "counts them as ordinary edges");
    if (!q_dev || !k_dev || !v_dev || !out_dev || heads < 1 || heads > TF_MAX_HEADS || width < 1 || width > TF_MAX_WIDTH || width % heads != 0 ||
        ldq < width || ldk < width || ldv < width || (root_dev && ldr < width) || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE ||
        !std::isfinite(scale))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_transformer (heads 1 .. %d dividing width 1 .. %d, ldq, ldk, ldv and "
                                      "root's ldr >= width, a gnnb_act, a finite scale)", TF_MAX_HEADS, TF_MAX_WIDTH);
    GNNB_HIP_TRY(launch_transformer_aggregate(ws->t, q_dev, ldq, k_dev, ldk, v_dev, ldv, root_dev, ldr, skip_dev, act, heads, scale, out_dev,
                                              width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_resgated(gnnb_workspace *ws, const float *k_dev, int ldk, const float *q_dev, int ldq, const float *v_dev, int ldv,
                            const float *root_dev, int ldr, const float *skip_dev, int act, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_resgated needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN) // (a GCN model's, a GATv2 model's with or without edge features)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_resgated takes a prepared batch whose tables keep explicit self loops: graph prep "
                                      "drops the (v, v) edges on a workspace of a GCN description (a GCN or GATv2 model's), and this layer "
                                      "counts them as ordinary edges");
    if (!k_dev || !q_dev || !v_dev || !out_dev || width < 1 || width > RG_MAX_WIDTH || ldk < width || ldq < width || ldv < width ||
        (root_dev && ldr < width) || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_resgated (k, q, v and out not NULL, width 1 .. %d, ldk, ldq, ldv and "
                                      "root's ldr >= width, a gnnb_act)", RG_MAX_WIDTH);
    GNNB_HIP_TRY(launch_resgated_aggregate(ws->t, k_dev, ldk, q_dev, ldq, v_dev, ldv, root_dev, ldr, skip_dev, act, out_dev, width,
                                           (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_ggnn(gnnb_workspace *ws, const float *p_dev, int ldp, const float *gh_dev, int ldgh, const float *h_dev, int ldh, int h_width,
                        const float *b_ih_dev, const float *skip_dev, int act, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_ggnn needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN) // (a GCN model's, a GATv2 model's, a GAT v1 model's, with or without edge features)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_ggnn takes a prepared batch whose tables keep explicit self loops: graph prep drops the "
                                      "(v, v) edges on a workspace of a GCN description (a GCN, GATv2 or GAT model's), and this layer counts "
                                      "them as ordinary edges");
    // (a prepared batch without nodes launches nothing and reads no operand: an empty tensor's NULL pointer is no error there)
    const bool operands = ws->t.num_nodes <= 0 || (p_dev && gh_dev && h_dev && out_dev);
    if (!operands || width < 1 || width > GG_MAX_WIDTH || h_width < 1 || h_width > width || ldp < 3 * width ||
        ldgh < 3 * width || ldh < h_width || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_ggnn (p, gh, h and out not NULL unless the batch has no nodes, width 1 .. %d, h_width 1 .. width, ldp "
                                      "and ldgh >= 3 width, ldh >= h_width, a gnnb_act)", GG_MAX_WIDTH);
    GNNB_HIP_TRY(launch_ggnn_aggregate(ws->t, p_dev, ldp, gh_dev, ldgh, h_dev, ldh, h_width, b_ih_dev, skip_dev, act, out_dev, width,
                                       (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_rgcn_slots(gnnb_workspace *ws, const int32_t *edge_type_dev, int relations, void *slot_rec_dev, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_rgcn_slots needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN) // (a GCN model's, a GATv2 model's, a GAT v1 model's, with or without edge features)
        return fail(GNNB_ERR_INVALID, "gnnb_rgcn_slots takes a prepared batch whose tables keep explicit self loops: graph prep drops the "
                                      "(v, v) edges on a workspace of a GCN description (a GCN, GATv2 or GAT model's), and this layer counts "
                                      "them as ordinary edges");
    // (a prepared batch without edges launches nothing and reads no operand)
    const bool operands = ws->t.num_edges <= 0 || (edge_type_dev && slot_rec_dev);
    if (!operands || relations < 1 || relations > RGCN_MAX_RELATIONS || ((uintptr_t)slot_rec_dev & 7) != 0)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_rgcn_slots (edge_type and slot_rec not NULL unless the batch has no edges, slot_rec "
                                      "8-byte aligned, relations 1 .. %d)", RGCN_MAX_RELATIONS);
    GNNB_HIP_TRY(launch_rgcn_slots(ws->t, edge_type_dev, relations, (RgcnSlot *)slot_rec_dev, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_rgcn(gnnb_workspace *ws, const void *slot_rec_dev, const float *p_dev, int ldp, int relations, const float *root_dev, int ldr,
                        const float *skip_dev, int act, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_rgcn needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_rgcn takes a prepared batch whose tables keep explicit self loops: graph prep drops the "
                                      "(v, v) edges on a workspace of a GCN description (a GCN, GATv2 or GAT model's), and this layer counts "
                                      "them as ordinary edges");
    // (a prepared batch without nodes launches nothing and reads no operand: an empty tensor's NULL pointer is no error there)
    const bool operands = ws->t.num_nodes <= 0 || (p_dev && out_dev && (slot_rec_dev || ws->t.num_edges <= 0));
    if (!operands || width < 1 || width > RGCN_MAX_WIDTH || relations < 1 || relations > RGCN_MAX_RELATIONS ||
        (int64_t)ldp < (int64_t)relations * width || (root_dev && ldr < width) || ((uintptr_t)slot_rec_dev & 7) != 0 || act < GNNB_ACT_RELU ||
        act > GNNB_ACT_NONE)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_rgcn (slot_rec, p and out not NULL unless the batch has no edges / nodes, "
                                      "slot_rec 8-byte aligned, width 1 .. %d, relations 1 .. %d, ldp >= relations width, ldr >= width, a "
                                      "gnnb_act)", RGCN_MAX_WIDTH, RGCN_MAX_RELATIONS);
    GNNB_HIP_TRY(launch_rgcn_aggregate(ws->t, (const RgcnSlot *)slot_rec_dev, p_dev, ldp, relations, root_dev, ldr, skip_dev, act, out_dev, width,
                                       (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_resgated_edges(gnnb_workspace *ws, const float *k_dev, int ldk, const float *q_dev, int ldq, const float *v_dev, int ldv,
                                  const float *root_dev, int ldr, const float *skip_dev, int act, const float *edge_attr_dev, int edge_dim,
                                  const float *wg_dev, int ldwg, const float *wv_dev, int ldwv, float *out_dev, int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_resgated_edges needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN) // (a GCN model's, a GATv2 model's with or without edge features)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_resgated_edges takes a prepared batch whose tables keep explicit self loops: graph prep "
                                      "drops the (v, v) edges on a workspace of a GCN description (a GCN or GATv2 model's), and this layer "
                                      "counts them as ordinary edges");
    if (!k_dev || !q_dev || !v_dev || !out_dev || width < 1 || width > RG_MAX_WIDTH || ldk < width || ldq < width || ldv < width ||
        (root_dev && ldr < width) || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_resgated_edges (k, q, v and out not NULL, width 1 .. %d, ldk, ldq, ldv "
                                      "and root's ldr >= width, a gnnb_act)", RG_MAX_WIDTH);
    if (!wg_dev || !wv_dev || edge_dim < 1 || edge_dim > RGE_MAX_EDGE_DIM || ldwg < edge_dim || ldwv < edge_dim ||
        (ws->t.num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_resgated_edges (wg and wv, edge_dim 1 .. %d, ldwg and ldwv >= edge_dim, "
                                      "edge_attr for a batch with edges)", RGE_MAX_EDGE_DIM);
    GNNB_HIP_TRY(launch_resgated_edge_aggregate(ws->t, k_dev, ldk, q_dev, ldq, v_dev, ldv, root_dev, ldr, skip_dev, act, edge_attr_dev, edge_dim,
                                                wg_dev, ldwg, wv_dev, ldwv, out_dev, width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_transformer_edges(gnnb_workspace *ws, const float *q_dev, int ldq, const float *k_dev, int ldk, const float *v_dev, int ldv,
                                     const float *qe_dev, int ldqe, const float *root_dev, int ldr, const float *skip_dev, int act, int heads,
                                     float scale, const float *edge_attr_dev, int edge_dim, const float *we_dev, int ldwe, float *out_dev,
                                     int width, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_transformer_edges needs a prepared batch (gnnb_graph_prep)");
    if (ws->desc.conv_type == GNNB_CONV_GCN) // (a GCN model's, a GATv2 model's with or without edge features)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate_transformer_edges takes a prepared batch whose tables keep explicit self loops: graph prep "
                                      "drops the (v, v) edges on a workspace of a GCN description (a GCN or GATv2 model's), and this layer "
                                      "counts them as ordinary edges, with their attribute rows");
    if (!q_dev || !k_dev || !v_dev || !out_dev || heads < 1 || heads > TF_MAX_HEADS || width < 1 || width > TF_MAX_WIDTH || width % heads != 0 ||
        ldq < width || ldk < width || ldv < width || (root_dev && ldr < width) || act < GNNB_ACT_RELU || act > GNNB_ACT_NONE ||
        !std::isfinite(scale))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_transformer_edges (heads 1 .. %d dividing width 1 .. %d, ldq, ldk, ldv and "
                                      "root's ldr >= width, a gnnb_act, a finite scale)", TF_MAX_HEADS, TF_MAX_WIDTH);
    if (!qe_dev || !we_dev || edge_dim < 1 || edge_dim > TFE_MAX_EDGE_DIM || ldqe < heads * edge_dim || ldwe < edge_dim ||
        (ws->t.num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_transformer_edges (qe and we, edge_dim 1 .. %d, ldqe >= heads * edge_dim, "
                                      "ldwe >= edge_dim, edge_attr for a batch with edges)", TFE_MAX_EDGE_DIM);
    GNNB_HIP_TRY(launch_transformer_edge_aggregate(ws->t, q_dev, ldq, k_dev, ldk, v_dev, ldv, qe_dev, ldqe, root_dev, ldr, skip_dev, act, heads,
                                                   scale, edge_attr_dev, edge_dim, we_dev, ldwe, out_dev, width, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_pna_product_aggregate(gnnb_workspace *ws, const float *x_dev, const float *wb_dev, int ldw, float *out_dev, int width,
                               void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_pna_product_aggregate needs a prepared batch (gnnb_graph_prep)");
    MathScope math_scope(ws->desc.math);
    if (!x_dev || !wb_dev || !out_dev || width < 1 || ldw < width)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_pna_product_aggregate");
    hipError_t he = launch_pna_pagg(ws->t, x_dev, width, wb_dev, ldw, out_dev, (hipStream_t)stream);
    if (he == hipErrorNotSupported)
        return fail(GNNB_ERR_INVALID, "gnnb_pna_product_aggregate takes widths 128 / 64 / 32, 16-byte aligned operands, an ldw that is a multiple of 4 and a workspace "
                                      "whose max_graph_nodes promise fits a 64-row stage (promise + tile rows - 1 <= 64), without a large "
                                      "segment; the option pna_pagg must be on (it is %s)", options().pna_pagg ? "on" : "OFF");
    GNNB_HIP_TRY(he);
    return GNNB_OK;
}

int gnnb_aggregate(gnnb_workspace *ws, int agg_kind, const float *x_dev, const float *self_dev,
                   float *out_dev, int width, float eps, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_aggregate needs a prepared batch (gnnb_graph_prep)");
    if (!x_dev || !out_dev || width < 1)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate");
    if (agg_kind < GNNB_AGG_GCN || agg_kind > GNNB_AGG_COPY)
        return fail(GNNB_ERR_INVALID, "unknown aggregate kind %d", agg_kind);
    // (PNA with self_dev == NULL: no destination term -- the statistics of p_j alone, what the degree-class form aggregates)
    if (ws->t.num_nodes == 0)
        return GNNB_OK;
    if (agg_kind == GNNB_AGG_GCN) {
        int rc = ensure_gcoef(ws, stream);
        if (rc != GNNB_OK)
            return rc;
    }
    GNNB_HIP_TRY(launch_aggregate(ws->t, agg_kind, x_dev, self_dev, out_dev, width, eps,
                                  (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_linear(const gnnb_gemm_seg *segs, int num_segs, const float *w_dev, int ldw,
                const float *bias_dev, const float *skip_dev, float *y_dev, int M, int N, int act,
                void *stream)
{
    return linear_segs(nullptr, segs, num_segs, w_dev, ldw, bias_dev, skip_dev, y_dev, M, N, act, stream);
}

int gnnb_debug_stream_k_guard(gnnb_workspace *ws, void *stream)
{
    // (a workspace whose model has no K >= 1024 layer owns no scratch: said so, instead of silently checking the stand-alone
    // scratch of (device, stream) or nothing at all -- round-5 advisor finding)
    if (ws && !ws->sk.part)
        return fail(GNNB_ERR_INVALID, "this workspace owns no stream-K scratch (no layer of its model has K >= 1024): nothing to check; "
                                      "pass ws = NULL for the stand-alone gnnb_linear scratch of (device, stream)");
    const int ok = stream_k_guard_intact(ws ? &ws->sk : nullptr, (hipStream_t)stream);
    if (ok < 0)
        return fail(GNNB_ERR_HIP, "reading the stream-K scratch back failed");
    if (ok == 0)
        return fail(GNNB_ERR_INVALID, "stream-K scratch: an arrival counter was left non-zero or the guard region behind the counters was written");
    return GNNB_OK;
}

int gnnb_global_pool(gnnb_workspace *ws, const float *x_dev, int d, const int32_t *pools,
                     int num_pools, float *out_dev, void *stream)
{
    if (!ws || !ws->prepared)
        return fail(GNNB_ERR_INVALID, "gnnb_global_pool needs a prepared batch");
    if (!x_dev || !out_dev || !pools || d < 1 || num_pools < 1 || num_pools > 3)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_global_pool");
    for (int i = 0; i < num_pools; i++)
        if (pools[i] < 0 || pools[i] > GNNB_POOL_MAX)
            return fail(GNNB_ERR_INVALID, "unsupported pooling %d", pools[i]);
    GNNB_HIP_TRY(launch_global_pool(x_dev, ws->t.graph_ptr, ws->t.num_graphs, d, pools, num_pools,
                                    out_dev, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_aggregate_timed(gnnb_workspace *ws, int agg_kind, const float *const *x_dev_list,
                         const float *self_dev, float *const *out_dev_list, int nbuf, int width,
                         float eps, int iters, void *stream, float *out_us_per_launch)
{
    if (!x_dev_list || !out_dev_list || nbuf < 1 || iters < 1 || !out_us_per_launch)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_aggregate_timed");
    // (the warm-up also touches every buffer)
    return timed_loop((hipStream_t)stream, nbuf, iters, [&](int i) {
        return gnnb_aggregate(ws, agg_kind, x_dev_list[i % nbuf], self_dev, out_dev_list[i % nbuf], width, eps, stream);
    }, out_us_per_launch);
}

int gnnb_linear_timed(const float *a_dev, int lda, int k, const float *w_dev, int ldw,
                      const float *bias_dev, float *y_dev, int M, int N, int act, int iters,
                      void *stream, float *out_us_per_launch)
{
    if (iters < 1 || !out_us_per_launch)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_linear_timed");
    gnnb_gemm_seg seg = {a_dev, nullptr, lda, k};
    return timed_loop((hipStream_t)stream, 3, iters, [&](int) { return gnnb_linear(&seg, 1, w_dev, ldw, bias_dev, nullptr, y_dev, M, N, act, stream); }, out_us_per_launch);
}

// ---------------------------------------------------------------------------------------
int gnnb_event_create(void **out_event)
{
    if (!out_event)
        return fail(GNNB_ERR_INVALID, "null out_event");
    hipEvent_t ev;
    GNNB_HIP_TRY(hipEventCreate(&ev));
    *out_event = (void *)ev;
    return GNNB_OK;
}

int gnnb_event_record(void *event, void *stream)
{
    GNNB_HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_event_elapsed_ms(void *start, void *stop, float *out_ms)
{
    if (!out_ms)
        return fail(GNNB_ERR_INVALID, "null out_ms");
    GNNB_HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    GNNB_HIP_TRY(hipEventElapsedTime(out_ms, (hipEvent_t)start, (hipEvent_t)stop));
    return GNNB_OK;
}

void gnnb_event_destroy(void *event)
{
    if (event)
        (void)hipEventDestroy((hipEvent_t)event);
}

int gnnb_malloc(void **out_dev, size_t bytes)
{
    if (!out_dev)
        return fail(GNNB_ERR_INVALID, "null out_dev");
    GNNB_HIP_TRY(hipMalloc(out_dev, bytes ? bytes : 4));
    return GNNB_OK;
}

void gnnb_free(void *dev)
{
    if (dev)
        (void)hipFree(dev);
}

int gnnb_memcpy_h2d(void *dst_dev, const void *src, size_t bytes, void *stream)
{
    GNNB_HIP_TRY(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return GNNB_OK;
}

int gnnb_memcpy_d2h(void *dst, const void *src_dev, size_t bytes, void *stream)
{
    GNNB_HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    GNNB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return GNNB_OK;
}

} // extern "C"
