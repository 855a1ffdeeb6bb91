// gnnb_runtime.hip -- host side of libgnnb_hip.so: model / workspace handles, the batched
// forward that sequences the kernels of k_*.hip on one HIP stream, and the C ABI
// declared in include/gnnb_hip.h.
//
// Sequencing follows the reference's generated top (gnnbuilder/templates/model.cpp.jinja):
//   load_parameters once (:724-730)            -> gnnb_model_create (device-resident weights)
//   compute_degree/neighbor_tables (:737-758)  -> k_graph_prep, once per batch, shared by all layers
//   compute_gnn_head (:151-359)                -> per layer: k_aggregate + k_linear (+skip +act fused)
//   compute_global_graph_pooling (:413-449)    -> k_global_pool
//   compute_mlp_head (:454-530)                -> k_linear chain
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
    const bool want_plan = options().stage_cut && (d.conv_type == GNNB_CONV_GCN || d.conv_type == GNNB_CONV_GIN) && d.num_layers >= 2;
    const int pooledw = d.num_pools * gnn_out_width(d);
    const int mlpw = std::max(d.mlp_hidden, d.mlp_out);
    const int min_tile_rows = 4;
    const size_t max_tiles = (size_t)max_nodes / min_tile_rows + 2;

    gnnb_workspace *ws = new gnnb_workspace();
    ws->desc = d;
    ws->max_graphs = max_graphs;
    ws->max_nodes = max_nodes;
    ws->max_edges = max_edges;
    (void)hipGetDevice(&ws->device);

    size_t off = 0;
    auto carve = [&](size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t N = max_nodes, E = std::max(max_edges, 1), B = max_graphs;
    // (models whose last conv layer ends in the large-K segmented GEMM -- GraphSAGE -- pool in that GEMM's epilogue: a
    // node -> graph table and the buffer for the pieces of graphs that cross 32-row blocks)
    const bool pool_epi = (d.conv_type == GNNB_CONV_SAGE || d.conv_type == GNNB_CONV_PNA) && d.num_layers >= 1 && d.fpx_w <= 0;
    const size_t o_rp = carve((N + 1) * 4), o_col = carve(E * 4), o_eid = carve(E * 4), o_rec = carve(N * 32), o_dinv = carve(N * 4), o_amp = carve(N * 4),
                 o_att = carve(N * 4), o_gcoef = carve(N * 16), o_tile = carve((max_tiles + 1) * 4), o_tedge = carve((max_tiles + 1) * 4), o_gptr = carve((B + 1) * 4),
                 o_tgraph = carve((max_tiles + 1) * 4), o_err = carve(4), o_cut = carve((4096 + 1) * 16), o_scut = carve((1024 + 2) * 4),
                 o_plan = carve(want_plan ? (size_t)stage_cut_levels((int)max_tiles) * (max_tiles + 1) * 4 : 0),
                 o_dwork = carve(d.conv_type == GNNB_CONV_PNA ? 1024 * 16 * 4 : 0),
                 o_dperm = carve(d.conv_type == GNNB_CONV_PNA ? ((N + 127) / 128 + GNNB_DEG_CLASSES + 1) * 128 * 4 : 0),
                 o_dcls = carve(d.conv_type == GNNB_CONV_PNA ? ((N + 127) / 128 + GNNB_DEG_CLASSES + 1) * 4 : 0),
                 o_ngraph = carve(pool_epi ? N * 4 : 0), o_part = carve(pool_epi ? ((N + 31) / 32) * 2 * (size_t)gnn_out_width(d) * 8 : 0),
                 o_a0 = carve(N * maxw * 4), o_a1 = carve(N * maxw * 4), o_agg = carve(N * aggw * 4),
                 o_t0 = carve(N * tmpw * 4), o_t1 = carve(N * tmpw * 4),
                 o_pool = carve(B * pooledw * 4), o_m0 = carve(B * mlpw * 4),
                 o_m1 = carve(B * mlpw * 4), o_sk = carve(want_sk ? stream_k_scratch_bytes() : 0);
    ws->bytes = off;
    hipError_t e = hipMalloc((void **)&ws->blob, ws->bytes);
    if (e != hipSuccess) {
        delete ws;
        return fail(GNNB_ERR_HIP, "workspace allocation of %zu bytes failed: %s", off,
                    hipGetErrorString(e));
    }
    char *b = ws->blob;
    ws->t.row_ptr = (int32_t *)(b + o_rp);
    ws->t.col = (int32_t *)(b + o_col);
    ws->t.eid = (int32_t *)(b + o_eid);
    ws->t.node_rec = (int4 *)(b + o_rec);
    ws->t.dinv = (float *)(b + o_dinv);
    ws->t.amp = (float *)(b + o_amp);
    ws->t.att = (float *)(b + o_att);
    ws->t.gcoef = (float4 *)(b + o_gcoef);
    ws->t.tile_first = (int32_t *)(b + o_tile);
    ws->t.graph_ptr = (int32_t *)(b + o_gptr);
    ws->t.tile_edge = (int32_t *)(b + o_tedge);
    ws->t.tile_graph = (int32_t *)(b + o_tgraph);
    ws->t.err = (int32_t *)(b + o_err);
    ws->t.agg_cut = (int4 *)(b + o_cut);
    ws->t.agg_cut_n = 0;
    ws->t.stage_cut = (int32_t *)(b + o_scut);
    ws->t.stage_cut_n = 0;
    ws->t.stage_cut_cap = 1024;
    ws->plan_scratch = want_plan ? (int32_t *)(b + o_plan) : nullptr;
    ws->t.node_graph = pool_epi ? (int32_t *)(b + o_ngraph) : nullptr;
    if (d.conv_type == GNNB_CONV_PNA) {
        ws->deg_work = (int32_t *)(b + o_dwork);
        ws->deg_perm = (int32_t *)(b + o_dperm);
        ws->deg_tile_cls = (int32_t *)(b + o_dcls);
    }
    ws->pool_part = pool_epi ? (float2 *)(b + o_part) : nullptr;
    ws->act[0] = (float *)(b + o_a0);
    ws->act[1] = (float *)(b + o_a1);
    ws->agg = (float *)(b + o_agg);
    ws->tmp0 = (float *)(b + o_t0);
    ws->tmp1 = (float *)(b + o_t1);
    ws->pooled = (float *)(b + o_pool);
    ws->mlp[0] = (float *)(b + o_m0);
    ws->mlp[1] = (float *)(b + o_m1);
    (void)hipMemset(ws->t.err, 0, sizeof(int32_t));
    if (want_sk) {
        ws->sk = stream_k_scratch_at(b + o_sk);
        // arrival counters zero (as every launch leaves them), guard pattern behind them.  Synchronous memsets, not the null
        // stream + a synchronise: that would join -- and could disturb a capture in progress on -- every blocking stream of the
        // process (round-5 advisor finding)
        (void)stream_k_scratch_init_sync(b + o_sk);
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

static BatchTables small_segment(const gnnb_workspace *ws);

// ---------------------------------------------------------------------------------------
// The prep plan: what graph prep has to know about a workspace, each question answered in ONE place.  All of it is a handful
// of integer tests on the workspace and the options: nothing here allocates or looks anything up.

// A GCN / GIN model of two or more layers under a max_graph_nodes promise, with the stack kernels on: the batch (its small
// segment) is meant for the LDS-resident stack kernels, so the node tiles are sized for their stages
static bool stack_promised(const gnnb_workspace *ws)
{
    const gnnb_model_desc &d = ws->desc;
    return options().fuse_gcn2 && (d.conv_type == GNNB_CONV_GCN || d.conv_type == GNNB_CONV_GIN) && d.num_layers >= 2 && ws->max_graph_nodes > 0;
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
           ws->large_g < 0 && ws->desc.fpx_w <= 0;
}

// The stage-cut planner MAY run behind the tables: the option is on and the workspace was created with its scratch.  (Coarse on
// purpose: it is asked before tile counts exist.  What graph_prep_impl launches under is this AND the conditions at the site.)
static bool may_plan_stage_cuts(const gnnb_workspace *ws) { return options().stage_cut && ws->plan_scratch; }

// GCN: the coefficient table is produced behind the tables unless the whole batch is expected on the stack kernels
static bool wants_gcoef_at_prep(const gnnb_workspace *ws) { return ws->desc.conv_type == GNNB_CONV_GCN && !stack_expected(ws); }

// Can this workspace's graph prep run as a guest of the forward's readout kernel (k_head_small's extra workgroups)?  The molecule
// path (promise <= 64 nodes) of a batch that needs NOTHING launched behind its tables: no stage cuts, no degree classes, no
// coefficient table -- the same predicates graph_prep_impl launches those under.
static bool guest_prep_eligible(const gnnb_workspace *ws, int num_nodes)
{
    if (!options().guest_prep || ws->max_graph_nodes <= 0 || ws->max_graph_nodes > 64 || ws->large_g >= 0 || num_nodes <= 0)
        return false;
    // (the row-balanced aggregate ranges are part of the prep kernel itself: nothing behind it)
    return !may_plan_stage_cuts(ws) && !wants_degree_classes(ws) && !wants_gcoef_at_prep(ws);
}

// defer != nullptr (and guest_prep_eligible): everything gnnb_graph_prep does EXCEPT the launch -- *defer receives the kernel's arguments
static int graph_prep_impl(gnnb_workspace *ws, const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev,
                           int num_graphs, int num_nodes, int num_edges, float pna_delta, void *stream, PrepParams *defer);

int gnnb_graph_prep(gnnb_workspace *ws, const int32_t *coo_dev, const int32_t *node_ptr_dev,
                    const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                    float pna_delta, void *stream)
{
    return graph_prep_impl(ws, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, pna_delta, stream, nullptr);
}

static int graph_prep_impl(gnnb_workspace *ws, const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev,
                           int num_graphs, int num_nodes, int num_edges, float pna_delta, void *stream, PrepParams *defer)
{
    if (!ws || !node_ptr_dev || !edge_ptr_dev || (num_edges > 0 && !coo_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_graph_prep");
    MathScope math_scope(ws->desc.math); // (the tile granularity depends on which stack kernel the mode selects)
    if (num_graphs < 0 || num_nodes < 0 || num_edges < 0)
        return fail(GNNB_ERR_INVALID, "negative batch size");
    if (num_graphs > ws->max_graphs || num_nodes > ws->max_nodes || num_edges > ws->max_edges)
        return fail(GNNB_ERR_CAPACITY,
                    "batch (%d graphs, %d nodes, %d edges) exceeds workspace (%d, %d, %d)",
                    num_graphs, num_nodes, num_edges, ws->max_graphs, ws->max_nodes, ws->max_edges);
    // lazy detection: a batch prepared EARLIER on this workspace was flagged on the device (edge leaving its graph,
    // broken ptr arrays, broken max_graph_nodes promise) and nobody called gnnb_workspace_check since.  Read from a
    // host-mapped word without synchronising: it reports what has already run, never the batch being enqueued now.
    if (ws->err_host && *(volatile int32_t *)ws->err_host != 0) {
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
        GNNB_HIP_TRY(launch_graph_prep(coo_dev, node_ptr_dev, edge_ptr_dev, t, prep_delta, drop_self,
                                       (hipStream_t)stream));
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
static int ensure_gcoef(gnnb_workspace *ws, void *stream)
{
    if (ws->gcoef_ready)
        return GNNB_OK;
    GNNB_HIP_TRY(launch_gcn_coef(ws->t, (hipStream_t)stream));
    ws->gcoef_ready = true;
    return GNNB_OK;
}

int gnnb_workspace_check(gnnb_workspace *ws, void *stream)
{
    if (!ws || !ws->prepared)
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
    if (err & ~GNNB_FLAG_RANGE)
        return fail(GNNB_ERR_GRAPH, "malformed batch (flags 0x%x): 1/2 ptr arrays not monotone/complete, 4 an edge leaves "
                                    "its graph, 8 a graph exceeds the max_graph_nodes promise, 16 the large-segment offsets "
                                    "disagree with node_ptr / edge_ptr, 32 a node exceeds the max_degree promise, 64 a reduced-precision "
                                    "kernel produced a non-finite value", err);
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

// rows: M of the call (0: nothing is read, so an empty operand may come without an address -- torch gives none)
static int build_gemm(GemmArgs &g, const gnnb_gemm_seg *segs, int num_segs, const float *w, int ldw, int rows = 1)
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
static int linear_segs(const StreamK *sk_owned, const gnnb_gemm_seg *segs, int num_segs, const float *w_dev, int ldw,
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

// ---------------------------------------------------------------------------------------
// one plain GEMM through the stand-alone entry (its stream-K scratch: per (device, stream), not a workspace's)
static int linear1(const float *a, int lda, int k, const float *w, int ldw, const float *bias,
                   const float *skip, float *y, int M, int N, int act, void *stream)
{
    gnnb_gemm_seg seg = {a, nullptr, lda, k};
    return gnnb_linear(&seg, 1, w, ldw, bias, skip, y, M, N, act, stream);
}

// One attempt at a launcher that may decline: it ran (TOOK), it launched nothing and the next form is tried (DECLINED:
// hipErrorNotSupported), or it failed -- FAILED: "<what> launch failed: ..." is the error text and GNNB_ERR_HIP the code to return
enum Attempt { TOOK, DECLINED, FAILED };
static Attempt attempt(hipError_t he, const char *what)
{
    if (he == hipSuccess)
        return TOOK;
    if (he == hipErrorNotSupported)
        return DECLINED;
    (void)fail(GNNB_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(he));
    return FAILED;
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
        g.wmid = model->conv[1][0];
        g.bmid = model->conv[1][1];
        if (L > 3) {
            g.mid_stride = (long)(model->conv[2][0] - model->conv[1][0]);
            g.bmid_stride = (long)(model->conv[2][1] - model->conv[1][1]);
        }
        for (int l = 1; l + 1 < L; l++)
            if (model->conv[l][0] != g.wmid + (long)(l - 1) * g.mid_stride || model->conv[l][1] != g.bmid + (long)(l - 1) * g.bmid_stride)
                return g;
    }
    g.skip = d.skip ? 1 : 0;
    g.nl = L;
    return g;
}

// The conv layers one by one (gather-aggregate + GEMM kernels) on the node rows [row_lo, N) of the prepared batch:
// row_lo = 0 is the whole batch; row_lo > 0 the caller's large segment (gnnb_workspace_set_large_segment), whose first
// node tile is tile_lo.  Aggregations index the batch-global buffers (sources are batch-global ids) and walk the tiles
// from tile_lo; the GEMMs take the row range as a pointer offset.  *out_cur = the last layer's output matrix ([N, width],
// rows below row_lo untouched).
static int run_conv_layers(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, int row_lo, int tile_lo,
                           const float **out_cur, void *stream, bool *pooled_in_epilogue = nullptr)
{
    if (pooled_in_epilogue)
        *pooled_in_epilogue = false;
    const gnnb_model_desc &d = model->desc;
    const int N = ws->t.num_nodes, M = N - row_lo;
    int rc;
    const bool fpx = d.fpx_w > 0;
    BatchTables tv = ws->t;
    tv.tile_lo = tile_lo;
    const StreamK *const sko = ws->sk.part ? &ws->sk : nullptr; // this workspace's stream-K scratch
    // the layers' GEMMs, on the workspace's scratch (unlike the stand-alone gnnb_linear / linear1)
    auto ws_linear = [&](const gnnb_gemm_seg *segs, int num_segs, const float *w_dev, int ldw, const float *bias_dev, const float *skip_dev,
                         float *y_dev, int M_, int N_, int act, void *st) -> int {
        return linear_segs(sko, segs, num_segs, w_dev, ldw, bias_dev, skip_dev, y_dev, M_, N_, act, st);
    };
    auto ws_linear1 = [&](const float *a, int lda, int k, const float *w, int ldw, const float *bias, const float *skip_, float *y, int M_, int N_,
                          int act, void *st) -> int {
        gnnb_gemm_seg seg = {a, nullptr, lda, k};
        return linear_segs(sko, &seg, 1, w, ldw, bias, skip_, y, M_, N_, act, st);
    };
    auto aggregate = [&](int kind, const float *x, const float *selfq, float *out, int w, float eps) -> int {
        if (M <= 0)
            return GNNB_OK;
        if (kind == GNNB_AGG_GCN) {
            int rc2 = ensure_gcoef(ws, stream);
            if (rc2 != GNNB_OK)
                return rc2;
        }
        GNNB_HIP_TRY(launch_aggregate(tv, kind, x, selfq, out, w, eps, (hipStream_t)stream));
        return GNNB_OK;
    };
    auto R = [&](const float *p, int width) { return p ? p + (size_t)row_lo * width : p; }; // row range of a [N, width] matrix
    auto Rw = [&](float *p, int width) { return p + (size_t)row_lo * width; };
    const bool whole = row_lo == 0;
    const float *cur = x_dev;
    int which = 0;
    bool mean_ready = false; // GraphSAGE: ws->agg already holds mean_j of the current layer's input rows (k_sage_first_mean)
    for (int l = 0; l < d.num_layers; l++) {
        const LayerDims ld = layer_dims(d, l);
        const int fi = ld.fin, fo = ld.fout;
        const std::vector<const float *> &p = model->conv[l];
        // skip connection on middle layers only (models.py:562-564); fused into the GEMM epilogue
        const float *skip = (d.skip && l != 0 && l != d.num_layers - 1) ? cur : nullptr;
        // (GraphSAGE / PNA: derived weight slots of such a layer carry the skip connection as + I on x's own weights: gnnb_model_create)
        const bool skip_fold = skip != nullptr && fi == fo && !fpx;
        float *nxt = ws->act[which];
        if ((const float *)nxt == cur) { // never write the buffer being read
            which ^= 1;
            nxt = ws->act[which];
        }
        switch (d.conv_type) {
        case GNNB_CONV_GCN:
            // aggregate at the input width, then transform (the reference's order, lib:1346-1379)
            if (whole && options().fuse_narrow && fi <= 32) {
                const Attempt at = attempt(launch_conv_gather(ws->t, GNNB_AGG_GCN, 0.f, cur, fi, fi, p[0], fi, p[1], skip, nxt,
                                                              fo, d.activation, (hipStream_t)stream), "fused narrow conv");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                if (at == TOOK)
                    break;
            }
            if ((rc = aggregate(GNNB_AGG_GCN, cur, nullptr, ws->agg, fi, 0.f)))
                return rc;
            if ((rc = ws_linear1(R(ws->agg, fi), fi, fi, p[0], fi, p[1], R(skip, fi), Rw(nxt, fo), M, fo, d.activation, stream)))
                return rc;
            break;
        case GNNB_CONV_GIN: {
            bool fused = false;
            if (whole && options().fuse_narrow && fi <= 32) {
                const Attempt at = attempt(launch_conv_gather(ws->t, GNNB_AGG_SUM, d.gin_eps, cur, fi, fi, p[0], fi, p[1], nullptr,
                                                              ws->tmp0, fo, GNNB_ACT_RELU, (hipStream_t)stream), "fused narrow conv");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                fused = at == TOOK;
            }
            if (!fused) {
                if ((rc = aggregate(GNNB_AGG_SUM, cur, nullptr, ws->agg, fi, d.gin_eps)))
                    return rc;
                if ((rc = ws_linear1(R(ws->agg, fi), fi, fi, p[0], fi, p[1], nullptr, Rw(ws->tmp0, fo), M, fo, GNNB_ACT_RELU, stream)))
                    return rc;
            }
            if ((rc = ws_linear1(R(ws->tmp0, fo), fo, fo, p[2], fo, p[3], R(skip, fo), Rw(nxt, fo), M, fo, d.activation, stream)))
                return rc;
            break;
        }
        case GNNB_CONV_SAGE: {
            if (whole && options().fuse_narrow && 2 * fi <= 32 && l + 1 < d.num_layers && skip == nullptr && !fpx) {
                // narrow input AND a layer behind it: the stage's output rows stay in LDS and the next layer's mean aggregate is
                // taken from there -- its aggregate kernel (a full read and write of [N, fo]) is not run
                const Attempt at = attempt(launch_sage_first_mean(ws->t, cur, fi, p[0], 2 * fi, p[1], nxt, ws->agg, fo, d.activation, (hipStream_t)stream), "first-layer + mean");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                if (at == TOOK) {
                    mean_ready = true;
                    break;
                }
            }
            if (whole && options().fuse_narrow && 2 * fi <= 32) {
                // narrow input: [mean_j x_j | x_i] is produced inside the GEMM's A stage (K = 2 F_in)
                const Attempt at = attempt(launch_conv_gather(ws->t, GNNB_AGG_MEAN, 0.f, cur, fi, 2 * fi, p[0], 2 * fi, p[1], skip, nxt,
                                                              fo, d.activation, (hipStream_t)stream, fi), "fused narrow conv");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                if (at == TOOK)
                    break;
            }
            if (!mean_ready && (rc = aggregate(GNNB_AGG_MEAN, cur, nullptr, ws->agg, fi, 0.f)))
                return rc;
            mean_ready = false;
            gnnb_gemm_seg segs[2] = {{R(ws->agg, fi), nullptr, fi, fi}, {R(cur, fi), nullptr, fi, fi}};
            // the LAST layer of a whole-batch run: global pooling in the GEMM's epilogue -- its [N, out] output is never
            // written and the separate pooling pass (a full read of it) disappears (reference: compute_gnn_head's last
            // layer + compute_global_graph_pooling, templates/model.cpp.jinja:151-449).  Falls back when the GEMM shape
            // has no such epilogue.
            if (pooled_in_epilogue && whole && l == d.num_layers - 1 && !fpx && options().fuse_pool && ws->t.node_graph && ws->pool_part) {
                GemmArgs g;
                if ((rc = build_gemm(g, segs, 2, p[0], 2 * fi)))
                    return rc;
                const PoolEpilogue pe = pool_epilogue(ws, d);
                const Attempt at = attempt(launch_linear(g, p[0], 2 * fi, p[1], nullptr, nxt, M, fo, d.activation, (hipStream_t)stream, &pe), "pooling GEMM");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                if (at == TOOK) {
                    GNNB_HIP_TRY(launch_pool_combine(pe, M, fo, (hipStream_t)stream));
                    *pooled_in_epilogue = true;
                    break;
                }
            }
            if (skip_fold && p.size() >= 3 && options().fold_skip) { // (slot 2: [Wl | Wr + I])
                if ((rc = ws_linear(segs, 2, p[2], 2 * fi, p[1], nullptr, Rw(nxt, fo), M, fo, d.activation, stream)))
                    return rc;
                break;
            }
            if ((rc = ws_linear(segs, 2, p[0], 2 * fi, p[1], R(skip, fi), Rw(nxt, fo), M, fo, d.activation, stream)))
                return rc;
            break;
        }
        case GNNB_CONV_PNA: {
            // a narrow input (the first layer): the whole layer in one kernel, whole graphs staged in LDS (k_pna_first.hip)
            if (whole && fi <= 12 && skip == nullptr && !fpx && p.size() >= 8 && options().pna_fold_lin && ws->prep_delta == d.pna_delta) {
                const Attempt at = attempt(launch_pna_first(ws->t, cur, fi, p[0], p[1], p[6], 13 * fi, p[7], nxt, fo, d.activation, (hipStream_t)stream), "narrow PNA layer");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                if (at == TOOK)
                    break;
            }
            // h_ij = Wpre [x_i || x_j] + b  ==  (Wpre[:, :F] x_i + b) + Wpre[:, F:] x_j
            float *q = ws->tmp0, *pp = ws->tmp1;
            // degree-class form (gnnb_workspace_set_max_degree; decided here: it folds the destination's pre-NN term into x's
            // class weights, so q is not computed and the aggregate runs without a destination term)
            // (the row-class GEMM addresses a row of its operands as a 32-bit byte offset on the operand's base, row * 16 fi
            // for the aggregate: the form applies while that stays below 2^32 -- 2^21 rows at fi = 128, 2^20 at fi = 256; larger
            // batches take the general form below, decided here, before anything of the layer is enqueued)
            const bool classes = p.size() >= 10 && options().pna_fold_lin && options().pna_classes && whole && ws->deg_ready && M > 0 && !fpx &&
                                 ws->deg_delta == model->desc.pna_delta && fo > 32 && (uint64_t)M * 16 * fi + 512 <= 0xffffffffull;
            if (!classes && (rc = ws_linear1(R(cur, fi), fi, fi, p[0], 2 * fi, p[1], nullptr, Rw(q, fi), M, fi, GNNB_ACT_NONE, stream)))
                return rc;
            // the source half p = x . Wb^T and its aggregate: in one kernel, p on chip, where the degree-class form (no destination
            // term) and the max_graph_nodes promise (whole graphs in a stage) allow; else GEMM -> [N, F] -> aggregate
            bool pagg = false;
            if (classes) {
                const Attempt at = attempt(launch_pna_pagg(ws->t, cur, fi, p[0] + fi, 2 * fi, ws->agg, (hipStream_t)stream), "PNA product + aggregate");
                if (at == FAILED)
                    return GNNB_ERR_HIP;
                pagg = at == TOOK;
            }
            if (!pagg) {
                if ((rc = ws_linear1(R(cur, fi), fi, fi, p[0] + fi, 2 * fi, nullptr, nullptr, Rw(pp, fi), M, fi, GNNB_ACT_NONE, stream)))
                    return rc;
                if ((rc = aggregate(GNNB_AGG_PNA, pp, classes ? nullptr : q, ws->agg, fi, 0.f)))
                    return rc;
            }
            // [x | A | amp.A | att.A] . Wpost^T without materialising the 13F concat
            gnnb_gemm_seg segs[4] = {{R(cur, fi), nullptr, fi, fi},
                                     {R(ws->agg, 4 * fi), nullptr, 4 * fi, 4 * fi},
                                     {R(ws->agg, 4 * fi), ws->t.amp + row_lo, 4 * fi, 4 * fi},
                                     {R(ws->agg, 4 * fi), ws->t.att + row_lo, 4 * fi, 4 * fi}};
            if (classes) {
                // degree-class form (gnnb_workspace_set_max_degree): [x | A] . W_class^T over the class-sorted rows, written to
                // the rows' own places; skip + activation in the epilogue (the last layer pools in the pass behind)
                gnnb_gemm_seg s2[2] = {{cur, nullptr, fi, fi}, {ws->agg, nullptr, 4 * fi, 4 * fi}};
                GemmArgs g;
                if ((rc = build_gemm(g, s2, 2, p[8], 5 * fi)))
                    return rc;
                RowClasses rcl;
                rcl.perm = ws->deg_perm;
                rcl.tile_cls = ws->deg_tile_cls;
                rcl.w_stride = (long)fo * 5 * fi;
                rcl.bias_stride = fo;
                hipError_t he = launch_linear(g, p[8], 5 * fi, p[9], skip_fold ? nullptr : skip, nxt, ws->deg_max_tiles * 128, fo, d.activation,
                                              (hipStream_t)stream, nullptr, &rcl, sko);
                if (he == hipSuccess)
                    break;
                // (no way back from here: the aggregate above ran without the destination term)
                return fail(GNNB_ERR_HIP, "degree-class GEMM launch failed: %s", hipGetErrorString(he));
            }
            if (p.size() >= 8 && options().pna_fold_lin) {
                // `lin` folded into the post-NN at upload (gnnb_model_create): one GEMM, skip + activation in its epilogue;
                // the last layer of a whole-batch run pools there too (as GraphSAGE's)
                if (pooled_in_epilogue && whole && l == d.num_layers - 1 && !fpx && options().fuse_pool && ws->t.node_graph && ws->pool_part && skip == nullptr) {
                    GemmArgs g;
                    if ((rc = build_gemm(g, segs, 4, p[6], 13 * fi)))
                        return rc;
                    const PoolEpilogue pe = pool_epilogue(ws, d);
                    const Attempt at = attempt(launch_linear(g, p[6], 13 * fi, p[7], nullptr, nxt, M, fo, d.activation, (hipStream_t)stream, &pe), "pooling GEMM");
                    if (at == FAILED)
                        return GNNB_ERR_HIP;
                    if (at == TOOK) {
                        GNNB_HIP_TRY(launch_pool_combine(pe, M, fo, (hipStream_t)stream));
                        *pooled_in_epilogue = true;
                        break;
                    }
                }
                if ((rc = ws_linear(segs, 4, p[6], 13 * fi, p[7], skip_fold ? nullptr : R(skip, fo), Rw(nxt, fo), M, fo, d.activation, stream)))
                    return rc;
                break;
            }
            float *hid = ws->tmp0; // q is dead after the aggregate
            if ((rc = ws_linear(segs, 4, p[2], 13 * fi, p[3], nullptr, Rw(hid, fo), M, fo, GNNB_ACT_NONE, stream)))
                return rc;
            if ((rc = ws_linear1(R(hid, fo), fo, fo, p[4], fo, p[5], R(skip, fo), Rw(nxt, fo), M, fo, d.activation, stream)))
                return rc;
            break;
        }
        }
        if ((rc = quantize(d, Rw(nxt, fo), (size_t)M * fo, stream)))
            return rc;
        cur = nxt;
        which ^= 1;
    }

    *out_cur = cur;
    return GNNB_OK;
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
        const std::vector<const float *> &p = model->conv[l];
        const float *skip = (d.skip && l != 0 && l != d.num_layers - 1) ? cur : nullptr;
        float *nxt = ws->act[which];
        if ((const float *)nxt == cur) {
            which ^= 1;
            nxt = ws->act[which];
        }
        const bool gin = d.conv_type == GNNB_CONV_GIN;
        hipError_t he = launch_conv_rows(ws->t, d.conv_type, cur, ld.fin, p[0], p[1], gin ? p[2] : nullptr, gin ? p[3] : nullptr,
                                         ld.fout, skip, nxt, ws->large_n, d.activation, d.gin_eps, s);
        if (he != hipSuccess)
            return he; // (NotSupported can only come from the first layer's checks above: nothing is half done)
        cur = nxt;
        which ^= 1;
    }
    const int gw = gnn_out_width(d), B = ws->t.num_graphs;
    return launch_global_pool(cur, ws->t.graph_ptr + ws->large_g, B - ws->large_g, gw, d.pools, d.num_pools,
                              ws->pooled + (size_t)ws->large_g * d.num_pools * gw, s);
}

// The batch tables restricted to the graphs the max_graph_nodes promise covers: everything, or -- with a large segment --
// graphs [0, large_g) = nodes [0, large_n) = edges [0, large_e).  The stack kernels clamp every table entry to these
// counts, so a tile that begins in the small segment ends at its last node.
static BatchTables small_segment(const gnnb_workspace *ws)
{
    BatchTables t = ws->t;
    if (ws->large_g >= 0 && ws->large_g < t.num_graphs) {
        t.num_graphs = ws->large_g;
        t.num_nodes = ws->large_n;
        t.num_edges = ws->large_e;
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
        he = launch_gcn2_zf(t, x_dev, d.in_dim, model->conv[0][0], model->conv[0][1], d.hidden_dim, model->conv[1][0],
                            model->conv[1][1], d.out_dim, d.activation, d.pools, d.num_pools, ws->pooled, s, model->zf_w1f,
                            offer ? &head : nullptr, offer ? model->head_dev : nullptr, offer ? head_out : nullptr, head_fused);
    }
    *path = GNNB_PATH_STACK_ZF;
    if (he == hipErrorNotSupported) {
        *path = GNNB_PATH_STACK;
        he = launch_gcn2_fused(t, x_dev, d.in_dim, model->conv[0][0], model->conv[0][1], d.hidden_dim,
                               model->conv[L - 1][0], model->conv[L - 1][1], d.out_dim, d.activation, d.pools,
                               d.num_pools, ws->pooled, s, deep);
    }
    return he;
}

// The readout of graphs [g0, B) from the pooled matrix in one launch (k_head_small / k_pool_mlp's pre-pooled form);
// hipErrorNotSupported (nothing launched) when the head does not fit it
static hipError_t launch_readout_pooled(const gnnb_model *model, gnnb_workspace *ws, int g0, float *out_dev, hipStream_t s)
{
    const gnnb_model_desc &d = model->desc;
    const int gw = gnn_out_width(d);
    return launch_pool_mlp(nullptr, ws->t.graph_ptr + g0, ws->t.num_graphs - g0, gw, d.pools, d.num_pools, model_head_args(model), d.mlp_activation,
                           out_dev + (size_t)g0 * d.mlp_out, s, ws->pooled + (size_t)g0 * d.num_pools * gw);
}

// ... and as a plain GEMM chain (a head too large for the readout kernels; the fixed-point emulation, each layer's output put
// on the grid).  Through the stand-alone GEMM entry: the head's GEMMs never use the workspace's stream-K scratch.
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
        if ((rc = linear1(h, din, din, model->head_w[i], din, model->head_b[i], nullptr, y, M, dout,
                          last ? GNNB_ACT_NONE : d.mlp_activation, stream)))
            return rc;
        if ((rc = quantize(d, y, (size_t)M * dout, stream)))
            return rc;
        h = y;
    }
    return GNNB_OK;
}

static int forward_prepared_body(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, float *out_dev,
                                 void *stream);

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

int gnnb_forward_prepared(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev,
                          float *out_dev, void *stream)
{
    // every launch below runs in the MODEL's math mode; the reduced modes' kernels flag this workspace
    MathScope math_scope(model ? model->desc.math : -1, ws ? ws->t.err : nullptr, ws ? ws->t.err_host_dev : nullptr);
    int rc = forward_prepared_body(model, ws, x_dev, out_dev, stream);
    if (rc != GNNB_OK)
        return rc;
    // output_activation(dim=-1) over every graph's output row (models.py:572-573)
    if (model->desc.output_activation != GNNB_OUT_NONE)
        GNNB_HIP_TRY(launch_output_activation(out_dev, ws->t.num_graphs, model->desc.mlp_out, model->desc.output_activation,
                                              (hipStream_t)stream));
    return GNNB_OK;
}

static int forward_prepared_body(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, float *out_dev,
                                 void *stream)
{
    if (!model || !ws || !x_dev || !out_dev)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward");
    if (!ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    if (memcmp(&model->desc, &ws->desc, sizeof(gnnb_model_desc)) != 0)
        return fail(GNNB_ERR_INVALID, "workspace was created for a different model");
    const gnnb_model_desc &d = model->desc;
    const int N = ws->t.num_nodes, B = ws->t.num_graphs;
    int rc;
    const bool fpx = d.fpx_w > 0;
    if (fpx) { // the input features enter as F_TYPE values: a quantised copy (the caller's buffer is not written)
        GNNB_HIP_TRY(launch_quantize(x_dev, ws->act[1], (size_t)N * d.in_dim, d.fpx_w, d.fpx_i, (hipStream_t)stream));
        x_dev = ws->act[1]; // (the layer loop never writes the buffer it reads)
    }

    // ---- fused path: the whole GCN stack (two or more layers) + pooling in one persistent kernel, then the MLP head
    const G2Deep deep = gcn_stack_middle_layers(model);
    // With a large segment (graphs the promise does not cover, ordered last by the caller) the stack runs on the graphs
    // in front of it and the large ones go layer by layer into the same pooled matrix: one oversized molecule no longer
    // sends the whole batch down the layer-by-layer path.  (large_g = 0: every graph is large -> layer by layer below.)
    const bool seg = ws->large_g >= 0 && ws->large_g < B;
    if (!fpx && deep.nl >= 2 && d.mlp_num_linear <= 8 && !(seg && ws->large_g == 0)) {
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
        if (he == hipSuccess) {
            if (seg && !forked && options().large_fork == 2) { // the small kernels on the caller's stream, behind the stack
                hipError_t hl = large_segment_small(model, ws, x_dev, (hipStream_t)stream);
                if (hl != hipSuccess && hl != hipErrorNotSupported)
                    return fail(GNNB_ERR_HIP, "large-segment launch failed: %s", hipGetErrorString(hl));
                forked = hl == hipSuccess;
            }
            if (seg && forked) {
                ws->last_path |= GNNB_PATH_LARGE_LAYERWISE;
            } else if (seg) {
                const float *lcur = nullptr;
                if ((rc = run_conv_layers(model, ws, x_dev, ws->large_n, ws->large_n / ws->t.tile_rows, &lcur, stream)))
                    return rc;
                const int gwl = gnn_out_width(d);
                GNNB_HIP_TRY(launch_global_pool(lcur, ws->t.graph_ptr + ws->large_g, B - ws->large_g, gwl, d.pools, d.num_pools,
                                                ws->pooled + (size_t)ws->large_g * d.num_pools * gwl, (hipStream_t)stream));
                ws->last_path |= GNNB_PATH_LARGE_LAYERWISE;
            }
            // (the stack kernel ran the head on its own graphs: what is left are the graphs of the large segment, if any)
            const int hg0 = head_fused ? (seg ? ws->large_g : B) : 0;
            if (hg0 >= B)
                return GNNB_OK;
            const Attempt at = attempt(launch_readout_pooled(model, ws, hg0, out_dev, (hipStream_t)stream), "readout");
            if (at != DECLINED)
                return at == TOOK ? GNNB_OK : GNNB_ERR_HIP;
            // head too large for the fused readout: plain GEMM chain on the pooled matrix (no fixed-point emulation on this route)
            return run_head_chain(model, ws, hg0, out_dev, stream);
        }
        if (attempt(he, "fused GCN stack") == FAILED)
            return GNNB_ERR_HIP;
    }

    ws->last_path = GNNB_PATH_LAYERWISE;
    const float *cur = nullptr;
    bool pooled_done = false;
    if ((rc = run_conv_layers(model, ws, x_dev, 0, 0, &cur, stream, &pooled_done)))
        return rc;

    const int gw = gnn_out_width(d);
    const bool head_fits = d.mlp_num_linear <= 8; // (what a HeadArgs holds)
    if (pooled_done && head_fits) {
        // (the last layer's GEMM pooled in its epilogue: ws->pooled is complete, the readout takes it as the stack path does)
        const Attempt at = attempt(launch_readout_pooled(model, ws, 0, out_dev, (hipStream_t)stream), "readout");
        if (at != DECLINED)
            return at == TOOK ? GNNB_OK : GNNB_ERR_HIP;
    } else if (!pooled_done && !fpx && head_fits) {
        // fused readout (pooling + whole MLP head, one launch) when the head fits LDS
        hipError_t he = hipErrorNotSupported;
        if (options().head_split) {
            // pooling pass (HBM-bound, every CU) + the small readout on the pooled matrix: neither needs the
            // 119 KB of LDS of the one-launch form, so both share CUs with other batches' kernels
            if ((rc = gnnb_global_pool(ws, cur, gw, d.pools, d.num_pools, ws->pooled, stream)))
                return rc;
            he = launch_readout_pooled(model, ws, 0, out_dev, (hipStream_t)stream);
        } else {
            he = launch_pool_mlp(cur, ws->t.graph_ptr, B, gw, d.pools, d.num_pools, model_head_args(model), d.mlp_activation, out_dev,
                                 (hipStream_t)stream);
        }
        Attempt at = attempt(he, "fused readout");
        if (at != DECLINED)
            return at == TOOK ? GNNB_OK : GNNB_ERR_HIP;
        // The head's weights do not fit LDS (SAGE d = 256 with three pools: 768 x 64 floats): pooling pass, then
        // the small readout that takes its weights from L2 as MFMA operands -- one launch over B / 16 workgroups
        // instead of a chain of GEMMs with M = B rows (64 workgroups of the 128-row tile at B = 8192: 51 us)
        if (!options().head_split && options().head_small) {
            if ((rc = gnnb_global_pool(ws, cur, gw, d.pools, d.num_pools, ws->pooled, stream)))
                return rc;
            at = attempt(launch_readout_pooled(model, ws, 0, out_dev, (hipStream_t)stream), "readout");
            if (at != DECLINED)
                return at == TOOK ? GNNB_OK : GNNB_ERR_HIP;
            pooled_done = true;
        }
    }
    if (!pooled_done && (rc = gnnb_global_pool(ws, cur, gw, d.pools, d.num_pools, ws->pooled, stream)))
        return rc;
    if ((rc = quantize(d, ws->pooled, (size_t)B * d.num_pools * gw, stream)))
        return rc;
    return run_head_chain(model, ws, 0, out_dev, stream);
}

int gnnb_forward_batched(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev,
                         const int32_t *coo_dev, const int32_t *node_ptr_dev,
                         const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                         float *out_dev, void *stream)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_batched");
    int rc = gnnb_graph_prep(ws, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes,
                             num_edges, model->desc.pna_delta, stream);
    if (rc != GNNB_OK)
        return rc;
    return gnnb_forward_prepared(model, ws, x_dev, out_dev, stream);
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
    int rc = graph_prep_impl(ws_next, coo_dev, node_ptr_dev, edge_ptr_dev, num_graphs, num_nodes, num_edges, model->desc.pna_delta, stream, &pp);
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
    if (num_graphs > ws->max_graphs || num_nodes > ws->max_nodes || num_edges > ws->max_edges)
        return fail(GNNB_ERR_CAPACITY,
                    "batch (%d graphs, %d nodes, %d edges) exceeds workspace (%d, %d, %d)",
                    num_graphs, num_nodes, num_edges, ws->max_graphs, ws->max_nodes, ws->max_edges);
    const gnnb_model_desc &d = model->desc;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    // staging buffers live in the workspace, sized once for its capacities: the reference's <name>_top is called once
    // per graph (model_tb.cpp.jinja:189-205), and a hipMalloc / hipFree pair per call would dominate it
    const size_t cx = up((size_t)ws->max_nodes * d.in_dim * 4), cc = up((size_t)std::max(ws->max_edges, 1) * 8),
                 cp = up(((size_t)ws->max_graphs + 1) * 4), co = up((size_t)ws->max_graphs * d.mlp_out * 4);
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

// ---------------------------------------------------------------------------------------
} // extern "C"

// The event-timed loop behind the *_timed entries: `warmup` launches, then `iters` launches between two events on `s`;
// launch(i) -> GNNB_OK or an error (which ends the loop and is returned).  *out_us = microseconds per launch.
template <typename F> static int timed_loop(hipStream_t s, int warmup, int iters, F launch, float *out_us)
{
    struct Events { // (destroyed on every return path)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events()
        {
            if (e0)
                (void)hipEventDestroy(e0);
            if (e1)
                (void)hipEventDestroy(e1);
        }
    } ev;
    GNNB_HIP_TRY(hipEventCreate(&ev.e0));
    GNNB_HIP_TRY(hipEventCreate(&ev.e1));
    int rc = GNNB_OK;
    for (int i = 0; i < warmup && rc == GNNB_OK; i++)
        rc = launch(i);
    if (rc != GNNB_OK)
        return rc;
    GNNB_HIP_TRY(hipStreamSynchronize(s));
    GNNB_HIP_TRY(hipEventRecord(ev.e0, s));
    for (int i = 0; i < iters && rc == GNNB_OK; i++)
        rc = launch(i);
    GNNB_HIP_TRY(hipEventRecord(ev.e1, s));
    GNNB_HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    GNNB_HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *out_us = ms * 1000.0f / (float)iters;
    return rc;
}

extern "C" {

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

int gnnb_gcn_stack_timed(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, int iters,
                         void *stream, float *out_us_per_launch)
{
    if (!model || !ws || !x_dev || iters < 1 || !out_us_per_launch)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_gcn_stack_timed");
    MathScope math_scope(model->desc.math, ws->t.err, ws->t.err_host_dev);
    if (!ws->prepared)
        return fail(GNNB_ERR_INVALID, "workspace has no prepared batch");
    const G2Deep deep = gcn_stack_middle_layers(model);
    if (deep.nl < 2)
        return fail(GNNB_ERR_INVALID, "the fused stack exists for GCN / GIN models of two or more layers");
    // (as the forward launches it: with the MLP head inside where k_gcn2_zf takes it; its output goes to a workspace buffer)
    bool head_fused = false;
    return timed_loop((hipStream_t)stream, 3, iters, [&](int) {
        const Attempt at = attempt(launch_conv_stack(model, ws, small_segment(ws), x_dev, deep, (hipStream_t)stream, &ws->last_path, ws->mlp[0], &head_fused),
                                   "fused GCN stack");
        if (at == DECLINED)
            return fail(GNNB_ERR_INVALID, "fused stack not eligible (shape, or no max_graph_nodes promise)");
        return at == TOOK ? (int)GNNB_OK : (int)GNNB_ERR_HIP;
    }, out_us_per_launch);
}

int gnnb_linear_timed(const float *a_dev, int lda, int k, const float *w_dev, int ldw,
                      const float *bias_dev, float *y_dev, int M, int N, int act, int iters,
                      void *stream, float *out_us_per_launch)
{
    if (iters < 1 || !out_us_per_launch)
        return fail(GNNB_ERR_INVALID, "bad argument to gnnb_linear_timed");
    return timed_loop((hipStream_t)stream, 3, iters, [&](int) { return linear1(a_dev, lda, k, w_dev, ldw, bias_dev, nullptr, y_dev, M, N, act, stream); },
                      out_us_per_launch);
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
