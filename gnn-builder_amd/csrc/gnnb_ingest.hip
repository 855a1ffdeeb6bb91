// gnnb_ingest.hip -- the PyG mini-batch entries of libgnnb_hip.so: the workspace's add-on allocations, the device ingest
// (gnnb_hip.h; k_ingest.hip), the ingest with the oversized graphs ordered last (gnnb_order.h; k_order.hip) and the ingest that
// carries a GINE model's edge attributes (gnnb_edge.h; k_ingest.hip's edge-attribute pass), each with its forward.  Host only, no
// kernels.  (gnnb_runtime.hip: workspace, graph prep, flags; gnnb_forward.hip: the forward behind forward_batched_tail.)
#include <algorithm>
#include <cstring>

#include "gnnb_host.h"

using namespace gnnb;

// One add-on allocation of a workspace, made once, right after gnnb_workspace_create: GNNB_OK with ws->*slot set, by this call or
// by an earlier one.  entry, addon, alloc: the names in the messages.
static int enable_addon(gnnb_workspace *ws, char *gnnb_workspace::*slot, size_t bytes, const char *entry, const char *addon, const char *alloc)
{
    if (!ws)
        return fail(GNNB_ERR_INVALID, "null workspace");
    if (ws->*slot)
        return GNNB_OK; // (enabled already: the allocation is made once)
    if (ws->prepared)
        return fail(GNNB_ERR_INVALID, "%s: the workspace is in use (a batch has been prepared on it); enable %s right after gnnb_workspace_create",
                    entry, addon);
    char *blob = nullptr;
    const hipError_t e = hipMalloc((void **)&blob, bytes);
    if (e != hipSuccess)
        return fail(GNNB_ERR_HIP, "%s allocation of %zu bytes failed: %s", alloc, bytes, hipGetErrorString(e));
    ws->*slot = blob;
    return GNNB_OK;
}

// ... will it allocate?  (What an add-on needs beside its blob -- the base ingest, the host-mapped triple -- is made in front of
// the blob, under this: a call that enable_addon refuses or answers at once makes nothing.)
static bool addon_pending(const gnnb_workspace *ws, char *gnnb_workspace::*slot) { return ws && !(ws->*slot) && !ws->prepared; }

extern "C" {

// ---------------------------------------------------------------------------------------
// PyG mini-batches (k_ingest.hip)
size_t gnnb_ingest_bytes(int max_graphs, int max_nodes, int max_edges)
{
    if (max_graphs < 0 || max_nodes < 0 || max_edges < 0)
        return 0;
    IngestParams p;
    return ingest_place(nullptr, max_graphs, max_nodes, max_edges, p);
}

int gnnb_workspace_enable_ingest(gnnb_workspace *ws)
{
    const bool pending = addon_pending(ws, &gnnb_workspace::ingest_blob);
    IngestParams p;
    const int rc = enable_addon(ws, &gnnb_workspace::ingest_blob, pending ? ingest_place(ws, p) : 0, "gnnb_workspace_enable_ingest", "ingest", "ingest");
    if (rc != GNNB_OK || !pending)
        return rc;
    (void)ingest_place(ws, p);
    // (synchronous, as the stream-K scratch's: joins no other stream)
    const hipError_t e = hipMemset(p.state, 0, INGEST_STATE_WORDS * 4);
    if (e != hipSuccess) {
        (void)hipFree(ws->ingest_blob);
        ws->ingest_blob = nullptr;
        return fail(GNNB_ERR_HIP, "ingest state initialisation failed: %s", hipGetErrorString(e));
    }
    return GNNB_OK;
}

int gnnb_ingest_pyg(gnnb_workspace *ws, const int64_t *edge_index_dev, const int64_t *batch_dev, const int64_t *ptr_dev,
                    int num_graphs, int num_nodes, int num_edges, const int32_t **coo_dev, const int32_t **node_ptr_dev,
                    const int32_t **edge_ptr_dev, void *stream)
{
    if (!ws || !coo_dev || !node_ptr_dev || !edge_ptr_dev || (num_edges > 0 && !edge_index_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_ingest_pyg");
    if (!ws->ingest_blob)
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg: call gnnb_workspace_enable_ingest on the workspace first");
    if (const int rc = check_batch_sizes(ws, num_graphs, num_nodes, num_edges))
        return rc;
    if (batch_dev && ptr_dev)
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg takes batch or ptr, not both");
    if (num_nodes == 0)
        batch_dev = nullptr; // (no node: every node_ptr entry is 0; an empty `batch` may come without an address -- torch gives none)
    else if (!batch_dev && !ptr_dev && num_graphs > 1)
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg needs batch or ptr for a batch of %d graphs", num_graphs);
    if ((num_graphs == 0 && (num_nodes > 0 || num_edges > 0)) || (num_nodes == 0 && num_edges > 0))
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg: %d nodes and %d edges in %d graphs", num_nodes, num_edges, num_graphs);
    if (const int rc = report_earlier_flags(ws, stream)) // (before anything is enqueued, as gnnb_graph_prep does)
        return rc;
    IngestParams p;
    memset(&p, 0, sizeof(p));
    (void)ingest_place(ws, p);
    p.src = (const long long *)edge_index_dev;
    p.dst = p.src + num_edges;
    p.batch = (const long long *)batch_dev;
    p.ptr = (const long long *)ptr_dev;
    p.B = num_graphs, p.N = num_nodes, p.E = num_edges;
    p.err = ws->t.err, p.err_host = ws->t.err_host_dev;
    GNNB_HIP_TRY(launch_ingest(p, (hipStream_t)stream));
    ws->ingested = true;
    *coo_dev = (const int32_t *)p.coo;
    *node_ptr_dev = p.node_ptr;
    *edge_ptr_dev = p.edge_ptr;
    return GNNB_OK;
}

// (the tails of the three forwards below: the ingest has reported what EARLIER batches left; its own kernels may have flagged this
// batch by now, which is for the next call (or gnnb_workspace_check) to report, not for the prep of this one -- ingest_reported)
int gnnb_forward_pyg(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                     const int64_t *batch_dev, const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges, float *out_dev,
                     void *stream)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_pyg");
    if (const int rc = refuse_edge_model(model, ws, "gnnb_forward_pyg", "gnnb_forward_pyg_edges"))
        return rc;
    if (const int rc = refuse_rgcn_model(model, ws, "gnnb_forward_pyg", "gnnb_forward_pyg_types"))
        return rc;
    const int32_t *coo = nullptr, *node_ptr = nullptr, *edge_ptr = nullptr;
    if (const int rc = gnnb_ingest_pyg(ws, edge_index_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, &coo, &node_ptr, &edge_ptr, stream))
        return rc;
    return forward_batched_tail(model, ws, x_dev, nullptr, coo, node_ptr, edge_ptr, num_graphs, num_nodes, num_edges, out_dev, stream, true);
}

// ---------------------------------------------------------------------------------------
// PyG mini-batches with the oversized graphs ordered last (k_order.hip)
size_t gnnb_order_bytes(int max_graphs, int max_nodes, int max_edges, int in_dim, int mlp_out)
{
    if (max_graphs < 0 || max_nodes < 0 || max_edges < 0 || in_dim < 0 || mlp_out < 0)
        return 0;
    OrderParams p;
    return order_place(nullptr, max_graphs, max_nodes, max_edges, in_dim, mlp_out, p);
}

int gnnb_workspace_enable_ordered_ingest(gnnb_workspace *ws)
{
    if (addon_pending(ws, &gnnb_workspace::order_blob)) {
        if (const int rc = gnnb_workspace_enable_ingest(ws))
            return rc;
        // the triple comes back through host-mapped memory (as the flag word does): required here, the launches behind it are sized
        // by it.  (Kept by the workspace should the blob's allocation fail below: the next call finds it.)
        if (!ws->order_triple) {
            int32_t *triple = nullptr;
            void *dp = nullptr;
            hipError_t e = hipHostMalloc((void **)&triple, 64, hipHostMallocMapped);
            if (e == hipSuccess)
                e = hipHostGetDevicePointer(&dp, triple, 0);
            if (e != hipSuccess || !dp) {
                if (triple)
                    (void)hipHostFree(triple);
                (void)hipGetLastError();
                return fail(GNNB_ERR_HIP, "host-mapped block of the ordered ingest failed: %s", hipGetErrorString(e));
            }
            triple[0] = triple[1] = triple[2] = 0;
            ws->order_triple = triple;
            ws->order_triple_dev = (int32_t *)dp;
        }
    }
    OrderParams p;
    return enable_addon(ws, &gnnb_workspace::order_blob, ws && !ws->order_blob ? order_place(ws, p) : 0, "gnnb_workspace_enable_ordered_ingest",
                        "the ordered ingest", "ordered-ingest");
}

int gnnb_ingest_pyg_ordered(gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev, const int64_t *batch_dev,
                            const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges, const float **x_ord_dev,
                            const int32_t **coo_dev, const int32_t **node_ptr_dev, const int32_t **edge_ptr_dev, const int32_t **perm_dev,
                            int *first_graph, int *first_node, int *first_edge, void *stream)
{
    if (!ws || !x_ord_dev || !coo_dev || !node_ptr_dev || !edge_ptr_dev || !perm_dev || !first_graph || !first_node || !first_edge ||
        (num_nodes > 0 && !x_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_ingest_pyg_ordered");
    if (!ws->order_blob)
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg_ordered: call gnnb_workspace_enable_ordered_ingest on the workspace first");
    // the triple is read on the host behind a wait: not under capture (nothing has been enqueued yet)
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg_ordered waits for its kernels and cannot be captured into a graph");
    }
    const int32_t *coo = nullptr, *node_ptr = nullptr, *edge_ptr = nullptr;
    if (const int rc = gnnb_ingest_pyg(ws, edge_index_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, &coo, &node_ptr, &edge_ptr, stream))
        return rc;
    OrderParams p;
    memset(&p, 0, sizeof(p));
    (void)order_place(ws, p);
    p.node_ptr = node_ptr, p.edge_ptr = edge_ptr, p.coo = (const int2 *)coo;
    p.x = x_dev;
    p.batch = num_nodes > 0 ? (const long long *)batch_dev : nullptr;
    p.B = num_graphs, p.N = num_nodes, p.E = num_edges, p.in_dim = ws->desc.in_dim;
    p.limit = ws->max_graph_nodes; // the promise as it stands at this call
    p.triple = ws->order_triple_dev;
    GNNB_HIP_TRY(launch_order(p, (hipStream_t)stream));
    GNNB_HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); // the one synchronisation of the path
    *first_graph = ((volatile int32_t *)ws->order_triple)[0];
    *first_node = ((volatile int32_t *)ws->order_triple)[1];
    *first_edge = ((volatile int32_t *)ws->order_triple)[2];
    *x_ord_dev = p.x_ord;
    *coo_dev = (const int32_t *)p.coo_ord;
    *node_ptr_dev = p.node_ptr_ord;
    *edge_ptr_dev = p.edge_ptr_ord;
    *perm_dev = p.perm;
    return GNNB_OK;
}

int gnnb_forward_pyg_ordered(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                             const int64_t *batch_dev, const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges,
                             float *out_dev, void *stream)
{
    if (!model || !ws || (num_graphs > 0 && !out_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_pyg_ordered");
    if (const int rc = refuse_edge_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg_edges"))
        return rc;
    if (const int rc = refuse_gat_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg"))
        return rc;
    if (const int rc = refuse_gatconv_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg"))
        return rc;
    if (const int rc = refuse_transformer_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg"))
        return rc;
    if (const int rc = refuse_resgated_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg"))
        return rc;
    if (const int rc = refuse_ggnn_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg"))
        return rc;
    if (const int rc = refuse_rgcn_model(model, ws, "gnnb_forward_pyg_ordered", "gnnb_forward_pyg_types"))
        return rc;
    const float *x_ord = nullptr;
    const int32_t *coo = nullptr, *node_ptr = nullptr, *edge_ptr = nullptr, *perm = nullptr;
    int g0 = 0, n0 = 0, e0 = 0;
    if (const int rc = gnnb_ingest_pyg_ordered(ws, x_dev, edge_index_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, &x_ord, &coo,
                                               &node_ptr, &edge_ptr, &perm, &g0, &n0, &e0, stream))
        return rc;
    // nothing large: no segment, the batch runs exactly as gnnb_forward_pyg would run it
    if (const int rc = g0 == num_graphs ? gnnb_workspace_set_large_segment(ws, -1, -1, -1) : gnnb_workspace_set_large_segment(ws, g0, n0, e0))
        return rc;
    OrderParams placed;
    (void)order_place(ws, placed);
    float *out_ord = placed.out_ord;
    if (const int rc = forward_batched_tail(model, ws, x_ord, nullptr, coo, node_ptr, edge_ptr, num_graphs, num_nodes, num_edges, out_ord, stream, true))
        return rc;
    GNNB_HIP_TRY(launch_order_out(out_ord, perm, out_dev, num_graphs, ws->desc.mlp_out, (hipStream_t)stream));
    return GNNB_OK;
}

// ---------------------------------------------------------------------------------------
// GINE models: PyG mini-batches with edge attributes (gnnb_edge.h; k_edge_attr_order of k_ingest.hip)
size_t gnnb_edge_ingest_bytes(int max_edges, int edge_dim)
{
    if (max_edges < 0 || edge_dim < 1 || edge_dim > 16)
        return 0;
    return arena_up((size_t)std::max(max_edges, 1) * (size_t)edge_dim * sizeof(float));
}

int gnnb_workspace_enable_edge_ingest(gnnb_workspace *ws)
{
    if (ws && !ws->edge_blob && !ws->edge_dim)
        return fail(GNNB_ERR_INVALID, "gnnb_workspace_enable_edge_ingest: the workspace belongs to a model without edge weights "
                                      "(gnnb_edge_model_create makes one with)");
    if (addon_pending(ws, &gnnb_workspace::edge_blob))
        if (const int rc = gnnb_workspace_enable_ingest(ws))
            return rc;
    return enable_addon(ws, &gnnb_workspace::edge_blob, ws ? gnnb_edge_ingest_bytes(ws->max_edges, ws->edge_dim) : 0,
                        "gnnb_workspace_enable_edge_ingest", "the edge ingest", "edge-ingest");
}

int gnnb_ingest_pyg_edges(gnnb_workspace *ws, const int64_t *edge_index_dev, const float *edge_attr_dev, const int64_t *batch_dev,
                          const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges, const int32_t **coo_dev,
                          const int32_t **node_ptr_dev, const int32_t **edge_ptr_dev, const float **edge_attr_ord_dev, void *stream)
{
    if (!ws || !edge_attr_ord_dev || (num_edges > 0 && !edge_attr_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_ingest_pyg_edges");
    if (!ws->edge_blob)
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg_edges: call gnnb_workspace_enable_edge_ingest on the workspace first");
    if (const int rc = gnnb_ingest_pyg(ws, edge_index_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, coo_dev, node_ptr_dev, edge_ptr_dev, stream))
        return rc;
    // the rows follow their edges: the general path's last pass left sorted position -> input edge in one half of idx (which half:
    // launch_ingest's pass count); whether that path ran at all is the state word, read by the kernel
    IngestParams p;
    (void)ingest_place(ws, p);
    const int passes = ingest_sort_passes(num_graphs);
    const int32_t *idx = (passes == 0 || num_edges < 2) ? nullptr : p.idx[passes & 1];
    GNNB_HIP_TRY(launch_edge_attr_order(edge_attr_dev, idx, p.state, (float *)ws->edge_blob, num_edges, ws->edge_dim, (hipStream_t)stream));
    *edge_attr_ord_dev = (const float *)ws->edge_blob;
    return GNNB_OK;
}

int gnnb_forward_pyg_edges(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                           const float *edge_attr_dev, const int64_t *batch_dev, const int64_t *ptr_dev, int num_graphs, int num_nodes,
                           int num_edges, float *out_dev, void *stream)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_pyg_edges");
    if (const int rc = refuse_rgcn_model(model, ws, "gnnb_forward_pyg_edges", "gnnb_forward_pyg_types"))
        return rc;
    if (!model->edge_dim || model->edge_dim != ws->edge_dim)
        return fail(GNNB_ERR_INVALID, "gnnb_forward_pyg_edges takes a model of gnnb_edge_model_create and its workspace");
    const int32_t *coo = nullptr, *node_ptr = nullptr, *edge_ptr = nullptr;
    const float *edge_attr = nullptr;
    if (const int rc = gnnb_ingest_pyg_edges(ws, edge_index_dev, edge_attr_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, &coo, &node_ptr,
                                             &edge_ptr, &edge_attr, stream))
        return rc;
    return forward_batched_tail(model, ws, x_dev, edge_attr, coo, node_ptr, edge_ptr, num_graphs, num_nodes, num_edges, out_dev, stream, true);
}

// ---------------------------------------------------------------------------------------
// RGCNConv models: PyG mini-batches with integer edge types (gnnb_rgcn.h; k_edge_type_order of k_ingest.hip)
size_t gnnb_type_ingest_bytes(int max_edges)
{
    if (max_edges < 0)
        return 0;
    return arena_up((size_t)std::max(max_edges, 1) * sizeof(int32_t));
}

int gnnb_workspace_enable_type_ingest(gnnb_workspace *ws)
{
    if (ws && !ws->type_blob && !ws->rgcn_relations)
        return fail(GNNB_ERR_INVALID, "gnnb_workspace_enable_type_ingest: the workspace belongs to a model without relations "
                                      "(gnnb_rgcn_model_create makes one with)");
    if (addon_pending(ws, &gnnb_workspace::type_blob))
        if (const int rc = gnnb_workspace_enable_ingest(ws))
            return rc;
    return enable_addon(ws, &gnnb_workspace::type_blob, ws ? gnnb_type_ingest_bytes(ws->max_edges) : 0, "gnnb_workspace_enable_type_ingest",
                        "the type ingest", "type-ingest");
}

int gnnb_ingest_pyg_types(gnnb_workspace *ws, const int64_t *edge_index_dev, const int64_t *edge_type_dev, const int64_t *batch_dev,
                          const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges, const int32_t **coo_dev,
                          const int32_t **node_ptr_dev, const int32_t **edge_ptr_dev, const int32_t **edge_type_ord_dev, void *stream)
{
    if (!ws || !edge_type_ord_dev || (num_edges > 0 && !edge_type_dev))
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_ingest_pyg_types");
    if (!ws->type_blob)
        return fail(GNNB_ERR_INVALID, "gnnb_ingest_pyg_types: call gnnb_workspace_enable_type_ingest on the workspace first");
    if (const int rc = gnnb_ingest_pyg(ws, edge_index_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, coo_dev, node_ptr_dev, edge_ptr_dev, stream))
        return rc;
    // the types follow their edges, as gnnb_ingest_pyg_edges' attribute rows do: which path ran is the state word, read by the kernel
    IngestParams p;
    (void)ingest_place(ws, p);
    const int passes = ingest_sort_passes(num_graphs);
    const int32_t *idx = (passes == 0 || num_edges < 2) ? nullptr : p.idx[passes & 1];
    GNNB_HIP_TRY(launch_edge_type_order((const long long *)edge_type_dev, idx, p.state, (int32_t *)ws->type_blob, num_edges, (hipStream_t)stream));
    *edge_type_ord_dev = (const int32_t *)ws->type_blob;
    return GNNB_OK;
}

int gnnb_forward_pyg_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                           const int64_t *edge_type_dev, const int64_t *batch_dev, const int64_t *ptr_dev, int num_graphs, int num_nodes,
                           int num_edges, float *out_dev, void *stream)
{
    if (!model || !ws)
        return fail(GNNB_ERR_INVALID, "null argument to gnnb_forward_pyg_types");
    if (!model->rgcn_relations || model->rgcn_relations != ws->rgcn_relations)
        return fail(GNNB_ERR_INVALID, "gnnb_forward_pyg_types takes a model of gnnb_rgcn_model_create and its workspace");
    const int32_t *coo = nullptr, *node_ptr = nullptr, *edge_ptr = nullptr, *edge_type = nullptr;
    if (const int rc = gnnb_ingest_pyg_types(ws, edge_index_dev, edge_type_dev, batch_dev, ptr_dev, num_graphs, num_nodes, num_edges, &coo, &node_ptr,
                                             &edge_ptr, &edge_type, stream))
        return rc;
    return forward_batched_types_tail(model, ws, x_dev, edge_type, coo, node_ptr, edge_ptr, num_graphs, num_nodes, num_edges, out_dev, stream, true);
}

} // extern "C"
