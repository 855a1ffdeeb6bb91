/*
 * gnnb_order.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): PyG mini-batches with oversized graphs,
 * ordered on the device.  gnnb_hip.h itself is unchanged by these entries.
 *
 * (new entry points at version 104: gnnb_model_desc, GNNB_VERSION, gnnb_ingest_bytes and the ingest allocation are unchanged.)
 * The large segment (gnnb_workspace_set_large_segment, gnnb_hip.h) needs the batch ordered so that the graphs beyond the
 * max_graph_nodes promise come LAST, and three host integers; gnnbuilder_amd.batching.order_large_last makes both on the host.  These entries make them on the device from
 * what gnnb_ingest_pyg leaves in the workspace (k_order.hip): a stable partition of the graphs -- a graph is LARGE when it has
 * more nodes than the workspace's max_graph_nodes promise as it stands at the call (promise 0: no graph is large) -- the rows
 * of x gathered into the new order, the edges moved and renumbered (the order inside a graph is kept), and perm [B], position ->
 * input graph.  Every array equals what order_large_last(from_pyg_batch(...), promise) returns, x_ord bit for bit.  The reference
 * has no counterpart (one graph per <name>_top call, model_tb.cpp.jinja:189-201; MAX_NODES is an array bound, never a path switch).
 *
 * The ONE synchronisation.  gnnb_ingest_pyg never synchronises; the ordered form does, once: the triple (first_graph,
 * first_node, first_edge) sizes the launches of the large segment, so it comes back through a host-mapped block of twelve
 * bytes after a wait on `stream` behind the last ordering kernel -- in place of the whole batch's round trip through the host.
 * For the same reason the ordered entries cannot be captured: while `stream` is being captured they return GNNB_ERR_INVALID
 * before anything is enqueued.  With nothing large the triple is (num_graphs, num_nodes, num_edges) and perm the identity.
 *
 * gnnb_workspace_enable_ordered_ingest enables the plain ingest if that has not been done, then makes ONE more device
 * allocation of gnnb_order_bytes(max_graphs, max_nodes, max_edges, in_dim, mlp_out) bytes -- x_ord, coo, the two ptr arrays,
 * perm, the per-graph shifts and the staged outputs of gnnb_forward_pyg_ordered; a pure function of its arguments, no GPU
 * needed -- plus the host-mapped triple; all owned by the workspace and freed with it, gnnb_workspace_bytes does not change.
 * Synchronous; call it outside stream capture, before the workspace is used (GNNB_ERR_INVALID once a batch has been prepared
 * on it; a second call is a no-op). */
#ifndef GNNB_ORDER_H
#define GNNB_ORDER_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t gnnb_order_bytes(int max_graphs, int max_nodes, int max_edges, int in_dim, int mlp_out);
int gnnb_workspace_enable_ordered_ingest(gnnb_workspace *ws);
/* gnnb_ingest_pyg, the ordering kernels and the wait, on `stream`.  x_dev: [num_nodes, in_dim] fp32 (any alignment).  batch_dev /
 * ptr_dev, capacity and argument errors as for gnnb_ingest_pyg; GNNB_ERR_INVALID without
 * gnnb_workspace_enable_ordered_ingest.  The five returned device pointers address the workspace's ordered allocation: valid
 * until the next ordered ingest on this workspace.  A batch the ingest flags (flag 128) stays CONTAINED here too: every
 * returned array is written, the ptr arrays are monotone from 0 to N / E, perm is a permutation, every coo entry lies in [0, N). */
int gnnb_ingest_pyg_ordered(gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                            const int64_t *batch_dev, const int64_t *ptr_dev,
                            int num_graphs, int num_nodes, int num_edges,
                            const float **x_ord_dev, const int32_t **coo_dev,
                            const int32_t **node_ptr_dev, const int32_t **edge_ptr_dev,
                            const int32_t **perm_dev,
                            int *first_graph, int *first_node, int *first_edge, void *stream);
/* gnnb_ingest_pyg_ordered, gnnb_workspace_set_large_segment(the triple) -- removed (first_graph = -1) when nothing is large, so
 * that such a batch runs exactly as gnnb_forward_pyg runs it -- gnnb_forward_batched on the ordered arrays into a staged matrix,
 * and the rows put back: out_dev [num_graphs, mlp_out], row g belongs to the CALLER's graph g.  The large-segment setting it
 * made is LEFT on the workspace, as if the caller had made it: a gnnb_forward_batched / gnnb_forward_pyg that follows on another
 * batch must set its own or remove it.  The stage entry points that follow see the ORDERED batch.  Lazy flag reporting as in
 * gnnb_forward_pyg: one report per call, in front of the ingest. */
int gnnb_forward_pyg_ordered(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev,
                             const int64_t *edge_index_dev, const int64_t *batch_dev, const int64_t *ptr_dev,
                             int num_graphs, int num_nodes, int num_edges, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_ORDER_H */
