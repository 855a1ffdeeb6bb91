/*
 * gnnb_edge.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): GINE models, i.e. GIN with edge
 * features, end to end.  gnnb_hip.h and gnnb_order.h themselves are unchanged by these entries.
 *
 * (new entry points at version 104: gnnb_model_desc, GNNB_VERSION, gnnb_ingest_bytes and the ingest allocation are unchanged.)
 * Reference: GINEConv_GNNB (gnnbuilder/models.py:97-123) and its native gine_conv (gnn_builder_lib.h:1555-1742):
 *   h_i' = nn((1 + eps) h_i + sum_{j->i} relu(h_j + W_e e_ij + b_e)),   nn = Linear -> ReLU -> Linear (hidden = out width).
 * The reference's emitter does not stack it (model.cpp.jinja:143-144 is a TODO); here a GINE model is an ordinary gnnb_model
 * that carries edge weights: its description is a GIN description (conv_type = GNNB_CONV_GIN, every other field as for GIN)
 * and edge_dim -- the width of an edge-attribute row, 1 .. 16 -- travels BESIDE it.  The same [E, edge_dim] edge attributes
 * go to every layer, each layer projects them with its own W_e [layer input width, edge_dim] and b_e.
 *
 * What such a model runs: layer by layer (gnnb_workspace_last_path: GNNB_PATH_LAYERWISE, whatever the max_graph_nodes
 * promise) -- k_gine_aggregate (csrc/k_gine.hip: the projection W_e e + b_e formed inside the aggregate, never in HBM; plain
 * fp32 in every math mode), then the two GEMMs of GIN with skip and activation in the second one's epilogue (desc.math applies
 * to them), pooling, the readout, the output activation.  No fixed-point emulation (fpx_w must be 0).
 *
 * The entries of gnnb_hip.h / gnnb_order.h that run a whole model (gnnb_forward_batched, gnnb_forward_prepared,
 * gnnb_forward_prepared_prep_next, gnnb_forward_batched_host, gnnb_forward_pyg, gnnb_forward_pyg_ordered,
 * gnnb_gcn_stack_timed) return GNNB_ERR_INVALID before anything is enqueued when given such a model or its workspace (the
 * message names the _edges entry); the _edges entries return GNNB_ERR_INVALID for a model without edge weights.
 * gnnb_workspace_set_max_graph_nodes / _set_max_degree / _set_large_segment, gnnb_graph_prep, gnnb_workspace_check and the
 * stage entry points work on such a workspace as on any other.
 *
 * A PNA model with edge features (gnnb_pna_edge.h: gnnb_pna_edge_model_create, a PNA description with edge_dim beside it) is the
 * other kind of model with edge weights: the forwards and the ingest entries below run it as they run a GINE model ("a model of
 * gnnb_edge_model_create" below reads "... or of gnnb_pna_edge_model_create"), gnnb_model_edge_dim reports its edge_dim, and the
 * entries that refuse a GINE model refuse it in the same way.
 */
#ifndef GNNB_EDGE_H
#define GNNB_EDGE_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of a GINE model, in gnnb_edge_model_create's order: per conv layer the four of GIN (mlp.linear_0.weight
 * [out, in], .bias, mlp.linear_1.weight [out, out], .bias) then conv.lin.weight [in, edge_dim] and conv.lin.bias [in]
 * (models.py:97-123; canonical_param_names), then the head's as in gnnb_model_create: 6 per layer + 2 per head linear.
 * Negative: a gnnb_status (GNNB_ERR_INVALID: edge_dim outside 1 .. 16, conv_type != GNNB_CONV_GIN, fpx_w != 0, or a
 * description gnnb_model_num_params refuses). */
int gnnb_edge_model_num_params(const gnnb_model_desc *desc, int edge_dim);
/* gnnb_model_create (load_parameters, model.cpp.jinja:724-730) for a GINE model; destroy with gnnb_model_destroy, make its
 * workspace with gnnb_workspace_create. */
int gnnb_edge_model_create(const gnnb_model_desc *desc, int edge_dim, const float *const *host_params, int num_params,
                           gnnb_model **out_model);
/* edge_dim of a model of gnnb_edge_model_create; 0: a model of gnnb_model_create (or NULL) */
int gnnb_model_edge_dim(const gnnb_model *model);

/* gnnb_forward_batched (the reference's <name>_top per graph, model_tb.cpp.jinja:189-201) with edge attributes:
 * edge_attr_dev [num_edges, edge_dim] fp32, row i belongs to coo row i (the reference's edge_attr input of gine_conv,
 * gnn_builder_lib.h:1640-1742).  num_edges = 0 is legal and edge_attr_dev may then be NULL. */
int gnnb_forward_batched_edges(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev,
                               const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev,
                               int num_graphs, int num_nodes, int num_edges, float *out_dev, void *stream);
/* gnnb_forward_prepared on the batch gnnb_graph_prep left in the workspace; edge_attr_dev in that batch's COO row order */
int gnnb_forward_prepared_edges(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev,
                                float *out_dev, void *stream);

/* Stage entry: GINE's aggregate with the projection inside (gine_conv_agg + the self term of gine_conv,
 * gnn_builder_lib.h:1555-1742; gnnb_aggregate_edges is the form that reads a projected [E, width] matrix):
 *   out_i = (1 + eps) x_i + sum_{j->i} relu(x_j + W_e e_ij + b_e)
 * on the prepared batch.  x_dev / out_dev [N, width] (any width >= 1; 16-byte accesses when width % 4 == 0 and both are
 * 16-byte aligned), edge_attr_dev [E, edge_dim] in COO row order (NULL when the batch has no edge), we_dev [width, ldwe]
 * with ldwe >= edge_dim, be_dev [width].  fp32 in every math mode.  Summation order (fixed, independent of the launch):
 * the projection's terms by increasing attribute index on top of b_e; a row's in-edges in CSR slot order in pieces of 64,
 * the pieces' sums added in order; the self term last. */
int gnnb_aggregate_edges_fused(gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev, int edge_dim,
                               const float *we_dev, int ldwe, const float *be_dev, float *out_dev, int width, float eps,
                               void *stream);

/* ------------------------------------------------------------------ PyG mini-batches with edge attributes
 * torch_geometric's Batch holds edge_attr [E, edge_dim] in edge_index's column order; gnnb_ingest_pyg (gnnb_hip.h) groups the
 * edges by graph with a stable sort when they are not grouped already, and the attribute rows have to follow their edges.
 * The reference has no counterpart (one graph per <name>_top call, model_tb.cpp.jinja:189-201).
 * gnnb_ingest_pyg_edges runs gnnb_ingest_pyg and ONE more kernel: edge_attr_ord[i] = edge_attr[the input edge of coo row i].
 * Which of the ingest's two paths ran is read on the device: no read-back, no synchronisation, the same launches for
 * grouped and shuffled input -- capturable as gnnb_forward_pyg is.  A batch the ingest flags (flag 128) stays contained:
 * every row of edge_attr_ord is a row of edge_attr.
 *
 * gnnb_workspace_enable_edge_ingest enables the plain ingest if that has not been done, then makes ONE more device
 * allocation of gnnb_edge_ingest_bytes(max_edges, edge_dim) bytes for edge_attr_ord (a pure function of its arguments, no
 * GPU needed; 0 for arguments out of range), owned by the workspace and freed with it; gnnb_ingest_bytes, the ingest
 * allocation and gnnb_workspace_bytes do not change.  The workspace must belong to a model of gnnb_edge_model_create.
 * Synchronous; call it outside stream capture, before the workspace is used (GNNB_ERR_INVALID once a batch has been
 * prepared on it; a second call is a no-op). */
size_t gnnb_edge_ingest_bytes(int max_edges, int edge_dim);
int gnnb_workspace_enable_edge_ingest(gnnb_workspace *ws);
/* edge_attr_dev [num_edges, edge_dim] fp32 (NULL when num_edges == 0); everything else as gnnb_ingest_pyg.  The four
 * returned device pointers address the workspace's allocations: valid until the next ingest on this workspace. */
int gnnb_ingest_pyg_edges(gnnb_workspace *ws, const int64_t *edge_index_dev, const float *edge_attr_dev,
                          const int64_t *batch_dev, const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges,
                          const int32_t **coo_dev, const int32_t **node_ptr_dev, const int32_t **edge_ptr_dev,
                          const float **edge_attr_ord_dev, void *stream);
/* gnnb_ingest_pyg_edges + gnnb_forward_batched_edges on `stream` (gnnb_forward_pyg for a GINE model); lazy flag reporting
 * as there: one report per call, in front of the ingest. */
int gnnb_forward_pyg_edges(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                           const float *edge_attr_dev, const int64_t *batch_dev, const int64_t *ptr_dev,
                           int num_graphs, int num_nodes, int num_edges, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_EDGE_H */
