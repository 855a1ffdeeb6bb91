/*
 * gnnb_rgcn.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): relational GCN models (Schlichtkrull et al.)
 * on graphs whose edges carry an INTEGER type -- a molecule's bonds as single / double / triple / aromatic --, end to end.  Every
 * other header is unchanged by these entries (no new version: the library stays at 104).
 *
 * Reference: none in gnnbuilder.  The model is RGCNConv_GNNB (gnn-builder_amd/models.py, class _RGCNConv): PyG's
 * RGCNConv(in, out, num_relations = R, aggr = 'mean', root_weight = True, bias = True) without basis or block decomposition,
 *   out_i = x_i @ root + bias + sum_{r < R} (1 / |N_r(i)|) * sum_{j in N_r(i)} x_j @ weight[r]
 * N_r(i) = the in-edges of i with type r: duplicate edges count as often as they occur, an explicit (v, v) edge is an ordinary
 * edge; no self loop is added and none is removed; a relation without an edge into i contributes 0.  weight [R, in, out] and
 * root [in, out] are applied as x @ W (NOT nn.Linear's [out, in] layout), bias [out].  It is also the typed message function of
 * the GGNN paper that gnnb_ggnn.h lists as out of scope.
 *
 * Such a model is an ordinary gnnb_model: its description is a GIN description (conv_type = GNNB_CONV_GIN, gin_eps ignored, every
 * other field as for GIN; fpx_w must be 0) with `relations` BESIDE it -- the tables of a GIN workspace keep explicit (v, v) edges,
 * those of a GCN workspace drop them (gnnb_hip.h, "Explicit self loops").  gnnb_model_rgcn_relations reports the relations; the
 * other families' queries are 0 for such a model.  A model matches a workspace only if both have the same relations.
 *
 * The fold.  The message is linear, so the per-relation transform moves into the layer's GEMM.  At upload
 *   w_rgcn = [weight[0]^T ; .. ; weight[R-1]^T ; root^T]     [(R + 1) out, in], pure transposes, no arithmetic
 *   b_rgcn = [0 | .. | 0 | bias]                             the relation blocks take NO bias: it would be counted once per edge
 * A layer is ONE GEMM x -> [p_0 | .. | p_{R-1} | root] [N, (R + 1) out] in the model's math mode and ONE launch of
 * k_rgcn_aggregate (csrc/k_rgcn.hip; plain fp32 in every math mode), which gathers ONE row-width per edge -- the traffic of a plain
 * sum: the column block is the edge's relation, the weight the per-(row, relation) mean weight -- with the root term, the middle
 * layers' skip term and the activation in its epilogue.  Which block and which weight is the slot record {rel, w} (8 bytes) of the
 * edge's CSR slot, written once per forward for all layers by k_rgcn_slots: rel = edge_type of the slot's edge,
 * w = 1.0f / (float)|N_rel(i)|, the count an integer (exact, whatever the order) and the division the correctly rounded one.
 *
 * Edge types.  int32 [E] in COO row order at the _types forwards (int64 in the input's order at the PyG entries, which permute and
 * narrow them on the device).  A type outside [0, relations) -- at the PyG entries also one that does not fit an int32 -- sets the
 * workspace's flag 256 and is reported as GNNB_ERR_GRAPH, once, by gnnb_workspace_check or lazily by the next entry call, like
 * every malformed batch.  Such an edge's record is {0, 0.0f}: it adds nothing to its row and takes no part in any count; no
 * address is ever formed from an unchecked type.  The results of a flagged forward are unspecified but finite for finite inputs.
 *
 * Summation order of the aggregate -- fixed by the batch and by the form (16-byte or scalar), never by the grid or by which
 * workgroup took a row; a repeat launch gives the same bits.  Per (row, column): the in-edges in CSR slot order in batches of 4,
 *   acc = fma(w_3, p_3, fma(w_2, p_2, fma(w_1, p_1, fma(w_0, p_0, acc))))
 * slots past the row's end taking no part; a row of more than 64 in-edges in pieces of 64 slots, each summed from 0, the pieces
 * added in piece order onto 0; then out = act((acc + root_ic) + skip_ic), an absent root or skip adding nothing, not + 0.
 *
 * What such a model runs: layer by layer (gnnb_workspace_last_path: GNNB_PATH_LAYERWISE), whatever the promises.  It needs the
 * batch's edge types, so only the _types entries below run it: every whole-model entry of gnnb_hip.h, gnnb_order.h and gnnb_edge.h
 * refuses it with GNNB_ERR_INVALID before anything is enqueued and names the _types entry; the _types entries refuse every other
 * model.  The slot records are built inside the forward into an allocation of 8 max_edges bytes that only such a model's workspace
 * has; graph prep takes no types and is unchanged.  Nothing in the forward allocates, waits or reads back: it can be captured.
 *
 * Out of scope: num_bases, num_blocks, aggr other than mean, root_weight = False and bias = False at model level (the stage
 * entry's root = NULL covers the kernel side), more than 8 relations, widths above 256, per-layer edge types, the ordered ingest,
 * the host-array forward, Project (code generation), the fixed-point emulation, and the aggregate-first order for narrow first
 * layers (aggregate per relation at the input width, then one GEMM with K = (R + 1) in).
 */
#ifndef GNNB_RGCN_H
#define GNNB_RGCN_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of an RGCNConv model of `relations` relations, in gnnb_rgcn_model_create's order: per conv layer conv.weight
 * [relations, in, out], conv.root [in, out], conv.bias [out] (models.py _RGCNConv; GNNModel.canonical_param_names), then the
 * head's as in gnnb_model_create: 3 per layer + 2 per head linear.  Negative: a gnnb_status (GNNB_ERR_INVALID: relations outside
 * 1 .. 8, a layer output width above 256, conv_type != GNNB_CONV_GIN, fpx_w != 0, or a description gnnb_model_num_params refuses). */
int gnnb_rgcn_model_num_params(const gnnb_model_desc *desc, int relations);
/* gnnb_model_create for such a model (models.py GNNModel with gnn_conv = RGCNConv_GNNB, gnn_relations = relations).  Destroy with
 * gnnb_model_destroy, make its workspace with gnnb_workspace_create. */
int gnnb_rgcn_model_create(const gnnb_model_desc *desc, int relations, const float *const *host_params, int num_params, gnnb_model **out_model);
/* relations of a model of gnnb_rgcn_model_create; 0 for every other model (and for NULL) */
int gnnb_model_rgcn_relations(const gnnb_model *model);

/* gnnb_forward_batched for such a model: graph prep, the slot records, the forward.  edge_type_dev: int32 [num_edges] in COO row
 * order (row e is the type of coo row e); NULL only with num_edges == 0.  Everything else as gnnb_forward_batched_edges
 * (gnnb_edge.h).  GNNB_ERR_INVALID for a model that is not of gnnb_rgcn_model_create or a workspace of another model. */
int gnnb_forward_batched_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev,
                               const int32_t *edge_type_dev /*int32 [E], COO row order; NULL when E == 0*/, const int32_t *coo_dev,
                               const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                               float *out_dev, void *stream);
/* gnnb_forward_prepared for such a model on the workspace's prepared batch (gnnb_graph_prep, which takes no types): the slot
 * records from edge_type_dev (as above, for the prepared batch's edges), then the forward. */
int gnnb_forward_prepared_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int32_t *edge_type_dev, float *out_dev,
                                void *stream);

/* Size of the allocation gnnb_workspace_enable_type_ingest makes for a workspace of max_edges edges (the types in COO row order);
 * 0 for a negative argument.  Host arithmetic. */
size_t gnnb_type_ingest_bytes(int max_edges);
/* The contract of gnnb_workspace_enable_edge_ingest (gnnb_edge.h) for such a model's workspace: enables the base ingest too, once,
 * right after gnnb_workspace_create.  GNNB_ERR_INVALID for a workspace of a model without relations. */
int gnnb_workspace_enable_type_ingest(gnnb_workspace *ws);
/* gnnb_ingest_pyg_edges with edge types in place of attribute rows: edge_type_dev int64 [num_edges] in the order of edge_index's
 * columns; *edge_type_ord_dev = (int32) the type of the input edge of every coo row, in the workspace (valid until the next
 * ingest); a value that does not fit the int32 is written as -1 (and flagged by the forward's slot pass).  Which path the ingest
 * took is read on the device: nothing is read back, the call can be captured. */
int gnnb_ingest_pyg_types(gnnb_workspace *ws, const int64_t *edge_index_dev, const int64_t *edge_type_dev /*int64 [E]*/, const int64_t *batch_dev,
                          const int64_t *ptr_dev, int num_graphs, int num_nodes, int num_edges, const int32_t **coo_dev,
                          const int32_t **node_ptr_dev, const int32_t **edge_ptr_dev, const int32_t **edge_type_ord_dev, void *stream);
/* gnnb_ingest_pyg_types, then gnnb_forward_batched_types on its outputs: the contract of gnnb_forward_pyg_edges. */
int gnnb_forward_pyg_types(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int64_t *edge_index_dev,
                           const int64_t *edge_type_dev, const int64_t *batch_dev, const int64_t *ptr_dev, int num_graphs, int num_nodes,
                           int num_edges, float *out_dev, void *stream);

/* Stage entries, on the prepared batch of any workspace whose tables keep explicit self loops (a GIN, GINE, GraphSAGE, PNA,
 * TransformerConv, ResGatedGraphConv, GatedGraphConv or RGCNConv model's); a workspace of a GCN description (a GCN, GATv2 or GAT
 * model's) is refused (GNNB_ERR_INVALID: its tables have dropped the (v, v) edges).
 *
 * gnnb_rgcn_slots: slot_rec_dev[s] = {int32 rel, float w} (8 bytes, 8-byte aligned, num_edges records of the caller's) for every
 * CSR slot s of the prepared batch, from edge_type_dev (int32 [E], COO row order) as described above; a type outside
 * [0, relations) sets flag 256 and gives {0, 0.0f}.  Slots that no row owns are not written.  relations 1 .. 8. */
int gnnb_rgcn_slots(gnnb_workspace *ws, const int32_t *edge_type_dev, int relations, void *slot_rec_dev /*caller's [E] records*/, void *stream);
/* gnnb_aggregate_rgcn: out [N, width] = act((sum over row i's slots s of w_s * p[col_s, rel_s * width + c] + root_ic) + skip_ic) in
 * the summation order above.  p_dev: rows of stride ldp >= relations * width, block r the relation's transformed features;
 * root_dev: rows of stride ldr >= width, or NULL (ldr ignored) -- the blocks of one [N, (relations + 1) width] GEMM output are
 * fine; skip_dev [N, width] or NULL; act a gnnb_act; width 1 .. 256; out_dev must not alias an input.  A record's relation is
 * clamped into [0, relations) before use.  16-byte accesses when width % 4 == 0 and p / root / skip / out and the strides are
 * 16-byte aligned, scalar accesses otherwise.  fp32 in every math mode. */
int gnnb_aggregate_rgcn(gnnb_workspace *ws, const void *slot_rec_dev, const float *p_dev, int ldp, int relations,
                        const float *root_dev /*or NULL*/, int ldr, const float *skip_dev /*[N, width] or NULL*/, int act /*gnnb_act*/,
                        float *out_dev /*[N, width]*/, int width, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_RGCN_H */
