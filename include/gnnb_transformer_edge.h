/*
 * gnnb_transformer_edge.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): TransformerConv models with edge
 * features (the Graph Transformer layer as PyG users build it on molecular graphs: TransformerConv(..., edge_dim = d)), end to
 * end.  gnnb_hip.h, gnnb_order.h, gnnb_edge.h, gnnb_pna_edge.h, gnnb_gat.h, gnnb_gat_edge.h and gnnb_transformer.h are unchanged
 * by these entries (no new version: the library stays at 104).
 *
 * Reference: none in gnnbuilder.  The model is TransformerEConv_GNNB (gnn-builder_amd/models.py, class _TransformerEConv): PyG's
 * TransformerConv(in, out / heads, heads = H, concat = True, beta = False, dropout = 0, edge_dim = d, bias = True,
 * root_weight = True),
 *   q, k, v [N, H, C], r = lin_skip(x) [N, H C]                                as in gnnb_transformer.h, C = out / H
 *   p_ij      = lin_edge(e_ij) [H, C]                                          lin_edge: Linear(d, H C, bias = False)
 *   s_ij[h]   = (q_i[h, :] . (k_j[h, :] + p_ij[h, :])) / sqrt(C)               j in N(i) -- the input's edges as they are
 *   a_ij[h]   = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
 *   out_i     = concat_h( sum_j a_ij[h] (v_j[h, :] + p_ij[h, :]) ) + r_i
 * Self loops: none is added and none is removed.  An explicit (v, v) edge of the input is an ordinary edge and its attribute row
 * an ordinary attribute row; a node without in-edges gets the root term r_i alone.  The same edge_attr [E, d] goes to every
 * layer; each layer has its own lin_edge.
 *
 * What is computed.  Dot-product attention is linear in the key and in the value, so the edge term leaves the per-edge work:
 *   q_i[h] . (k_j[h] + W_e[h] e_ij)   = q_i[h] . k_j[h] + qe_i[h] . e_ij          qe_i[h] = W_e[h]^T q_i[h]  in R^d
 *   sum_j a_ij (v_j[h] + W_e[h] e_ij) = sum_j a_ij v_j[h] + W_e[h] (sum_j a_ij e_ij)
 * Per (edge, head) the edge term costs d FMAs in the score and d FMAs in a second, d-wide accumulator; W_e is applied once per
 * (row, head).  The [E, out] projected term exists nowhere.  qe is itself linear in x: H d more columns of the layer's one GEMM,
 * with the weights W_e[h]^T W_q[h] and the bias W_e[h]^T b_q[h] formed on the host at model creation (accumulated in double over
 * the head's columns in increasing order, rounded once).
 *
 * Such a model is an ordinary gnnb_model: its description is a GIN description (conv_type = GNNB_CONV_GIN, gin_eps ignored), so
 * the tables keep explicit (v, v) edges; heads (1 .. 8) and edge_dim (1 .. 16) travel BESIDE it.  gnnb_model_transformer_heads
 * and gnnb_model_edge_dim report them; gnnb_model_gat_heads is 0.
 *
 * What such a model runs: layer by layer (GNNB_PATH_LAYERWISE whatever the promises, which change no bit).  A layer is ONE GEMM,
 * x -> [q | k | v | r | qe] [N, 4 out + roundup4(H d)] in the model's math mode, and ONE launch of k_transformer_edge_aggregate
 * (csrc/k_transformer_edge.hip; plain fp32 in every math mode).  Nothing in the forward allocates, waits or reads back: it can be
 * captured.  The entries with edge attributes of gnnb_edge.h run it -- gnnb_forward_batched_edges, gnnb_forward_prepared_edges,
 * gnnb_workspace_enable_edge_ingest, gnnb_ingest_pyg_edges, gnnb_forward_pyg_edges --; the entries without edge attributes refuse
 * it and name the _edges entry; gnnb_forward_pyg_ordered refuses it.  A model matches a workspace only if both are of this kind
 * with equal heads and edge_dim.
 *
 * Out of scope: beta = True, concat = False, root_weight = False at model level (the stage entry's root = NULL covers the kernel
 * side), dropout.
 */
#ifndef GNNB_TRANSFORMER_EDGE_H
#define GNNB_TRANSFORMER_EDGE_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of such a model, in gnnb_transformer_edge_model_create's order: per conv layer gnnb_transformer.h's eight
 * (conv.lin_key.weight [out, in], .bias, conv.lin_query.*, conv.lin_value.*, conv.lin_skip.*), then conv.lin_edge.weight
 * [out, edge_dim] (no bias), then the head's as in gnnb_model_create: 9 per layer + 2 per head linear.  Negative: a gnnb_status
 * (GNNB_ERR_INVALID: what gnnb_transformer_model_num_params refuses, or edge_dim outside 1 .. 16). */
int gnnb_transformer_edge_model_num_params(const gnnb_model_desc *desc, int heads, int edge_dim);
/* gnnb_model_create for such a model (models.py GNNModel with gnn_conv = TransformerEConv_GNNB).  Destroy with
 * gnnb_model_destroy, make its workspace with gnnb_workspace_create. */
int gnnb_transformer_edge_model_create(const gnnb_model_desc *desc, int heads, int edge_dim, const float *const *host_params,
                                       int num_params, gnnb_model **out_model);

/* Stage entry: one such layer behind its GEMM,
 *   out_i[h, c] = act( ((acc_c + sum_d we[h C + c][d] * aacc[d]) / (l + 1e-16) + root) + skip )
 *   s_ij[h]     = (q_i[h] . k_j[h] + sum_d qe_i[h * edge_dim + d] * e_ij[d]) * scale
 * with (l, acc, aacc) the softmax sums of 1, v_j[h, c] and e_ij[d] over the row's in-edges, on the prepared batch of any workspace
 * whose tables keep explicit self loops; a GCN, GATv2 or GATv2-with-edges workspace is refused (GNNB_ERR_INVALID: its tables
 * have dropped the (v, v) edges).  qe_dev and we_dev are separate operands on purpose: the entry computes what it is given (the
 * layer passes qe = W_e^T q as columns of its GEMM output and lin_edge's raw weight), so the score term and the value term can be
 * exercised apart.  q / k / v / root / skip / act / heads / scale / out / width as in gnnb_aggregate_transformer; qe_dev: rows of
 * heads * edge_dim floats at row stride ldqe >= heads * edge_dim; edge_attr_dev [E, edge_dim] in COO row order (NULL only for a
 * batch without edges); edge_dim 1 .. 16; we_dev [width, edge_dim] rows at stride ldwe >= edge_dim.  16-byte accesses of the rows
 * when (width / heads) % 4 == 0 and q / k / v / root / skip / out and their strides are 16-byte aligned; of edge_attr and qe each
 * when edge_dim % 4 == 0 and the operand (and qe's stride) is 16-byte aligned; scalar accesses otherwise -- the values do not
 * depend on the latter two (we is staged in LDS once per workgroup, any alignment).  A row without in-edges gives act(root_i + skip_i), bit for bit.  With all-zero edge_attr the
 * values are gnnb_aggregate_transformer's.  GNNB_ERR_INVALID (nothing launched): what gnnb_aggregate_transformer refuses, edge_dim
 * out of range, ldqe < heads * edge_dim, ldwe < edge_dim, NULL qe_dev or we_dev, NULL edge_attr_dev for a batch with edges.
 * Summation order -- fixed by the batch and by the form (16-byte or scalar rows), never by the grid or by which workgroup took a
 * row; a repeat launch gives the same bits.  Per (row, head): a score's products per lane over its columns (fma, column
 * increasing), the lanes' partials in a butterfly, then the edge dot onto that sum, fma(qe[d], e[d], .) with d increasing, then
 * the sum times scale (dot, then edge dot, then scale); the state (m, l, acc, aacc) starts at (-inf, 0, 0, 0); the in-edges in CSR
 * slot order in batches of 4: m' = max(m, s_0 .. s_3), l = l exp(m - m') + (((e_0 + e_1) + e_2) + e_3), acc = acc exp(m - m') +
 * e_0 v_0 + .. + e_3 v_3 with e_r = exp(s_r - m'), aacc by the same rule on the attribute rows; a row of more than 64 in-edges in
 * pieces of 64 slots, each from the empty state, merged in piece order; then t = acc_c, t = fma(we[h C + c][d], aacc[d], t) with d
 * increasing, out = act((t / (l + 1e-16) + root) + skip).  exp is the hardware's exp2 of the argument scaled by log2(e). */
int gnnb_aggregate_transformer_edges(gnnb_workspace *ws, const float *q_dev, int ldq, const float *k_dev, int ldk,
                                     const float *v_dev, int ldv, const float *qe_dev /*[N, heads * edge_dim] rows at ldqe*/,
                                     int ldqe, const float *root_dev /*[N, width] rows at ldr, or NULL*/, int ldr,
                                     const float *skip_dev /*[N, width] or NULL*/, int act /*gnnb_act*/, int heads, float scale,
                                     const float *edge_attr_dev /*[E, edge_dim], COO row order; NULL only without edges*/,
                                     int edge_dim, const float *we_dev /*[width, edge_dim] rows at ldwe*/, int ldwe,
                                     float *out_dev /*[N, width]*/, int width, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_TRANSFORMER_EDGE_H */
