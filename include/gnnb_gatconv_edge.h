/*
 * gnnb_gatconv_edge.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): GAT (v1) models with edge features,
 * end to end.  gnnb_hip.h, gnnb_order.h, gnnb_edge.h, gnnb_gat.h, gnnb_gat_edge.h, gnnb_gatconv.h and the other extensions are
 * unchanged by these entries (no new version: the library stays at 104).
 *
 * The model is GATv1EConv_GNNB (gnn-builder_amd/models.py, class _GATEConv): PyG's GATConv(in, out / heads, heads = H,
 * concat = True, negative_slope, add_self_loops = True, bias = True, edge_dim = d, fill_value = 'mean', dropout = 0,
 * residual = False),
 *   x' = lin(x) [N, H, C],  C = out / H                                           (lin has no bias)
 *   p_ij      = lin_edge(e_ij) [H, C]                                             lin_edge: Linear(d, H C, bias = False)
 *   s_ij[h]   = leaky_relu(att_src[h] . x'_j[h] + att_dst[h] . x'_i[h] + att_edge[h] . p_ij[h])          j in N(i) u {i}
 *   a_ij[h]   = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
 *   out_i[h]  = sum_j a_ij[h] x'_j[h, :] + bias              (the message is x'_j alone: the edge term enters the score only)
 * Self loops: explicit (v, v) rows of the input are removed together with their attribute rows (which are never read), one self
 * loop is added per node, and its attribute is e_ii = the mean of e_ji over the remaining in-edges of i (taken after the
 * removal), 0 for a node without in-edges.  The same edge_attr [E, d] goes to every layer; each layer has its own lin_edge and
 * att_edge.
 *
 * Such a model is an ordinary gnnb_model: its description is a GCN description (conv_type = GNNB_CONV_GCN), so graph prep drops
 * explicit (v, v) edges from the tables and the kernel adds the one self term itself; heads (1 .. 8), negative_slope and edge_dim
 * (1 .. 16) travel BESIDE it.  gnnb_model_gatconv_heads (gnnb_gatconv.h) reports its heads, gnnb_model_edge_dim (gnnb_edge.h) its
 * edge_dim; gnnb_model_gat_heads (gnnb_gat.h) stays 0 for it.
 *
 * What such a model runs: layer by layer (gnnb_workspace_last_path: GNNB_PATH_LAYERWISE, whatever the max_graph_nodes and
 * max_degree promises, which change no bit).  The edge term of the score is linear in the attribute,
 *   att_edge[h] . (W_e e)[h] = (A_edge W_e)[h, :] . e,
 * so att_edge is folded into lin_edge at upload, as att_src and att_dst are folded into lin: per layer ONE table a_edge [H, d]
 * (row h = sum_c att_edge[h, c] W_e[h C + c, :], summed in double with c increasing and rounded once).  A layer is the plain GAT
 * model's ONE GEMM, x -> [x' | s_src | s_dst | pad] [N, out + roundup4(2 heads)], unchanged, and ONE launch of
 * k_gat_edge_aggregate (csrc/k_gat_edge.hip: per edge and head d FMAs on the edge's attribute row, two adds and one leaky_relu in
 * front of an online softmax fused with the weighted sum, nothing per edge in HBM; bias, the middle layers' skip term and the
 * activation in its epilogue; plain fp32 in every math mode).  The self loop's edge term is the mean of the row's edge terms --
 * the term is linear, so this is the term of the mean attribute up to rounding.  No stack kernel, no fixed-point emulation (fpx_w
 * must be 0), no capture restrictions: nothing in the forward allocates, waits or reads back.
 *
 * It is run by the _edges entries of gnnb_edge.h: gnnb_forward_batched_edges, gnnb_forward_prepared_edges,
 * gnnb_forward_pyg_edges; gnnb_workspace_enable_edge_ingest accepts its workspace.  The entries without edge attributes
 * (gnnb_forward_batched, gnnb_forward_prepared, gnnb_forward_pyg, ...) refuse it with GNNB_ERR_INVALID and name the _edges entry;
 * gnnb_forward_pyg_ordered refuses it.  A model matches a workspace only if the kind, heads, negative_slope and edge_dim are all
 * equal: a GATv2 model with edge features and the same numbers is another kind.
 */
#ifndef GNNB_GATCONV_EDGE_H
#define GNNB_GATCONV_EDGE_H

#include "gnnb_gatconv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of such a model, in gnnb_gatconv_edge_model_create's order: per conv layer the four of
 * gnnb_gatconv_model_create (conv.lin.weight [out, in], conv.att_src [1, heads, out / heads], conv.att_dst likewise, conv.bias
 * [out]), then conv.att_edge [1, heads, out / heads] (= [out]), then conv.lin_edge.weight [out, edge_dim] (models.py _GATEConv;
 * GNNModel.canonical_param_names), then the head's as in gnnb_model_create: 6 per layer + 2 per head linear.  Negative: a
 * gnnb_status (GNNB_ERR_INVALID: what gnnb_gatconv_model_num_params refuses, or edge_dim outside 1 .. 16). */
int gnnb_gatconv_edge_model_num_params(const gnnb_model_desc *desc, int heads, int edge_dim);
/* gnnb_gatconv_model_create for such a model (models.py GNNModel with gnn_conv = GATv1EConv_GNNB).  Destroy with
 * gnnb_model_destroy, make its workspace with gnnb_workspace_create. */
int gnnb_gatconv_edge_model_create(const gnnb_model_desc *desc, int heads, float negative_slope, int edge_dim,
                                   const float *const *host_params, int num_params, gnnb_model **out_model);

/* Stage entry: one such layer behind its GEMM,
 *   out_i = act( sum_{j in N(i) u {i}} a_ij xl_j + bias + skip_i ),   a_ij[h] = softmax_j leaky_relu(ssrc_j[h] + sdst_i[h] + ae[h] . e_ij)
 * on the prepared batch of a GCN workspace (or a GAT / GATv2 model's, with or without edge features): the tables hold no (v, v)
 * edge and the kernel takes the self term itself, LAST, with the mean of the row's edge terms.  The operands of gnnb_aggregate_gat,
 * and edge_attr_dev [E, edge_dim] in COO row order (row e belongs to edge e of the batch's coo; NULL only for a batch without
 * edges), ae_dev: the folded table [heads, edge_dim] at row stride ldae >= edge_dim, edge_dim 1 .. 16.  16-byte accesses for
 * xl / skip / out as in gnnb_aggregate_gat; the attribute rows in 16-byte pieces when edge_dim % 4 == 0 and edge_attr_dev is
 * 16-byte aligned, scalar loads otherwise; ae_dev needs no alignment.  fp32 in every math mode.  A row without in-edges gives
 * act(xl_i + bias + skip_i), bit for bit.  GNNB_ERR_INVALID (nothing launched): what gnnb_aggregate_gat refuses, edge_dim out of
 * range, ldae < edge_dim, a NULL ae_dev, a NULL edge_attr_dev for a batch with edges.
 * Summation order -- fixed by the batch and by the form (16-byte or scalar), never by the grid, by which workgroup took a row or
 * by how many lanes share it; a repeat launch gives the same bits, and an H-head launch gives the bits of H one-head launches on
 * the column slices and the rows of ae.  Per (edge, head): t = fma(ae[h][d - 1], e[d - 1], ... fma(ae[h][0], e[0], 0));
 * z = (ssrc_j[h] + sdst_i[h]) + t; s = z > 0 ? z : z * negative_slope.  Per (row, head): the state (m, l, acc) starts from
 * (-inf, 0, 0) and tsum from 0; the in-edges in CSR slot order in batches of 4: m' = max(m, s_0 .. s_3),
 * l = l exp(m - m') + (((e_0 + e_1) + e_2) + e_3), acc = acc exp(m - m') + e_0 x_0 + .. + e_3 x_3 with e_r = exp(s_r - m'), and
 * tsum = (((tsum + t_0) + t_1) + t_2) + t_3 in slot order; a row of more than 64 in-edges in pieces of 64 slots, each from
 * (-inf, 0, 0) and 0, merged -- tsum added -- in piece order; then the self term, last, with t_ii = tsum / in-degree (0 at
 * in-degree 0): one more step of the same recurrence; out = act((acc / (l + 1e-16) + bias) + skip).  exp is the hardware's exp2 of
 * the argument scaled by log2(e). */
int gnnb_aggregate_gat_edges(gnnb_workspace *ws, const float *xl_dev, int ldl, const float *ssrc_dev /*[N, heads]*/, int lds,
                             const float *sdst_dev /*[N, heads]*/, int ldd, const float *bias_dev /*[width] or NULL*/,
                             const float *skip_dev /*[N, width] or NULL*/, int act /*gnnb_act*/, int heads, float negative_slope,
                             const float *edge_attr_dev /*[E, edge_dim], COO row order*/, int edge_dim,
                             const float *ae_dev /*[heads, edge_dim]*/, int ldae, float *out_dev /*[N, width]*/, int width, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_GATCONV_EDGE_H */
