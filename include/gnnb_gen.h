/*
 * gnnb_gen.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): GENConv models -- the layer of DeeperGCN (Li et
 * al.), whose aggregate is a per-column softmax-weighted sum of the messages themselves --, end to end, with or without edge features.
 * Every other header is unchanged by these entries (no new version: the library stays at 104).
 *
 * Reference: none in gnnbuilder.  The model is GENConv_GNNB / GENEConv_GNNB (gnn-builder_amd/models.py, class _GENConv).  For a layer
 * in -> out, edge attributes e_ij of edge_dim d (d = 0: none), temperature t (any real, one per layer) and eps_m = 1e-7:
 *   s = lin_src(x) if in != out else x,   r = lin_dst(x) if in != out else x                              [N, out]
 *   m_ij[c] = relu(s_j[c] + p_ij[c]) + eps_m,   p_ij = lin_edge(e_ij) = W_e e_ij + b_e   (d = 0: p = 0)
 *   a_ij[c] = exp(t m_ij[c]) / sum_{k -> i} exp(t m_ik[c])          -- softmax over i's in-edges, PER COLUMN
 *   agg_i[c] = sum_{j -> i} a_ij[c] m_ij[c]                         (a row without in-edges: 0)
 *   out_i = mlp(agg_i + r_i),   mlp = Linear(out, 2 out) -> ReLU -> Linear(2 out, out)
 * No self loop is added or removed, duplicate edges count as often as they occur, an explicit (v, v) edge is an ordinary edge.
 * t = 0 is the mean of the messages, a large t approaches their max, a negative t their min.  PyG's + 1e-16 in the softmax
 * denominator is dropped: behind the max shift the denominator is >= 1.  Every linear carries a bias (PyG's bias = False model is this
 * one with zero biases).  This FORMULA is what is pinned; the parameter names follow PyG's as far as they are remembered.
 *
 * Such a model is an ordinary gnnb_model: its description is a GIN description (conv_type = GNNB_CONV_GIN, gin_eps ignored, every
 * other field as for GIN; fpx_w must be 0; every layer width at most 256) with edge_dim (0 .. 16) and the per-layer temperatures
 * BESIDE it.  gnnb_model_gen reports 1, gnnb_model_edge_dim reports d; the other families' queries are 0.  A model matches a
 * workspace only of the same kind and edge_dim.
 *
 * A layer with in != out is ONE GEMM x -> [s | r] [N, 2 out] on [lin_src.weight ; lin_dst.weight] with the stacked bias, ONE launch
 * of k_gen_aggregate (csrc/k_gen.hip; plain fp32 in every math mode) on the two column blocks, and the MLP's two GEMMs with the
 * model's skip term and activation in the second's epilogue.  A layer with in == out (every middle layer) has no first GEMM:
 * s = r = x.  The temperature is read at upload and passed by value at every launch.
 *
 * Summation order of the aggregate -- fixed by the batch and by the form (16-byte or scalar), never by the grid or by occupancy: per
 * (row, column) the in-edges in CSR slot order; p = fma(W_e[c][d-1], e[d-1], .. fma(W_e[c][0], e[0], b_e[c])); m = fmaxf(s_j + p, 0)
 * + eps_m; z = t m; onto the state (M, S, W) = (-inf, 0, 0): with dz = z - M, f = exp(-|dz|) -- dz > 0: S = fma(S, f, 1),
 * W = fma(W, f, m), M = z; else S = S + f, W = fma(f, m, W).  A row of more than 64 in-edges in pieces of 64 slots, each from the
 * empty state, merged in piece order onto the empty state: M' = max(M, M_p), S = fma(S_p, exp(M_p - M'), S exp(M - M')), W likewise.
 * out = (S > 0 ? W / S : 0) + r.  exp(x) is the hardware's exp2 of x log2(e).
 *
 * What such a model runs: layer by layer (GNNB_PATH_LAYERWISE), whatever the promises.  edge_dim = 0: the ordinary forwards
 * (gnnb_forward_batched, gnnb_forward_prepared, gnnb_forward_pyg, gnnb_forward_batched_host, gnnb_forward_prepared_prep_next);
 * edge_dim >= 1: the _edges entries of gnnb_edge.h (gnnb_forward_batched_edges, gnnb_forward_prepared_edges,
 * gnnb_workspace_enable_edge_ingest, gnnb_ingest_pyg_edges, gnnb_forward_pyg_edges) with ONE edge_attr [E, d] for every layer.  Every
 * other whole-model entry -- the wrong one of plain / _edges, gnnb_forward_pyg_ordered -- refuses it with GNNB_ERR_INVALID and names
 * the right one.  Nothing in the forward allocates, waits or reads back: it can be captured.
 *
 * Out of scope: aggr = "powermean" and learn_p, msg_norm, a norm layer inside the MLP (an eval-mode BatchNorm is an affine map the
 * user can fold into mlp.0), num_layers != 2 or expansion != 2, edge_dim above 16, widths above 256, per-layer edge attributes, the
 * LDS-resident stack kernels and every fused rung, the ordered ingest, Project (code generation), the templates and tb_data, the
 * fixed-point emulation, bench.py workloads.
 */
#ifndef GNNB_GEN_H
#define GNNB_GEN_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of a GENConv model, in gnnb_gen_model_create's order: per conv layer (in != out only: conv.lin_src.weight
 * [out, in], conv.lin_src.bias [out], conv.lin_dst.weight [out, in], conv.lin_dst.bias [out],) (edge_dim > 0 only:
 * conv.lin_edge.weight [out, edge_dim], conv.lin_edge.bias [out],) conv.mlp.0.weight [2 out, out], conv.mlp.0.bias [2 out],
 * conv.mlp.2.weight [out, 2 out], conv.mlp.2.bias [out] -- 4 .. 10 per layer --, then the head's as in gnnb_model_create: 2 per head
 * linear.  conv.t is NOT among them: it travels as t_per_layer.  Negative: a gnnb_status (GNNB_ERR_INVALID: edge_dim outside
 * 0 .. 16, a layer width above 256, conv_type != GNNB_CONV_GIN, fpx_w != 0, or a description gnnb_model_num_params refuses). */
int gnnb_gen_model_num_params(const gnnb_model_desc *desc, int edge_dim);
/* gnnb_model_create for such a model (models.py GNNModel with gnn_conv = GENConv_GNNB: edge_dim = 0, or GENEConv_GNNB);
 * t_per_layer: desc->num_layers host floats, finite.  Destroy with gnnb_model_destroy, make its workspace with
 * gnnb_workspace_create. */
int gnnb_gen_model_create(const gnnb_model_desc *desc, int edge_dim, const float *t_per_layer, const float *const *host_params, int num_params,
                          gnnb_model **out_model);
/* 1 for a model of gnnb_gen_model_create, 0 for every other model (and for NULL) */
int gnnb_model_gen(const gnnb_model *model);

/* Stage entry, on the prepared batch of any workspace whose tables keep explicit self loops; a workspace of a GCN description is
 * refused.  out[i, c] = agg_i[c] + r[i, c] in the summation order above (r_dev NULL: the bare aggregate).  s_dev, r_dev, out_dev
 * [N, width] with row strides lds, ldr, ldo >= width (s and r may be the two column blocks of one [N, 2 width] GEMM result), width
 * 1 .. 256; edge_dim 0: edge_attr_dev, we_dev, be_dev unread; edge_dim 1 .. 16: edge_attr_dev [E, edge_dim] in COO row order (NULL
 * only for a batch without edges), we_dev [width, edge_dim] rows of stride ldwe, be_dev [width].  16-byte accesses when width, lds,
 * ldr, ldo are multiples of 4 and s, r, out are 16-byte aligned, scalar accesses otherwise: the same bits.  out_dev must not alias
 * an input. */
int gnnb_aggregate_gen(gnnb_workspace *ws, const float *s_dev, int lds, const float *r_dev /*or NULL*/, int ldr, int width,
                       const float *edge_attr_dev /*or NULL*/, int edge_dim /*0..16*/, const float *we_dev, int ldwe,
                       const float *be_dev, float t, float eps_m, float *out_dev, int ldo, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_GEN_H */
