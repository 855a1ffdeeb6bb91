/*
 * gnnb_schnet.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): SchNet models -- the continuous-filter
 * convolution of Schuett et al., PyG's torch_geometric.nn.models.schnet.InteractionBlock / CFConv --, end to end.  Every other header is
 * unchanged by these entries (no new version: the library stays at 104).
 *
 * Reference: none in gnnbuilder.  The model is SchNetConv_GNNB (gnn-builder_amd/models.py, class _SchNetConv).  For a layer in -> out
 * the number of filters is F = out; every edge carries a distance d_ij = edge_attr[e, 0]; G gaussians and a cutoff c > 0:
 *   x1    = lin1(x)                                  [N, F]   conv.lin1.weight [F, in], no bias
 *   rbf_k = exp(coeff (d_ij - mu_k)^2),  mu = linspace(0, c, G),  coeff = -0.5 / (mu_1 - mu_0)^2     (G = 1: mu = [0], coeff = -0.5 / c^2)
 *   h     = ssp(mlp.0(rbf))                          [F]      mlp.0.weight [F, G], mlp.0.bias
 *   w_ij  = mlp.2(h) C(d_ij),   C(d) = 0.5 (cos(pi d / c) + 1)      mlp.2.weight [F, F], mlp.2.bias; no clamp beyond c, as PyG
 *   agg_i = sum_{j -> i} x1_j * w_ij                 (a row without in-edges: 0)
 *   out_i = lin(ssp(lin2(agg_i)))                    conv.lin2 [out, F] + bias, lin [out, out] + bias
 *   ssp(v) = softplus(v) - ln 2
 * No self loop is added or removed, duplicate edges count as often as they occur, an explicit (v, v) edge is an ordinary edge.
 *
 * Such a model is an ordinary gnnb_model: its description is a GIN description (conv_type = GNNB_CONV_GIN, gin_eps ignored, every
 * other field as for GIN; fpx_w must be 0; every layer width at most 256) with `gaussians` (1 .. 64) and `cutoff` BESIDE it;
 * gnnb_model_edge_dim reports 1, gnnb_model_schnet the gaussians.  A model matches a workspace only of the same kind, gaussians and
 * cutoff.
 *
 * A layer is the GEMM x -> x1, ONE launch of k_schnet_cfconv (csrc/k_schnet.hip: the filter MLP on the matrix cores inside the
 * aggregate, v_mfma_f32_16x16x4_f32, exact fp32 products in every math mode; neither the basis [E, G], nor the hidden tensor [E, F], nor
 * the filter [E, F] reaches HBM) with its short fix-up pass, the GEMM lin2, ssp in place, and the GEMM lin with the model's skip term
 * and activation in its epilogue.  The slot -> row map the kernel reads is built once per forward.
 *
 * Summation order of the aggregate -- fixed by the batch and by the tile size TE (64 slots, 32 where the LDS carve asks for it: a
 * function of width and gaussians alone), never by the grid or by occupancy; 16-byte and scalar gathers give the same bits: rbf W1^T
 * and h W2^T are the matrix instruction's chains over k steps 0, 1, .. from the bias, step t adding columns 4 t .. 4 t + 3; the
 * message is (w C) x1_j; per (row, column) the messages of one tile of TE consecutive CSR slots in slot order onto 0; a row split
 * over tiles: its pieces in tile order onto 0.  No float atomics.
 *
 * What such a model runs: layer by layer (GNNB_PATH_LAYERWISE), through the _edges entries of gnnb_edge.h (gnnb_forward_batched_edges,
 * gnnb_forward_prepared_edges, gnnb_workspace_enable_edge_ingest, gnnb_ingest_pyg_edges, gnnb_forward_pyg_edges) with ONE edge_attr
 * [E, 1] for every layer.  Every other whole-model entry refuses it with GNNB_ERR_INVALID and names the right one.  Nothing in the
 * forward allocates, waits or reads back: it can be captured.
 *
 * Out of scope: num_filters != out, the radius graph and the distances from positions, the atom embedding and the atomwise readout,
 * more than 64 gaussians, widths above 256, per-layer distances, the reduced math modes inside the kernel, the LDS-resident stack
 * kernels and every fused rung, the ordered ingest, Project (code generation), bench.py workloads.
 */
#ifndef GNNB_SCHNET_H
#define GNNB_SCHNET_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of a SchNet model, in gnnb_schnet_model_create's order: per conv layer conv.lin1.weight [out, in], mlp.0.weight
 * [out, gaussians], mlp.0.bias [out], mlp.2.weight [out, out], mlp.2.bias [out], conv.lin2.weight [out, out], conv.lin2.bias [out],
 * lin.weight [out, out], lin.bias [out] -- 9 per layer --, then the head's as in gnnb_model_create: 2 per head linear.  Negative: a
 * gnnb_status (GNNB_ERR_INVALID: gaussians outside 1 .. 64, a layer width above 256, conv_type != GNNB_CONV_GIN, fpx_w != 0, or a
 * description gnnb_model_num_params refuses). */
int gnnb_schnet_model_num_params(const gnnb_model_desc *desc, int gaussians);
/* gnnb_model_create for such a model (models.py GNNModel with gnn_conv = SchNetConv_GNNB); cutoff > 0 and finite.  Destroy with
 * gnnb_model_destroy, make its workspace with gnnb_workspace_create. */
int gnnb_schnet_model_create(const gnnb_model_desc *desc, int gaussians, float cutoff, const float *const *host_params, int num_params,
                             gnnb_model **out_model);
/* the gaussians of a model of gnnb_schnet_model_create, 0 for every other model (and for NULL) */
int gnnb_model_schnet(const gnnb_model *model);

/* Stage entry, on the prepared batch of any workspace whose tables keep explicit self loops; a workspace of a GCN description is
 * refused.  out[i] = agg_i of the formula above in its summation order.  x1_dev, out_dev [N, width] with row strides ldx, ldo >=
 * width, width 1 .. 256; edge_dist_dev [E] in COO row order (NULL only for a batch without edges); w1_dev [width, gaussians] and
 * w2_dev [width, width] rows of stride ldw1, ldw2; b1_dev, b2_dev [width].  16-byte gathers when width and ldx are multiples of 4 and
 * x1 is 16-byte aligned, scalar ones otherwise: the same bits.  A workspace of a SchNet model carries the kernel's scratch; on any
 * other workspace the first call allocates it (that call cannot be captured).  out_dev must not alias an input. */
int gnnb_aggregate_cfconv(gnnb_workspace *ws, const float *x1_dev, int ldx, int width, const float *edge_dist_dev, const float *w1_dev,
                          int ldw1, const float *b1_dev, const float *w2_dev, int ldw2, const float *b2_dev, int gaussians, float cutoff,
                          float *out_dev, int ldo, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_SCHNET_H */
