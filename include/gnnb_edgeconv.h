/*
 * gnnb_edgeconv.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): EdgeConv models -- the layer of DGCNN (Wang et
 * al.), PyG's EdgeConv(nn, aggr="max") --, end to end.  Every other header is unchanged by these entries (no new version: the library
 * stays at 104).
 *
 * Reference: none in gnnbuilder.  The model is EdgeConv_GNNB (gnn-builder_amd/models.py).  For a layer in -> out the hidden width of
 * nn is H = out:
 *   m_ij  = nn.2(relu(nn.0([x_i | x_j - x_i])))       nn.0.weight [out, 2 in], nn.0.bias [out], nn.2.weight [out, out], nn.2.bias [out]
 *   out_i = max_{j -> i} m_ij                         (i = edge_index[1]; a row without in-edges: 0, and NO bias)
 * No self loop is added or removed, duplicate edges count as often as they occur, an explicit (v, v) edge is an ordinary edge.
 *
 * Such a model is an ordinary gnnb_model: its description is a GIN description (conv_type = GNNB_CONV_GIN, gin_eps ignored, every
 * other field as for GIN; fpx_w must be 0; every layer width at most 256); gnnb_model_edgeconv reports 1.  A model matches a workspace
 * only of the same kind.
 *
 * max does not commute with nn.2, so the second linear stays per edge; the first folds into the nodes at upload:
 *   nn.0([x_i | x_j - x_i]) = (W1a - W1b) x_i + b1 + W1b x_j = a_i + b_j,     nn.0.weight = [W1a | W1b]
 * (the difference taken in double and rounded once).  A layer is ONE GEMM x -> [a | b] [N, 2 out] and ONE launch of k_edgeconv_max
 * (csrc/k_edgeconv.hip: relu(a_i + b_j) formed in LDS from two gathered rows, the product with nn.2.weight on the matrix cores --
 * v_mfma_f32_16x16x4_f32, exact fp32 products in every math mode --, a segmented max from -inf in LDS; neither the hidden tensor [E, H]
 * nor the messages [E, out] reach HBM) with its short fix-up pass; nn.2.bias (it commutes with the max; rows with an in-edge only),
 * the model's skip term and activation in its store.  The slot -> row map the kernel reads is built once per forward.
 *
 * Order: a message is the matrix instruction's chain from 0 over K-panels of 16 columns in order, within panel p step t adding columns
 * 16 p + t + {0, 4, 8, 12}; the max is order-free.  The result does not depend on the tile size (64 slots, 32 where the LDS carve asks
 * for it), the grid, where a row is split over tiles, or 16-byte against scalar gathers: the same bits.  No float atomics.
 *
 * What such a model runs: layer by layer (GNNB_PATH_LAYERWISE), through the ordinary entries of gnnb_hip.h (gnnb_forward_batched,
 * gnnb_forward_prepared, gnnb_forward_pyg, ...).  The _edges entries of gnnb_edge.h, the _types entries of gnnb_rgcn.h and
 * gnnb_forward_pyg_ordered refuse it with GNNB_ERR_INVALID and name the ordinary one.  Nothing in the forward allocates, waits or
 * reads back: it can be captured.
 *
 * Out of scope: aggr add / mean / sum (the aggregate-first follow-up: sum_j relu(a_i + b_j), then nn.2 as a node GEMM), H != out in a
 * model (the stage entry takes any), a deeper nn or BatchNorm inside it (eval-mode BatchNorm folds into the linears), DynamicEdgeConv's
 * k-NN, widths above 256, the LDS-resident stack kernels and every fused rung, the fixed-point emulation, Project (code generation),
 * bench.py workloads.
 */
#ifndef GNNB_EDGECONV_H
#define GNNB_EDGECONV_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of an EdgeConv model, in gnnb_edgeconv_model_create's order: per conv layer nn.0.weight [out, 2 in], nn.0.bias
 * [out], nn.2.weight [out, out], nn.2.bias [out] -- 4 per layer --, then the head's as in gnnb_model_create: 2 per head linear.
 * Negative: a gnnb_status (GNNB_ERR_INVALID: a layer width above 256, conv_type != GNNB_CONV_GIN, fpx_w != 0, or a description
 * gnnb_model_num_params refuses). */
int gnnb_edgeconv_model_num_params(const gnnb_model_desc *desc);
/* gnnb_model_create for such a model (models.py GNNModel with gnn_conv = EdgeConv_GNNB, gnn_aggr = "max").  Destroy with
 * gnnb_model_destroy, make its workspace with gnnb_workspace_create. */
int gnnb_edgeconv_model_create(const gnnb_model_desc *desc, const float *const *host_params, int num_params, gnnb_model **out_model);
/* 1 for a model of gnnb_edgeconv_model_create, 0 for every other model (and for NULL) */
int gnnb_model_edgeconv(const gnnb_model *model);

/* Stage entry, on the prepared batch of any workspace whose tables keep explicit self loops; a workspace of a GCN description is
 * refused.  out[i] = act(max_{j -> i} (w2 relu(a_i + b_j)) + b2 + skip_i) for a row with in-edges, act(skip_i) for one without.
 * ab_dev [N, 2 hidden] rows of stride ldab >= 2 hidden: the column blocks [a | b] of one GEMM result; hidden, width 1 .. 256; w2_dev
 * [width, hidden] rows of stride ldw2; b2_dev [width] or NULL; skip_dev [N, width] contiguous or NULL; act a gnnb_act; out_dev [N,
 * width] rows of stride ldo >= width.  16-byte gathers when hidden and ldab are multiples of 4 and ab is 16-byte aligned, scalar ones
 * otherwise: the same bits.  A workspace of an EdgeConv or a SchNet model carries the kernel's scratch; on any other workspace the
 * first call allocates it (that call cannot be captured).  out_dev must not alias an input. */
int gnnb_aggregate_edgeconv(gnnb_workspace *ws, const float *ab_dev, int ldab, int hidden, const float *w2_dev, int ldw2, const float *b2_dev,
                            int width, const float *skip_dev, int act, float *out_dev, int ldo, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_EDGECONV_H */
