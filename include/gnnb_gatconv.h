/*
 * gnnb_gatconv.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): GAT (v1) models, end to end.  gnnb_hip.h,
 * gnnb_order.h, gnnb_edge.h, gnnb_pna_edge.h, gnnb_gat.h and the other extensions are unchanged by these entries (no new version:
 * the library stays at 104).
 *
 * Reference: none in gnnbuilder -- its GATConv_GNNB (gnnbuilder/models.py) raises NotImplementedError and has no native kernel;
 * the class of that name here stays that stub.  The model is GATv1Conv_GNNB (gnn-builder_amd/models.py, class _GATConv): PyG's
 * GATConv(in, out / heads, heads = H, concat = True, negative_slope, add_self_loops = True, bias = True, edge_dim = None,
 * dropout = 0, residual = False),
 *   x' = lin(x) [N, H, C],  C = out / H                                           (lin has no bias)
 *   s_ij[h]   = leaky_relu(sum_c att_src[h, c] x'_j[h, c] + sum_c att_dst[h, c] x'_i[h, c])          j in N(i) u {i}
 *   a_ij[h]   = exp(s_ij[h] - max_j s_ij[h]) / (sum_j exp(s_ij[h] - max_j s_ij[h]) + 1e-16)
 *   out_i[h]  = sum_j a_ij[h] x'_j[h, :] + bias
 * Self loops are PyG's: explicit (v, v) edges of the input are removed and exactly one is added per node.
 *
 * Such a model is an ordinary gnnb_model: its description is a GCN description (conv_type = GNNB_CONV_GCN, every other field as for
 * GCN) and heads (1 .. 8) and negative_slope travel BESIDE it, as they do for a GATv2 model (gnnb_gat.h).  The model's workspaces
 * are GCN workspaces, so graph prep drops explicit (v, v) edges from the tables (gnnb_hip.h, "Explicit self loops") and the kernel
 * adds the one self term itself.  It is a kind of its own: gnnb_model_gat_heads is 0 for it, gnnb_model_gatconv_heads is 0 for a
 * GATv2 model, and neither runs on the other's workspace.
 *
 * What such a model runs: layer by layer (gnnb_workspace_last_path: GNNB_PATH_LAYERWISE, whatever the max_graph_nodes and
 * max_degree promises, which change no bit).  Both terms of the score are per-NODE scalars and linear in x, so att_src and att_dst
 * are folded into the layer's weight at upload: a layer is ONE GEMM, x -> [x' | s_src | s_dst | pad] [N, out + roundup4(2 heads)]
 * on [W ; A_src W ; A_dst W ; 0] in the model's math mode (row out + h = sum_c att_src[h, c] W[h C + c, :], summed in double and
 * rounded once), and ONE launch of k_gat_aggregate (csrc/k_gat.hip: per edge and head one scalar load, one add and one leaky_relu
 * in front of an online softmax fused with the weighted sum, nothing per edge in HBM; bias, the middle layers' skip term and the
 * activation in its epilogue; plain fp32 in every math mode).  Then the readout and the output activation as for every model.  No
 * stack kernel, no fixed-point emulation (fpx_w must be 0), no capture restrictions: nothing in the forward allocates, waits or
 * reads back.
 *
 * It has no edge attributes, so the ordinary entries run it: gnnb_forward_batched, gnnb_forward_prepared, gnnb_forward_pyg (and
 * gnnb_forward_batched_host, gnnb_forward_prepared_prep_next).  The _edges entries of gnnb_edge.h refuse it as a model without
 * edge weights; gnnb_forward_pyg_ordered refuses it (GNNB_ERR_INVALID: the ordered ingest exists for the stack kernels' promise).
 * A model matches a workspace only if the kind, heads and negative_slope are equal too.
 */
#ifndef GNNB_GATCONV_H
#define GNNB_GATCONV_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of a GAT model, in gnnb_gatconv_model_create's order: per conv layer conv.lin.weight [out, in] (no bias),
 * conv.att_src [1, heads, out / heads] (= [out]), conv.att_dst likewise, conv.bias [out] (models.py _GATConv;
 * GNNModel.canonical_param_names), then the head's as in gnnb_model_create: 4 per layer + 2 per head linear.  Negative: a
 * gnnb_status (GNNB_ERR_INVALID: heads outside 1 .. 8, a layer output width not divisible by heads or above 256,
 * conv_type != GNNB_CONV_GCN, fpx_w != 0, or a description gnnb_model_num_params refuses). */
int gnnb_gatconv_model_num_params(const gnnb_model_desc *desc, int heads);
/* gnnb_model_create (load_parameters, model.cpp.jinja:724-730) for such a model (models.py GNNModel with gnn_conv =
 * GATv1Conv_GNNB); also GNNB_ERR_INVALID for a negative_slope that is not finite.  Destroy with gnnb_model_destroy, make its
 * workspace with gnnb_workspace_create. */
int gnnb_gatconv_model_create(const gnnb_model_desc *desc, int heads, float negative_slope, const float *const *host_params, int num_params,
                              gnnb_model **out_model);
/* heads of a model of gnnb_gatconv_model_create; 0 for every other model (a GATv2 model too) and for NULL */
int gnnb_model_gatconv_heads(const gnnb_model *model);

/* Stage entry: one GAT layer behind its GEMM,
 *   out_i = act( sum_{j in N(i) u {i}} a_ij xl_j + bias + skip_i ),   a_ij[h] = softmax_j leaky_relu(ssrc_j[h] + sdst_i[h])
 * on the prepared batch of a GCN workspace (or a GAT / GATv2 model's, which is one): the tables hold no (v, v) edge and the kernel
 * takes the self term itself, first.  xl_dev: rows of `width` floats at row stride ldl >= width; ssrc_dev / sdst_dev: rows of
 * `heads` floats at row strides lds / ldd >= heads -- the column blocks of one [N, width + 2 heads ..] GEMM output are fine;
 * bias_dev [width] or NULL, skip_dev [N, width] or NULL, act a gnnb_act, heads 1 .. 8 dividing width, width 1 .. 256, out_dev
 * [N, width].  16-byte accesses when (width / heads) % 4 == 0 -- a lane's four columns then share a head; width 24 with 8 heads is
 * scalar -- and xl / skip / out and ldl are 16-byte aligned, scalar accesses otherwise.  fp32 in every math mode.  A row without
 * in-edges gives act(xl_i + bias + skip_i), bit for bit.  GNNB_ERR_INVALID (nothing launched): an unprepared workspace, a NULL
 * operand, heads or width out of range, a stride below its row, a negative_slope that is not finite.
 * Summation order -- fixed by the batch and by the form (16-byte or scalar), never by the grid, by which workgroup took a row or
 * by how many lanes share it; a repeat launch gives the same bits, and an H-head launch gives the bits of H one-head launches on
 * the column slices.  Per (row, head): a score is s = z > 0 ? z : z * negative_slope with z = ssrc_j[h] + sdst_i[h] (no sum over
 * columns); the state (m, l, acc) starts from the self term (s_ii, 1, xl_i); the in-edges in CSR slot order in batches of 4:
 * m' = max(m, s_0 .. s_3), l = l exp(m - m') + (((e_0 + e_1) + e_2) + e_3), acc = acc exp(m - m') + e_0 x_0 + .. + e_3 x_3 with
 * e_r = exp(s_r - m'); a row of more than 64 in-edges in pieces of 64 slots, each from (-inf, 0, 0), merged in piece order onto
 * the self state; out = act((acc / (l + 1e-16) + bias) + skip).  exp is the hardware's exp2 of the argument scaled by log2(e). */
int gnnb_aggregate_gat(gnnb_workspace *ws, const float *xl_dev, int ldl, const float *ssrc_dev /*[N, heads]*/, int lds,
                       const float *sdst_dev /*[N, heads]*/, int ldd, const float *bias_dev /*[width] or NULL*/,
                       const float *skip_dev /*[N, width] or NULL*/, int act /*gnnb_act*/, int heads, float negative_slope,
                       float *out_dev /*[N, width]*/, int width, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_GATCONV_H */
