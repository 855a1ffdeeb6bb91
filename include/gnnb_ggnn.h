/*
 * gnnb_ggnn.h -- extension of the C ABI in gnnb_hip.h (same library, libgnnb_hip.so): GatedGraphConv models (the Gated Graph
 * Neural Network of Li et al., the update function of Gilmer's MPNN family), end to end.  Every other header is unchanged by
 * these entries (no new version: the library stays at 104).
 *
 * Reference: none in gnnbuilder.  The model is GatedGraphConv_GNNB (gnn-builder_amd/models.py, class _GatedGraphConv): PyG's
 * GatedGraphConv(out_channels = out, num_layers = steps, aggr = 'add', bias = True),
 *   h = [x | 0]                       x [N, in] padded with zero columns to out (in <= out)
 *   for t in 0 .. steps - 1:
 *     m_i = sum_{j in N(i)} (h_j @ weight[t])            weight [steps, out, out], a plain matmul; j in N(i) -- the input's edges
 *     h   = GRUCell(m, h)                                ONE cell (torch.nn.GRUCell, gate rows r, z, n), shared by all steps:
 *       gi = m @ weight_ih^T + bias_ih,  gh = h @ weight_hh^T + bias_hh
 *       r = sigmoid(gi_r + gh_r),  z = sigmoid(gi_z + gh_z),  n = tanh(gi_n + r * gh_n),  h' = n + z * (h - n)
 * Self loops: none is added and none is removed.  An explicit (v, v) edge of the input is an ordinary edge; a node without
 * in-edges gets GRUCell(0, h).
 *
 * Such a model is an ordinary gnnb_model: its description is a GIN description (conv_type = GNNB_CONV_GIN, gin_eps ignored, every
 * other field as for GIN) with a "ggnn" mark and `steps` BESIDE it.  The reason is gnnb_transformer.h's: the tables of a GCN
 * workspace drop explicit (v, v) edges in graph prep (gnnb_hip.h, "Explicit self loops"), the tables of a GIN workspace keep them.
 * gnnb_model_ggnn_steps reports the steps; gnnb_model_is_resgated, gnnb_model_gat_heads, gnnb_model_gatconv_heads,
 * gnnb_model_transformer_heads and gnnb_model_edge_dim are 0 for such a model.
 *
 * The fold.  Everything in front of the GRU's nonlinearities is linear: m @ weight_ih^T = sum_j h_j @ (weight[t] @ weight_ih^T).  At
 * upload W_p[t] = weight_ih @ weight[t]^T [3 out, out] is formed in double and rounded once, and stacked on weight_hh.  A step is
 * then ONE GEMM h -> [p | gh] [N, 6 out] on [W_p[t] ; weight_hh] with the bias vector [0 | bias_hh] in the model's math mode -- the p
 * block takes NO bias: it would be counted once per edge --, and ONE launch of k_ggnn_aggregate (csrc/k_ggnn.hip: the sum of the
 * neighbours' p rows and the whole GRU cell in one pass over the edges; bias_ih is added once per row, behind the sum; plain fp32 in
 * every math mode).  Neither the messages [E, out], nor the aggregated message [N, out], nor the input side's gate pre-activations
 * [N, 3 out] reach HBM.  At step 0 of a layer with in < out the GEMM takes only the first `in` input columns (K = in): the zero
 * padding costs no flops, and the kernel takes h's columns at or beyond `in` as 0 without loading them.
 *
 * What such a model runs: layer by layer (gnnb_workspace_last_path: GNNB_PATH_LAYERWISE, whatever the max_graph_nodes and
 * max_degree promises, which change no bit).  A layer is steps x (GEMM, kernel) on two [N, out] state buffers used in turn; the
 * inner steps run with no skip term and no activation, the last step applies the middle layers' skip term and the layer's
 * activation in the kernel's epilogue.  Then the readout and the output activation as for every model.  No stack kernel, no stage
 * plan, no fixed-point emulation (fpx_w must be 0), no capture restrictions: nothing in the forward allocates, waits or reads
 * back.
 *
 * It has no edge attributes, so the ordinary entries run it: gnnb_forward_batched, gnnb_forward_prepared, gnnb_forward_pyg,
 * gnnb_forward_batched_host and gnnb_forward_prepared_prep_next.  The _edges entries of gnnb_edge.h refuse it as a model without
 * edge weights; gnnb_forward_pyg_ordered refuses it and names gnnb_forward_pyg.  A model matches a workspace only if both are ggnn
 * with the same steps.
 *
 * Out of scope: aggr other than add, bias = False at model level (the stage entry's b_ih = NULL covers the kernel side),
 * edge_weight, edge features, widths above 256, steps above 8, a GRU fused into the GEMM's epilogue.
 */
#ifndef GNNB_GGNN_H
#define GNNB_GGNN_H

#include "gnnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameter tensors of a GatedGraphConv model of `steps` steps per layer, in gnnb_ggnn_model_create's order: per conv layer
 * conv.weight [steps, out, out], conv.rnn.weight_ih [3 out, out], conv.rnn.weight_hh [3 out, out], conv.rnn.bias_ih [3 out],
 * conv.rnn.bias_hh [3 out] (models.py _GatedGraphConv; GNNModel.canonical_param_names), then the head's as in gnnb_model_create:
 * 5 per layer + 2 per head linear.  Negative: a gnnb_status (GNNB_ERR_INVALID: steps outside 1 .. 8, a layer whose input width
 * exceeds its output width, a layer output width above 256, conv_type != GNNB_CONV_GIN, fpx_w != 0, or a description
 * gnnb_model_num_params refuses). */
int gnnb_ggnn_model_num_params(const gnnb_model_desc *desc, int steps);
/* gnnb_model_create (load_parameters, model.cpp.jinja:724-730) for such a model (models.py GNNModel with gnn_conv =
 * GatedGraphConv_GNNB, gnn_steps = steps).  Destroy with gnnb_model_destroy, make its workspace with gnnb_workspace_create. */
int gnnb_ggnn_model_create(const gnnb_model_desc *desc, int steps, const float *const *host_params, int num_params, gnnb_model **out_model);
/* steps of a model of gnnb_ggnn_model_create; 0 for every other model (and for NULL) */
int gnnb_model_ggnn_steps(const gnnb_model *model);

/* Stage entry: one GatedGraphConv step behind its GEMM.  Per (row i, column c), with g in r, z, n the three column blocks:
 *   acc_g = sum_{j in N(i)} p_j[g];   gi_g = acc_g + b_ih[g]
 *   r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(fma(r, gh_n, gi_n));  u = fma(z, h - n, n);  out = act(u + skip)
 * on the prepared batch of any workspace whose tables keep explicit self loops (a GIN, GINE, GraphSAGE, PNA, TransformerConv,
 * ResGatedGraphConv or GatedGraphConv model's); a workspace of a GCN description (a GCN, GATv2 or GAT model's) is refused
 * (GNNB_ERR_INVALID: its tables have dropped the (v, v) edges).  p_dev / gh_dev: rows of 3 width floats in blocks r | z | n at row
 * strides ldp / ldgh >= 3 width -- the two halves of one [N, 6 width] GEMM output are fine; h_dev: rows of h_width <= width floats
 * at stride ldh >= h_width, its columns at or beyond h_width are taken as 0 and are not loaded; b_ih_dev [3 width] or NULL;
 * skip_dev [N, width] or NULL; act a gnnb_act; width 1 .. 256; out_dev [N, width], which must not alias an input.  An absent term
 * adds nothing: it does not add 0.  A row without in-edges gives the cell on gi = b_ih (0 with b_ih NULL).  16-byte accesses when
 * width % 4 == 0, h_width % 4 == 0 and p / gh / h / b_ih / skip / out and the strides are 16-byte aligned, scalar accesses
 * otherwise.  fp32 in every math mode.  GNNB_ERR_INVALID (nothing launched): an unprepared workspace, a GCN description's workspace,
 * a NULL p, gh, h or out (unless the prepared batch has no nodes: nothing is read then), width outside 1 .. 256, h_width outside
 * 1 .. width, ldp or ldgh below 3 width, ldh below h_width, an act that is no gnnb_act.
 * The gates: sigmoid(s) = 1 / (1 + exp(-s)) as the hardware's reciprocal of 1 + the hardware's exp2 of s * -log2(e);
 * tanh(s) = 1 - 2 / (1 + exp(2 s)) as fma(-2, rcp(1 + exp2(s * 2 log2(e))), 1) (exp2 and rcp 1 ulp each).  Both saturate exactly: an
 * argument of -200 gives a gate of exactly 0 and a tanh of exactly -1, +200 exactly 1 and +1, and no finite input gives a NaN.
 * Summation order -- fixed by the batch and by the form (16-byte or scalar), never by the grid or by which workgroup took a row;
 * a repeat launch gives the same bits.  Per (row, column, block): the in-edges in CSR slot order in batches of 4, plain adds in
 * slot order, acc = (((acc + p_0) + p_1) + p_2) + p_3, slots past the row's end taking no part; a row of more than 64 in-edges in
 * pieces of 64 slots, each summed from 0, the pieces added in piece order onto 0; b_ih once, behind the sum. */
int gnnb_aggregate_ggnn(gnnb_workspace *ws, const float *p_dev, int ldp, const float *gh_dev, int ldgh, const float *h_dev, int ldh,
                        int h_width, const float *b_ih_dev /*[3 width] or NULL*/, const float *skip_dev /*[N, width] or NULL*/,
                        int act /*gnnb_act*/, float *out_dev /*[N, width]*/, int width, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNB_GGNN_H */
