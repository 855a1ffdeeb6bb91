// gnnb_host.h -- what the host translation units of libgnnb_hip.so share (gnnb_model.hip: description and weight upload;
// gnnb_runtime.hip: workspace, graph prep, stage entry points, C-ABI utilities; gnnb_ingest.hip: the PyG mini-batch entries;
// gnnb_forward.hip: the forward): the two handle structs, the error helpers, the dimension helpers of a model description and
// what the units take from each other.  Host only: no kernel unit includes it.  (The dimension helpers and the weights' named slots:
// gnnb_weights.h, which needs no HIP header.)
#pragma once

#include <vector>

#include "gnnb_internal.h"
#include "gnnb_weights.h"
#include "gnnb_order.h"
#include "gnnb_edge.h"
#include "gnnb_pna_edge.h"
#include "gnnb_gat.h"
#include "gnnb_gat_edge.h"
#include "gnnb_gatconv.h"
#include "gnnb_gatconv_edge.h"
#include "gnnb_transformer.h"
#include "gnnb_transformer_edge.h"
#include "gnnb_resgated.h"
#include "gnnb_resgated_edge.h"
#include "gnnb_ggnn.h"
#include "gnnb_rgcn.h"

namespace gnnb {

// sets the calling thread's gnnb_last_error() text and returns `code` (gnnb_runtime.hip)
int fail(int code, const char *fmt, ...);

#define GNNB_HIP_TRY(expr)                                                                        \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail(GNNB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                        __FILE__, __LINE__);                                                      \
    } while (0)

} // namespace gnnb

struct gnnb_model {
    gnnb_model_desc desc;
    float *blob = nullptr; // all weights, device
    size_t blob_floats = 0;
    std::vector<gnnb::LayerWeights> conv; // per conv layer, device pointers by name (gnnb_weights.h: LayerSlots)
    std::vector<const float *> head_w, head_b;
    const float *zf_w1f = nullptr; // 2-layer GCN: layer 1's weight once more, in MFMA-fragment order (see k_gcn2_zf)
    // GIN stacks (k_gcn2_fused<GIN>): every wide matrix once more in EXECUTION order, each hidden x hidden at one stride --
    // Wb0 | Wa1 Wb1 | ... | Wa(L-1) Wb(L-1) -- and the biases likewise.  A last layer narrower than hidden (the reference's
    // benchmark model: 128 -> 64, models.py:530-545) is zero-padded to hidden x hidden: its extra output columns are
    // act(0 + 0) and never leave the kernel.  nullptr when the model is no GIN stack the kernel takes.
    const float *gin_w = nullptr, *gin_b = nullptr;
    gnnb::HeadArgs *head_dev = nullptr; // the MLP head's {weights, biases, widths} once more in device memory: k_gcn2_zf reads it at the
                                        // end of a workgroup's life (by value the 42 dwords stayed in scalar registers through its stage loop)
    int edge_dim = 0; // > 0: a GINE model (gnnb_edge_model_create) or PNA with edge features (gnnb_pna_edge_model_create: desc.conv_type says which) -- every layer has edge_w [in, edge_dim] and edge_b [in]
    int gat_heads = 0;      // > 0: a GATv2 model (gnnb_gat_model_create; desc is a GCN description) -- every layer has w_lr, b_lr, att, gat_bias;
                            // with edge_dim > 0 besides: GATv2 with edge features (gnnb_gat_edge_model_create) -- and w_edge [out, edge_dim]
    float gat_slope = 0.0f; // ... and its leaky_relu slope (a GAT v1 model's as well)
    int gat1_heads = 0;     // > 0: a GAT v1 model (gnnb_gatconv_model_create; desc is a GCN description) -- every layer has w_gat and
                            // gat_bias and none of GCN's slots.  Its own field: gnnb_model_gat_heads stays 0 for such a model;
                            // with edge_dim > 0 besides: GAT v1 with edge features (gnnb_gatconv_edge_model_create) -- and a_edge
                            // [heads, roundup4(edge_dim)]
    int tf_heads = 0;       // > 0: a TransformerConv model (gnnb_transformer_model_create; desc is a GIN description) -- every layer has
                            // w_qkvr, b_qkvr and none of GIN's slots.  Its own field: gnnb_model_gat_heads stays 0 for such a model;
                            // with edge_dim > 0 besides: TransformerConv with edge features (gnnb_transformer_edge_model_create) --
                            // w_qkvre, b_qkvre and w_edge [out, edge_dim] instead
    int gated = 0;          // 1: a ResGatedGraphConv model (gnnb_resgated_model_create; desc is a GIN description) -- every layer has
                            // w_kqvr, b_kqvr and none of GIN's slots; with edge_dim > 0 besides: ResGatedGraphConv with edge features
                            // (gnnb_resgated_edge_model_create) -- w_kqvr of the x column blocks, b_kqvr and w_gv_edge [2 out, edge_dim]
    int ggnn_steps = 0;     // > 0: a GatedGraphConv model (gnnb_ggnn_model_create; desc is a GIN description) of that many steps per
                            // layer -- every layer has w_ggc, w_ggc_next (steps > 1), b_ggc, b_ih and none of GIN's slots
    int rgcn_relations = 0; // > 0: an RGCNConv model (gnnb_rgcn_model_create; desc is a GIN description) of that many relations --
                            // every layer has w_rgcn, b_rgcn and none of GIN's slots
    int device = 0;
    ~gnnb_model(); // frees blob and head_dev (gnnb_model.hip)
};

struct gnnb_workspace {
    gnnb_model_desc desc;
    int max_graphs = 0, max_nodes = 0, max_edges = 0;
    char *blob = nullptr;
    size_t bytes = 0;
    gnnb::BatchTables t{};
    float *act[2] = {nullptr, nullptr}; // ping-pong node embeddings [max_nodes, maxw]
    float *agg = nullptr;               // aggregate output [max_nodes, aggw]
    float *tmp0 = nullptr, *tmp1 = nullptr; // GIN hidden / PNA p,q
    float *pooled = nullptr;            // [max_graphs, np*d]
    float *mlp[2] = {nullptr, nullptr}; // [max_graphs, max(mlp_hidden, mlp_out)]
    bool prepared = false;
    char *ingest_blob = nullptr; // gnnb_workspace_enable_ingest: the outputs and the sort scratch of gnnb_ingest_pyg (ingest_place), one allocation
    bool ingested = false;       // an ingest has been enqueued: gnnb_workspace_check has something to report on
    int edge_dim = 0;            // of the model the workspace was created for (0: no edge weights)
    int gat_heads = 0;           // ... and its heads and slope when it is a GATv2 model (0: it is not)
    float gat_slope = 0.0f;
    int gat1_heads = 0;          // ... and its heads when it is a GAT v1 model (0: it is not; its slope is gat_slope)
    int tf_heads = 0;            // ... and its heads when it is a TransformerConv model (0: it is not)
    int gated = 0;               // ... and 1 when it is a ResGatedGraphConv model
    int ggnn_steps = 0;          // ... and its steps when it is a GatedGraphConv model (0: it is not)
    int rgcn_relations = 0;      // ... and its relations when it is an RGCNConv model (0: it is not)
    gnnb::RgcnSlot *rgcn_rec = nullptr; // such a model's workspace only: the slot records of the batch (k_rgcn_slots), 8 max_edges bytes,
                                 // rebuilt by every _types forward
    char *type_blob = nullptr;   // gnnb_workspace_enable_type_ingest: edge_type in COO row order, int32 [max_edges], one allocation
    char *edge_blob = nullptr;   // gnnb_workspace_enable_edge_ingest: edge_attr in COO row order, [max_edges, edge_dim], one allocation
    char *order_blob = nullptr;  // gnnb_workspace_enable_ordered_ingest: the ordered batch and the staged outputs (order_place), one allocation
    int32_t *order_triple = nullptr, *order_triple_dev = nullptr; // host-mapped (first large graph, node row, edge row) of k_order_graphs, and
                                                                  // its device-visible address
    float2 *pool_part = nullptr; // pieces of graphs that cross the 32-row blocks of the pooling GEMM epilogue (PoolEpilogue::part)
    bool gcoef_ready = false; // t.gcoef holds the prepared batch's GCN coefficients (ensure_gcoef)
    // (both promises are read by graph prep alone: the prepared forward goes by what the prep left -- t.max_graph_nodes_hint,
    // t.tile_rows, gcoef_ready, deg_ready -- so a setter between a prep and its forward speaks of the NEXT prep)
    int max_graph_nodes = 0; // caller's promise (0 = none)
    int max_degree = 0;      // caller's promise on the in-degree (0 = none): gnnb_workspace_set_max_degree
    // PNA degree classes of the prepared batch (launch_degree_classes): valid when deg_ready; deg_delta = the delta it was prepared with
    int32_t *deg_work = nullptr, *deg_perm = nullptr, *deg_tile_cls = nullptr;
    int deg_max_tiles = 0;
    bool deg_ready = false;
    float deg_delta = 0.0f;
    int32_t *plan_scratch = nullptr; // k_stage_cut's binary-lifting tables (GCN / GIN workspaces: stage_cut_levels x (max tiles + 1) ints)
    float prep_delta = 0.0f; // the delta the prepared batch's amp / att tables were computed with (PNA workspaces; 0: none)
    int last_path = GNNB_PATH_NONE; // which kernels the last forward on this workspace ran (gnnb_workspace_last_path)
    // "large segment" of the NEXT batches (gnnb_workspace_set_large_segment): graphs [large_g, B) -- nodes from large_n,
    // edges from large_e -- are exempt from the max_graph_nodes promise and run layer by layer; -1 = no such segment.  Read by
    // graph prep alone, which checks the triple against the batch and bakes it into t (promise_graphs, large_n, large_e): the
    // prepared forward takes the PREPARED batch's segment from there (gnnb_forward.hip, prepared_large_g)
    int large_g = -1, large_n = -1, large_e = -1;
    // fork / join for the large segment: its small kernels run on `side` beside the stack kernel on the caller's stream
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int device = 0;
    int32_t *err_host = nullptr; // host-mapped word the prep kernel drops "flagged" into (lazy detection, see gnnb_graph_prep)
    gnnb::StreamK sk{};      // this workspace's own stream-K scratch (k_linear_dma's large-K tail; part == nullptr: the model has no such GEMM)
    char *stage = nullptr;   // device staging of the host-buffer entry (x | coo | node_ptr | edge_ptr | out), sized for
    size_t stage_bytes = 0;  // the workspace's capacities; allocated by the first gnnb_forward_batched_host call
};

namespace gnnb {
// A GatedGraphConv workspace's scratch (gnnb_ggnn.h), stated once for gnnb_workspace_create, which sizes it, and ggnn_layer, which
// carves it: tmp0 and tmp1 are [max_nodes, tmpw] with tmpw >= GGNN_TMP_BLOCKS * out for every layer.  tmp0 takes a step's GEMM
// output [p | gh] [N, 6 out]; tmp1 takes the two [N, out] state buffers, the second ggnn_state_offset floats behind the first (a
// whole number of 16-byte pieces), so both end within 2 N out + 3 <= 3 N out floats of it
constexpr int GGNN_TMP_BLOCKS = 6;
static_assert(GGNN_TMP_BLOCKS >= 6, "tmp0 holds [p | gh]: six column blocks of a layer's output width");
static_assert(GGNN_TMP_BLOCKS >= 3, "tmp1 holds two [N, out] state buffers and up to 3 floats of alignment between them");
inline size_t ggnn_state_offset(size_t num_nodes, size_t fo) { return (num_nodes * fo + 3) / 4 * 4; }

// An RGCNConv workspace's scratch (gnnb_rgcn.h): tmp0 takes a layer's GEMM output [p_0 | .. | p_{R-1} | root] [N, (R + 1) out]
inline int rgcn_tmp_blocks(int relations) { return relations + 1; }

// the model's MLP head as the readout kernels take it (gnnb_model.hip): the ONLY place that fills a HeadArgs
HeadArgs model_head_args(const gnnb_model *model);

// GNNB_OK, or GNNB_ERR_INVALID for a GINE model / its workspace at `entry`, which takes no edge attributes: says which entry does
int refuse_edge_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// GNNB_OK, or GNNB_ERR_INVALID for a GATv2 model / its workspace at `entry`, which serves the stack kernels' promise only: says which entry runs it
int refuse_gat_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// ... and for a GAT v1 model / its workspace (gnnb_gatconv.h)
int refuse_gatconv_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// ... and for a TransformerConv model / its workspace (gnnb_transformer.h)
int refuse_transformer_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// ... and for a ResGatedGraphConv model / its workspace (gnnb_resgated.h)
int refuse_resgated_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// ... and for a GatedGraphConv model / its workspace (gnnb_ggnn.h)
int refuse_ggnn_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// ... and for an RGCNConv model / its workspace (gnnb_rgcn.h): `use` names the _types entry
int refuse_rgcn_model(const gnnb_model *model, const gnnb_workspace *ws, const char *entry, const char *use);

// gnnb_runtime.hip, for the forward (gnnb_forward.hip) -- each is described where it is defined
int ensure_gcoef(gnnb_workspace *ws, void *stream);
int build_gemm(GemmArgs &g, const gnnb_gemm_seg *segs, int num_segs, const float *w, int ldw, int rows = 1);
int linear_segs(const StreamK *sk_owned, const gnnb_gemm_seg *segs, int num_segs, const float *w_dev, int ldw, const float *bias_dev,
                const float *skip_dev, float *y_dev, int M, int N, int act, void *stream);
bool guest_prep_eligible(const gnnb_workspace *ws, int num_nodes);
// ingest_reported: this call's ingest has made the lazy flag report already; graph prep skips its own, which could already see
// what THIS batch's ingest kernels flagged -- that is for the next call (or gnnb_workspace_check) to report
int graph_prep_impl(gnnb_workspace *ws, const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev,
                    int num_graphs, int num_nodes, int num_edges, float pna_delta, void *stream, PrepParams *defer, bool ingest_reported);
// ... and for the PyG entries (gnnb_ingest.hip) as well
int report_earlier_flags(gnnb_workspace *ws, void *stream);
int check_batch_sizes(const gnnb_workspace *ws, int num_graphs, int num_nodes, int num_edges);
// gnnb_forward.hip, for graph prep
BatchTables small_segment(const gnnb_workspace *ws);
// gnnb_forward.hip: the tail of every gnnb_forward_batched* / gnnb_forward_pyg* entry behind its own checks -- graph prep, then
// the prepared forward; edge_attr_dev: a GINE model's [E, edge_dim] attributes in COO row order (nullptr: a model without)
int forward_batched_tail(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const float *edge_attr_dev, const int32_t *coo_dev,
                         const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs, int num_nodes, int num_edges,
                         float *out_dev, void *stream, bool ingest_reported);

// ... and of gnnb_forward_batched_types / gnnb_forward_pyg_types (gnnb_rgcn.h): the model and workspace checks, graph prep, the slot
// records from edge_type_dev (int32 [E] in COO row order; nullptr only with num_edges == 0), the prepared forward
int forward_batched_types_tail(const gnnb_model *model, gnnb_workspace *ws, const float *x_dev, const int32_t *edge_type_dev,
                               const int32_t *coo_dev, const int32_t *node_ptr_dev, const int32_t *edge_ptr_dev, int num_graphs, int num_nodes,
                               int num_edges, float *out_dev, void *stream, bool ingest_reported);

// the add-on allocations at a workspace's capacities: their arrays placed in the workspace's blob, and their size (the size alone
// while the blob is not allocated)
inline size_t ingest_place(const gnnb_workspace *ws, IngestParams &p) { return ingest_place(ws->ingest_blob, ws->max_graphs, ws->max_nodes, ws->max_edges, p); }
inline size_t order_place(const gnnb_workspace *ws, OrderParams &p) { return order_place(ws->order_blob, ws->max_graphs, ws->max_nodes, ws->max_edges, ws->desc.in_dim, ws->desc.mlp_out, p); }

// The event-timed loop behind the *_timed entries: `warmup` launches, then `iters` launches between two events on `s`;
// launch(i) -> GNNB_OK or an error (which ends the loop and is returned).  *out_us = microseconds per launch.
template <typename F> static int timed_loop(hipStream_t s, int warmup, int iters, F launch, float *out_us)
{
    struct Events { // (destroyed on every return path)
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events()
        {
            if (e0)
                (void)hipEventDestroy(e0);
            if (e1)
                (void)hipEventDestroy(e1);
        }
    } ev;
    GNNB_HIP_TRY(hipEventCreate(&ev.e0));
    GNNB_HIP_TRY(hipEventCreate(&ev.e1));
    int rc = GNNB_OK;
    for (int i = 0; i < warmup && rc == GNNB_OK; i++)
        rc = launch(i);
    if (rc != GNNB_OK)
        return rc;
    GNNB_HIP_TRY(hipStreamSynchronize(s));
    GNNB_HIP_TRY(hipEventRecord(ev.e0, s));
    for (int i = 0; i < iters && rc == GNNB_OK; i++)
        rc = launch(i);
    GNNB_HIP_TRY(hipEventRecord(ev.e1, s));
    GNNB_HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = 0.f;
    GNNB_HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *out_us = ms * 1000.0f / (float)iters;
    return rc;
}
} // namespace gnnb
