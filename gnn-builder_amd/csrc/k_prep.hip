// k_prep.hip -- graph prep: COO -> CSR-by-destination + degree scalers + node tiles (latency bound)
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include <cstring>

#include "gnnb_prep.h"

namespace gnnb {

// k_graph_prep: one wavefront per graph of the batch (prep_one_graph), or -- GROUP > 1 -- per GROUP consecutive graphs with
// their fetches batched (prep_graph_group); wave B, one past the last graph, writes the end entries of the tables and gives
// the rows that no graph owns empty records.  The three paths a graph can take are described in gnnb_prep.h.
template <int PREP_FAST_NODES, int GROUP>
__global__ __launch_bounds__(WG) void k_graph_prep(PrepParams p)
{
    __shared__ __attribute__((aligned(16))) int32_t s_first[WG / 64][prep_wave_lds_ints(PREP_FAST_NODES)]; // first four sources of every node (read / written 16 B at a time)
    // Highest wave priority: with batches in flight on several streams this kernel runs BESIDE the conv-stack kernel of
    // another batch (one wave slot per SIMD is left over there) and sits on its own stream's critical path -- 37-53 us
    // instead of 7 when it queues behind sixteen MFMA-issuing waves per CU.  It is a few hundred instructions per wave;
    // letting them issue first costs the big kernel nothing measurable (C2 step 55.5 -> 54.0 us).
    __builtin_amdgcn_s_setprio(GNNB_GUEST_PRIO);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (GROUP > 1)
        prep_graph_group<PREP_FAST_NODES, GROUP>(p, (blockIdx.x * (WG / 64) + wave) * GROUP, lane, s_first[wave]);
    else {
        const int g = blockIdx.x * (WG / 64) + wave;
        if (g > p.B)
            return;
        prep_one_graph<PREP_FAST_NODES>(p, g, lane, s_first[wave]);
    }
}

// the kernel arguments of one graph prep (also handed to the readout kernel that runs the prep of its stream's next batch, k_readout.hip)
PrepParams make_prep_params(const int32_t *coo, const int32_t *node_ptr, const int32_t *edge_ptr, const BatchTables &t, float pna_delta,
                            int drop_self_loops)
{
    int cut_log2 = -1; // (row-balanced aggregate ranges: only for a power-of-two range count)
    if (t.agg_cut && t.agg_cut_n > 0 && (t.agg_cut_n & (t.agg_cut_n - 1)) == 0 && t.num_nodes > 0)
        for (cut_log2 = 0; (1 << cut_log2) < t.agg_cut_n; cut_log2++) {
        }
    PrepParams p;
    memset(&p, 0, sizeof(p)); // (padding too: the runtime compares parameter blocks bytewise)
    p.coo = (const int2 *)coo, p.node_ptr = node_ptr, p.edge_ptr = edge_ptr;
    p.B = t.num_graphs, p.N = t.num_nodes, p.E = t.num_edges;
    p.row_ptr = t.row_ptr, p.col = t.col, p.eid = t.eid, p.node_rec = t.node_rec, p.dinv = t.dinv, p.amp = t.amp, p.att = t.att;
    p.delta = pna_delta;
    p.tile_first = t.tile_first, p.tile_edge = t.tile_edge, p.tile_graph = t.tile_graph, p.graph_ptr = t.graph_ptr;
    p.tile_rows = t.tile_rows, p.num_tiles = t.num_tiles, p.max_graph_nodes_hint = t.max_graph_nodes_hint, p.promise_graphs = t.promise_graphs;
    p.large_n = t.large_n, p.large_e = t.large_e, p.drop_self = drop_self_loops, p.err = t.err, p.err_host = t.err_host_dev;
    p.agg_cut = cut_log2 >= 0 ? t.agg_cut : nullptr, p.cut_log2 = cut_log2, p.node_graph = t.node_graph;
    return p;
}

hipError_t launch_graph_prep(const PrepParams &p, hipStream_t s)
{
    // the workspace's flag word is zeroed when the workspace is created and again whenever it is read
    // (gnnb_workspace_check), so no per-batch memset node sits in front of this launch
    const int waves = p.B + 1;
    const dim3 one(prep_grid_blocks(waves, 1, WG)), four(prep_grid_blocks(waves, 4, WG));
    if (p.max_graph_nodes_hint > 0 && p.max_graph_nodes_hint <= 64) {
        // molecule-sized graphs: a wave prepares a GROUP of graphs with its fetches batched (prep_graph_group) once there are enough
        // graphs to fill the chip's guest wave slots several times over
        // (BASELINE config 2, 4096 graphs, three batches in flight: 41.2 instead of 42.3 us per step; ONE batch in flight, where the chip's
        // every wave slot is free, is slower with groups -- 58.9 instead of 55.7 us per forward: option prep_group = 1)
        const int group = (int)options().prep_group;
        if (group >= 4 && waves >= 2048)
            hipLaunchKernelGGL((k_graph_prep<64, 4>), four, dim3(WG), 0, s, p);
        else
            hipLaunchKernelGGL((k_graph_prep<64, 1>), one, dim3(WG), 0, s, p);
    } else
        hipLaunchKernelGGL((k_graph_prep<256, 1>), one, dim3(WG), 0, s, p);
    return hipGetLastError();
}

} // namespace gnnb
