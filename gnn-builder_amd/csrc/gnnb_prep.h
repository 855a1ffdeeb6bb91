// gnnb_prep.h -- graph prep (COO -> CSR by destination, degree scalers, node tiles) as DEVICE FUNCTIONS: one wavefront per graph.
// Included by k_prep.hip (the stand-alone kernel k_graph_prep) and by k_readout.hip: the readout kernel k_head_small can run the
// graph prep of the NEXT batch of its stream as extra workgroups (PrepParams, gnnb_internal.h).
// Reference: compute_degree_tables + compute_neighbor_tables (gnn_builder_lib.h:1051-1124), edge-index table (:1126-1166).
// A graph of n nodes and ne edges (its clamped ranges) takes one of three paths, chosen wave-uniformly in prep_one_graph:
//   n <= 64 and ne <= 64                                  prep_graph_small     (molecule path)
//   else n <= PREP_FAST_NODES and ne <= PREP_FAST_EDGES   prep_graph_ballot    (register path)
//   else                                                  prep_graph_scan
#pragma once
#include "gnnb_device.h"

namespace gnnb {

static constexpr int PREP_REG_CHUNKS = 4;   // scan path: edge chunks of 64 a wave keeps in registers
static constexpr int PREP_FAST_EDGES = 256; // register path: 4 edge chunks
// One statement of the prep's launch shape, read by k_graph_prep and by the guest form in k_head_small: blocks of `threads`
// threads for `waves` waves' worth of graphs at G graphs per wave, and the LDS ints of one wave (s_first_w below)
constexpr int prep_grid_blocks(int waves, int G, int threads) { return ((waves + G - 1) / G + threads / 64 - 1) / (threads / 64); }
constexpr int prep_wave_lds_ints(int fast_nodes) { return fast_nodes * 4; }

// the clamped node and edge range of one graph
struct GraphRange {
    int n0, n1, e0, e1;
};

// batch-validation flag of graph prep (report_flag, gnnb_device.h)
__device__ __forceinline__ void flag_batch(const PrepParams &p, int bits) { report_flag(p.err, p.err_host, bits); }

// ---- the steps the three paths share ------------------------------------------------------------------------------------
// Does edge e enter the tables?  An edge that leaves its graph is an error (`bad`) and is dropped, so that later gathers stay
// in range; on a GCN workspace an explicit self loop is not an edge (PyG add_remaining_self_loops, see gnnb_hip.h).
__device__ __forceinline__ bool accept_edge(const PrepParams &p, const GraphRange &r, const int2 e, bool &bad)
{
    if (e.x < r.n0 || e.x >= r.n1 || e.y < r.n0 || e.y >= r.n1) {
        bad = true;
        return false;
    }
    return !(p.drop_self && e.x == e.y);
}

// PNA's degree scalers of row v with in-degree d (gnn_builder_lib.h:1972-1982; delta <= 0: the model has no PNA layer, the
// scalers are not needed)
__device__ __forceinline__ void store_degree_scalers(const PrepParams &p, int v, int d)
{
    if (p.delta > 0.0f) {
        const int dcl = d < 1 ? 1 : d;
        const float logd = logf((float)(dcl + 1));
        p.amp[v] = logd / p.delta;
        p.att[v] = p.delta / logd;
    }
}

// node record of row v: CSR start, in-degree, first four sources
__device__ __forceinline__ void store_node_record(const PrepParams &p, int v, int start, int deg, int4 first)
{
    p.node_rec[2 * (size_t)v] = make_int4(start, deg, first.x, first.y);
    p.node_rec[2 * (size_t)v + 1] = make_int4(first.z, first.w, 0, 0);
}

// default first-four-sources record of node v in a wave's LDS: unused source slots alias the node itself
__device__ __forceinline__ void default_first_sources(int32_t *s_first_w, int slot, int v)
{
    *reinterpret_cast<int4 *>(s_first_w + slot * 4) = make_int4(v, v, v, v);
}

// The exchange through s_first_w crosses lanes: wave_barrier alone is not a memory ordering at the IR level, so each
// hand-over is a wavefront-scope release / acquire pair -- no instruction on the device, only a compiler ordering.
__device__ __forceinline__ void wave_handover()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows [r0, r1) that no graph owns: empty records (degree 0)
__device__ __forceinline__ void prep_empty_rows(const PrepParams &p, int r0, int r1, int lane)
{
    for (int v = r0 + lane; v < r1; v += 64) {
        p.row_ptr[v] = 0;
        if (p.node_graph)
            p.node_graph[v] = -1;
        store_node_record(p, v, 0, 0, make_int4(v, v, v, v));
        p.dinv[v] = 1.0f;
        store_degree_scalers(p, v, 0);
    }
}

// ---- scan path: n > PREP_FAST_NODES or ne > PREP_FAST_EDGES (any graph size) ----------------------------------------------
// Lanes hold DESTINATION NODES, 64 at a time; the edges are scanned one at a time by register broadcasts (v_readlane with a
// scalar index), so the sort is stable by construction and needs no atomics and no LDS.  Up to 64 * PREP_REG_CHUNKS edges
// stay in registers (lane l holds edge 64c + l of chunk c); a longer edge list is re-read from global memory (L2) chunk by
// chunk for every 64 nodes.
__device__ void prep_graph_scan(const PrepParams &p, const GraphRange r, int lane)
{
    const int n0 = r.n0, n1 = r.n1, e0 = r.e0;
    const int ne = r.e1 - r.e0;
    const int nchunks = (ne + 63) >> 6;
    const bool inreg = nchunks <= PREP_REG_CHUNKS; // wave-uniform
    bool bad = false;

    // a dropped edge is neutralised: dst = -1 never matches, src stays in range
    auto fetch = [&](int c, int &es, int &ed) {
        const int i = c * 64 + lane;
        es = n0;
        ed = -1;
        if (i < ne) {
            const int2 e = p.coo[e0 + i];
            if (accept_edge(p, r, e, bad)) {
                es = e.x;
                ed = e.y;
            }
        }
    };
    int rs[PREP_REG_CHUNKS], rd[PREP_REG_CHUNKS];
#pragma unroll
    for (int c = 0; c < PREP_REG_CHUNKS; c++) {
        rs[c] = n0;
        rd[c] = -1;
        if (inreg && c < nchunks)
            fetch(c, rs[c], rd[c]);
    }

    int base = e0;
    for (int c0 = n0; c0 < n1; c0 += 64) {
        const int v = c0 + lane;
        const bool active = v < n1;
        // ---- in-degree of node v: scan the edges, one broadcast per edge
        int cnt = 0;
        if (inreg) {
#pragma unroll
            for (int c = 0; c < PREP_REG_CHUNKS; c++) {
                if (c < nchunks) {
                    const int m = min(64, ne - c * 64);
                    for (int i = 0; i < m; i++)
                        cnt += (__builtin_amdgcn_readlane(rd[c], i) == v) ? 1 : 0;
                }
            }
        } else {
            for (int c = 0; c < nchunks; c++) {
                int es, ed;
                fetch(c, es, ed);
                const int m = min(64, ne - c * 64);
                for (int i = 0; i < m; i++)
                    cnt += (__builtin_amdgcn_readlane(ed, i) == v) ? 1 : 0;
            }
        }
        if (!active)
            cnt = 0;
        const int incl = wave_scan_incl(cnt);
        const int start = base + incl - cnt;
        if (active) {
            p.row_ptr[v] = start;
            p.dinv[v] = 1.0f / sqrtf(1.0f + (float)cnt);
            store_degree_scalers(p, v, cnt);
        }
        // ---- stable fill: edges are visited in COO order; the first four sources also go into the node record
        int pos = start;
        int jf[4] = {v, v, v, v};
        auto put = [&](int src, int edge) {
            const int q = pos - start;
            if (q == 0) jf[0] = src;
            else if (q == 1) jf[1] = src;
            else if (q == 2) jf[2] = src;
            else if (q == 3) jf[3] = src;
            p.eid[pos] = edge; // COO row of the CSR slot (compute_neighbor_and_edge_index_tables, gnn_builder_lib.h:1126-1166)
            p.col[pos++] = src;
        };
        if (inreg) {
#pragma unroll
            for (int c = 0; c < PREP_REG_CHUNKS; c++) {
                if (c < nchunks) {
                    const int m = min(64, ne - c * 64);
                    for (int i = 0; i < m; i++) {
                        const int d = __builtin_amdgcn_readlane(rd[c], i);
                        const int sc = __builtin_amdgcn_readlane(rs[c], i);
                        if (d == v)
                            put(sc, e0 + c * 64 + i);
                    }
                }
            }
        } else {
            for (int c = 0; c < nchunks; c++) {
                int es, ed;
                fetch(c, es, ed);
                const int m = min(64, ne - c * 64);
                for (int i = 0; i < m; i++) {
                    const int d = __builtin_amdgcn_readlane(ed, i);
                    const int sc = __builtin_amdgcn_readlane(es, i);
                    if (d == v)
                        put(sc, e0 + c * 64 + i);
                }
            }
        }
        if (active)
            store_node_record(p, v, start, cnt, make_int4(jf[0], jf[1], jf[2], jf[3]));
        base += __shfl(incl, 63, 64);
    }
    if (bad)
        flag_batch(p, GNNB_FLAG_EDGE);
}

// 1 / sqrt(1 + d) for the in-degrees the molecule path can meet (<= 64 edges), as correctly rounded fp32 divisions of
// correctly rounded fp32 square roots -- bit-identical to `1.0f / sqrtf(1.0f + d)` on the device and in the oracle (hex
// float literals; generated with numpy float32).  One load instead of the ~35 instructions of the IEEE sqrt + division.
static __device__ const float k_dinv_by_degree[65] = {
    0x1.0000000000000p+0f, 0x1.6a09e60000000p-1f, 0x1.279a740000000p-1f, 0x1.0000000000000p-1f, 0x1.c9f25c0000000p-2f,
    0x1.a20bd60000000p-2f, 0x1.8309200000000p-2f, 0x1.6a09e60000000p-2f, 0x1.5555560000000p-2f, 0x1.43d1360000000p-2f,
    0x1.34bf640000000p-2f, 0x1.279a740000000p-2f, 0x1.1c01aa0000000p-2f, 0x1.11acee0000000p-2f, 0x1.08654a0000000p-2f,
    0x1.0000000000000p-2f, 0x1.f0b6860000000p-3f, 0x1.e2b7e00000000p-3f, 0x1.d5d7ea0000000p-3f, 0x1.c9f25c0000000p-3f,
    0x1.bee9040000000p-3f, 0x1.b4a2940000000p-3f, 0x1.ab099a0000000p-3f, 0x1.a20bd60000000p-3f, 0x1.99999a0000000p-3f,
    0x1.91a5560000000p-3f, 0x1.8a23460000000p-3f, 0x1.8309200000000p-3f, 0x1.7c4dd60000000p-3f, 0x1.75e9740000000p-3f,
    0x1.6fd4e80000000p-3f, 0x1.6a09e60000000p-3f, 0x1.6482d40000000p-3f, 0x1.5f3aa80000000p-3f, 0x1.5a2cd80000000p-3f,
    0x1.5555560000000p-3f, 0x1.50b06a0000000p-3f, 0x1.4c3abe0000000p-3f, 0x1.47f1460000000p-3f, 0x1.43d1360000000p-3f,
    0x1.3fd8080000000p-3f, 0x1.3c03660000000p-3f, 0x1.38512c0000000p-3f, 0x1.34bf640000000p-3f, 0x1.314c3e0000000p-3f,
    0x1.2df60c0000000p-3f, 0x1.2abb440000000p-3f, 0x1.279a740000000p-3f, 0x1.24924a0000000p-3f, 0x1.21a1860000000p-3f,
    0x1.1ec7020000000p-3f, 0x1.1c01aa0000000p-3f, 0x1.19507e0000000p-3f, 0x1.16b2900000000p-3f, 0x1.1426fc0000000p-3f,
    0x1.11acee0000000p-3f, 0x1.0f43a40000000p-3f, 0x1.0cea620000000p-3f, 0x1.0aa07c0000000p-3f, 0x1.08654a0000000p-3f,
    0x1.0638320000000p-3f, 0x1.0418a40000000p-3f, 0x1.0206140000000p-3f, 0x1.0000000000000p-3f, 0x1.fc0bd80000000p-4f};

// What a wave that prepares SEVERAL graphs fetched for one of them up front (prep_graph_group below): the graph's five table
// entries and, when its clamped edge range holds <= 64 edges, lane l's edge.  nullptr = the graph's wave fetches for itself.
struct PrepFetched {
    int np_m1, np_0, np_p1; // node_ptr[g - 1] (0 for g == 0), node_ptr[g], node_ptr[g + 1]
    int ep_0, ep_p1;        // edge_ptr[g], edge_ptr[g + 1]
    bool has_edge;          // `edge` is coo[e0 + lane] for lane < ne (e0, ne: the clamped range, as prep_one_graph forms it)
    int2 edge;
};

// ---- molecule path: n <= 64 and ne <= 64 (QM9, ESOL, most of ogbg-molhiv) -----------------------------------------------
// One lane per edge, one lane per node.  Written for INSTRUCTION COUNT: with batches in flight this code runs beside the
// conv-stack kernel of another batch and costs the pipeline what it issues.  Instead of one ballot per destination
// node (a loop of n iterations of ~12 vector + scalar instructions), the lanes are matched on the BITS of the destination
// index: ceil(log2 n) ballots give every edge lane the mask of the lanes with the same destination (rank among them =
// popcount below the lane: stable, lanes are in COO order) and, from the same ballots, every NODE lane the mask of its
// in-edges (degree = popcount).
__device__ __forceinline__ void prep_graph_small(const PrepParams &p, const GraphRange r, int lane, int32_t *s_first_w, const PrepFetched *pre)
{
    const int n0 = r.n0, e0 = r.e0;
    const int n = r.n1 - r.n0, ne = r.e1 - r.e0;
    // ---- this lane's edge
    int src = n0, d = 0;
    bool keep = false, bad = false;
    if (lane < ne) {
        const int2 e = (pre && pre->has_edge) ? pre->edge : p.coo[e0 + lane];
        if (accept_edge(p, r, e, bad)) {
            keep = true;
            src = e.x;
            d = e.y - n0;
        }
    }
    // ---- match on the bits of the destination: `same` = edge lanes with this lane's destination, `mine` = edge lanes
    // whose destination is THIS lane's node index
    const unsigned long long valid = __ballot(keep);
    unsigned long long same = valid, mine = valid;
    const int nbits = 32 - __builtin_clz(max(n - 1, 1)); // wave-uniform, <= 6
    for (int b = 0; b < nbits; b++) {
        const unsigned long long mb = __ballot(keep && ((d >> b) & 1));
        same &= ((d >> b) & 1) ? mb : ~mb;
        mine &= ((lane >> b) & 1) ? mb : ~mb;
    }
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0));
    const int deg = lane < n ? __popcll(mine) : 0;
    // ---- row starts: inclusive wave scan of the degrees over the node lanes
    const int incl = wave_scan_incl(deg);
    const int start = e0 + incl - deg;
    if (lane < n) {
        const int v = n0 + lane;
        p.row_ptr[v] = start;
        p.dinv[v] = k_dinv_by_degree[min(deg, 64)];
        store_degree_scalers(p, v, deg);
        default_first_sources(s_first_w, lane, v);
    }
    wave_handover();
    // ---- scatter: col[start[dst] + rank] = src (one store per edge lane), first four sources -> the node's record
    const int st = __shfl(start, d, 64);
    if (keep) {
        p.col[st + rank] = src;
        p.eid[st + rank] = e0 + lane; // COO row of this CSR slot (gnn_builder_lib.h:1126-1166)
        if (rank < 4)
            s_first_w[d * 4 + rank] = src;
    }
    wave_handover();
    if (lane < n)
        store_node_record(p, n0 + lane, start, deg, *reinterpret_cast<const int4 *>(s_first_w + lane * 4));
    if (bad)
        flag_batch(p, GNNB_FLAG_EDGE);
}

// ---- register path: n <= PREP_FAST_NODES and ne <= PREP_FAST_EDGES, but not both <= 64 ------------------------------------
// Lanes hold EDGES (lane l: edge 64c + l of chunk c, in registers).  One loop over the graph's destination nodes:
// ballot(dst == v) gives, in a single instruction, the in-degree of v (popcount) and the rank of every edge among v's in-edges
// (popcount of the lower lanes) -- stable, because lanes are in COO order.  Starts come from a wave prefix sum over node lanes,
// and `col` is then written by ONE scatter per 64 edges instead of a divergent store per edge: n iterations of ~8 instructions
// per edge chunk replace the scan path's 2 ne iterations of a dependent chain.
template <int PREP_FAST_NODES>
__device__ __forceinline__ void prep_graph_ballot(const PrepParams &p, const GraphRange r, int lane, int32_t *s_first_w)
{
    const int n0 = r.n0, e0 = r.e0;
    const int n = r.n1 - r.n0, ne = r.e1 - r.e0;
    // ---- edges -> registers; a dropped edge keeps dst = -1, which never matches
    constexpr int EC = PREP_FAST_EDGES / 64, NC = PREP_FAST_NODES / 64;
    int es[EC], ed[EC], erank[EC];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < EC; c++) {
        es[c] = n0;
        ed[c] = -1;
        erank[c] = 0;
        const int i = c * 64 + lane;
        if (i < ne) {
            const int2 e = p.coo[e0 + i];
            if (accept_edge(p, r, e, bad)) {
                es[c] = e.x;
                ed[c] = e.y - n0; // local destination
            }
        }
    }
    GNNB_STAMP(1);
    // ---- one pass over destination nodes: degree of node v -> node lane (v & 63) of chunk v >> 6;
    // rank of each matching edge among v's in-edges -> that edge's lane
    int deg[NC];
#pragma unroll
    for (int q = 0; q < NC; q++)
        deg[q] = 0;
    const int nec = (ne + 63) >> 6;
    for (int v = 0; v < n; v++) {
        int before = 0; // in-edges of v in earlier edge chunks
#pragma unroll
        for (int c = 0; c < EC; c++) {
            if (c < nec) {
                const unsigned long long m = __ballot(ed[c] == v);
                if (ed[c] == v)
                    erank[c] = before + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                before += __popcll(m);
            }
        }
#pragma unroll
        for (int q = 0; q < NC; q++)
            if ((v >> 6) == q && lane == (v & 63))
                deg[q] = before;
    }
    GNNB_STAMP(2);
    // ---- row starts: wave prefix sum over node lanes, chunk by chunk
    int start[NC];
    int base = e0;
#pragma unroll
    for (int q = 0; q < NC; q++) {
        start[q] = 0;
        if (q * 64 < n) {
            const int incl = wave_scan_incl(deg[q]);
            start[q] = base + incl - deg[q];
            base += __shfl(incl, 63, 64);
            const int vl = q * 64 + lane;
            if (vl < n) {
                const int v = n0 + vl;
                p.row_ptr[v] = start[q];
                p.dinv[v] = 1.0f / sqrtf(1.0f + (float)deg[q]);
                store_degree_scalers(p, v, deg[q]);
                default_first_sources(s_first_w, vl, v);
            }
        }
    }
    wave_handover();
    // ---- scatter: col[start[dst] + rank] = src, one store instruction per 64 edges
#pragma unroll
    for (int c = 0; c < EC; c++) {
        if (c < nec) { // wave-uniform: the cross-lane reads below run with every lane active
            const int d = ed[c] < 0 ? 0 : ed[c];
            int st = 0;
#pragma unroll
            for (int q = 0; q < NC; q++) {
                const int t = __shfl(start[q], d & 63, 64);
                if ((d >> 6) == q)
                    st = t;
            }
            if (ed[c] >= 0) {
                p.col[st + erank[c]] = es[c];
                p.eid[st + erank[c]] = e0 + c * 64 + lane; // COO row of this CSR slot (gnn_builder_lib.h:1126-1166)
                if (erank[c] < 4)
                    s_first_w[d * 4 + erank[c]] = es[c];
            }
        }
    }
    wave_handover();
#pragma unroll
    for (int q = 0; q < NC; q++) {
        const int vl = q * 64 + lane;
        if (vl < n)
            store_node_record(p, n0 + vl, start[q], deg[q], *reinterpret_cast<const int4 *>(s_first_w + vl * 4));
    }
    if (bad)
        flag_batch(p, GNNB_FLAG_EDGE);
}

// One graph (g < B), or the batch's tail (g == B: the end entries of the tables, the rows no graph owns), by one wavefront.
// s_first_w: prep_wave_lds_ints(PREP_FAST_NODES) ints of LDS owned by this wave.
// PREP_FAST_NODES: 256 (4 node chunks of 64 lanes) in general, 64 when the caller promises graphs of <= 64
// nodes -- 4 KB of LDS per workgroup instead of 16 KB, so that graph prep of the next batch fits on a CU
// beside two workgroups of the conv-stack kernel and the readout of the previous one.
// pre: g < B only -- the batch's tail reads entries 0 and B
template <int PREP_FAST_NODES>
__device__ __forceinline__ void prep_one_graph(const PrepParams &p, int g, int lane, int32_t *s_first_w, const PrepFetched *pre = nullptr)
{
    const int B = p.B, N = p.N, E = p.E;
    auto np_at = [&](int k) { return pre ? (k < g ? pre->np_m1 : (k == g ? pre->np_0 : pre->np_p1)) : p.node_ptr[k]; };
    auto ep_at = [&](int k) { return pre ? (k == g ? pre->ep_0 : pre->ep_p1) : p.edge_ptr[k]; };

    // ---- node tiles: tile_first[t] = min{ node_ptr[g'] : node_ptr[g'] >= t*tile_rows }
    {
        // clamped so that a malformed node_ptr (flagged below) cannot write out of range
        const int np = (g == B) ? N : min(max(np_at(g), 0), N);
        const int t_lo = (g == 0) ? 0 : max(min(max(np_at(g - 1), 0), N) / p.tile_rows + 1, 0);
        const int t_hi = (g == B) ? p.num_tiles : min(np / p.tile_rows, p.num_tiles);
        // edges are grouped by graph, so the CSR segment of graph g starts at edge_ptr[g]
        const int pe = (g == B) ? E : min(max(ep_at(g), 0), E);
        for (int t = t_lo + lane; t <= t_hi; t += 64) {
            p.tile_first[t] = np;
            p.tile_edge[t] = pe;
            p.tile_graph[t] = g;
        }
        if (lane == 0)
            p.graph_ptr[g] = np; // the clamped copy later kernels read
    }
    // The caller's large segment (gnnb_workspace_set_large_segment) names its first graph AND that graph's node / edge
    // offsets; the stack kernels run on rows [0, large_n) and the layer-wise half on the rest.  A triple that disagrees
    // with the ptr arrays of THIS batch (stale workspace state from the batch before) would leave the rows between the two
    // boundaries to neither half: flagged here, where both arrays are read anyway.
    if (p.large_n >= 0 && g == p.promise_graphs && lane == 0 && (np_at(g) != p.large_n || ep_at(g) != p.large_e))
        flag_batch(p, GNNB_FLAG_LARGE_SEGMENT);
    // Containment of malformed batches: whatever node_ptr / edge_ptr hold, every row in [0, N) leaves this
    // kernel with a record that later kernels can follow without leaving the buffers -- start and start + deg
    // inside [0, E], sources inside [0, N).  A graph's ranges are CLAMPED instead of rejected (any row r < N lies
    // in some pair node_ptr[g] <= r < node_ptr[g+1] when node_ptr runs from 0 to N; rows before node_ptr[0] or
    // after node_ptr[B] are given empty records by the last wave), only edges inside the clamped node range are
    // accepted, and the results of a flagged batch are unspecified but in range.
    if (g == B) {
        const int first = p.node_ptr[0], last = p.node_ptr[B];
        if (lane == 0) {
            if (p.agg_cut)
                p.agg_cut[1 << p.cut_log2] = make_int4(N, N, E, B); // (the end of the last range)
            p.row_ptr[N] = E;
            if (last != N || p.edge_ptr[B] != E || first != 0 || p.edge_ptr[0] != 0)
                flag_batch(p, GNNB_FLAG_PTR_ENDS);
        }
        if (first > 0)
            prep_empty_rows(p, 0, min(first, N), lane);
        if (last < N)
            prep_empty_rows(p, max(last, 0), N, lane);
        return;
    }

    GNNB_STAMP(0);
    GraphRange r{np_at(g), np_at(g + 1), ep_at(g), ep_at(g + 1)};
    if (r.n0 > r.n1 || r.e0 > r.e1 || r.n1 > N || r.e1 > E || r.n0 < 0 || r.e0 < 0) {
        if (lane == 0)
            flag_batch(p, GNNB_FLAG_PTR_ORDER);
        r.n0 = min(max(r.n0, 0), N);
        r.n1 = min(max(r.n1, 0), N);
        r.e0 = min(max(r.e0, 0), E);
        r.e1 = min(max(r.e1, 0), E);
        if (r.n0 >= r.n1)
            return; // covers no row
        if (r.e0 > r.e1)
            r.e1 = r.e0; // no usable edge range: the rows get empty records
    }
    const int n = r.n1 - r.n0, ne = r.e1 - r.e0;
    if (p.node_graph) // (the pooling epilogue of the last layer's GEMM walks rows by graph id: launch_linear, PoolEpilogue)
        for (int v = r.n0 + lane; v < r.n1; v += 64)
            p.node_graph[v] = g;
    // Row-balanced ranges of the gather-aggregate workgroups (k_aggregate_ring): range b of 2^cut_log2 starts at row
    // floor(b N / 2^cut_log2), usually in the middle of a graph -- the wave of the graph that owns that row records the
    // graph's first row / CSR slot beside it (both neighbours stage the boundary graph, each reduces its own rows).  No
    // search: lane l tests candidate b_est - 1 + l around a float estimate, exactly.
    if (p.agg_cut) {
        int bb = (int)((float)r.n0 * (float)(1 << p.cut_log2) / (float)max(N, 1)) - 2; // (wave-uniform)
        do { // (one pass for any graph of less than ~60 ranges' worth of rows)
            const int b = bb + lane;
            if (b >= 0 && b < (1 << p.cut_log2)) {
                const int row = (int)(((long long)b * N) >> p.cut_log2);
                if (row >= r.n0 && row < r.n1)
                    p.agg_cut[b] = make_int4(row, r.n0, r.e0, g);
            }
            bb += 64;
        } while (bb < (1 << p.cut_log2) && (int)(((long long)max(bb, 0) * N) >> p.cut_log2) < r.n1);
    }
    if (p.max_graph_nodes_hint > 0 && n > p.max_graph_nodes_hint && g < p.promise_graphs && lane == 0)
        flag_batch(p, GNNB_FLAG_GRAPH_NODES); // the caller's max_graph_nodes promise does not hold for this batch
    // (all three conditions are wave-uniform)
    if (n > PREP_FAST_NODES || ne > PREP_FAST_EDGES)
        prep_graph_scan(p, r, lane);
    else if (n <= 64 && ne <= 64) {
        prep_graph_small(p, r, lane, s_first_w, pre);
        GNNB_STAMP_END(3);
    } else {
        prep_graph_ballot<PREP_FAST_NODES>(p, r, lane, s_first_w);
        GNNB_STAMP_END(3);
    }
}

// a kernel's FIRST argument where it lies in the kernarg segment: a PrepParams that only some of the kernel's workgroups read (k_head_small)
__device__ __forceinline__ const PrepParams *kernarg_prep_params()
{
    return (const PrepParams *)__builtin_amdgcn_kernarg_segment_ptr(); // (constant address space -> generic: the loads stay scalar)
}

// G consecutive graphs g0 .. g0 + G - 1 (those <= B) by ONE wavefront, their fetches batched.  The prep of a graph is a
// chain of dependent round trips -- its table entries, then its edges, then a few hundred instructions and the stores -- that
// occupies a wave slot for ~6 us and the machine hardly at all.  Beside the stack kernel of another batch there is ONE wave slot
// per SIMD for every guest kernel (k_gcn2_zf: four waves of <= 104 registers per SIMD leave 96): at BASELINE config 2 (4096
// graphs) one graph per wave made the prep 1025 workgroups x ~6 us = 24 us of ALL 256 guest slots per step, the readout's 11 us
// on top, against a 37.5-us step -- the guests queued and the pipeline ran at 42 us per step.  Here every lane-parallel load
// serves the whole group (lane l: entry g0 - 1 + l of node_ptr, g0 + l of edge_ptr), then the G edge loads are in flight
// together: two round trips per G graphs instead of 2 G, a quarter of the workgroups at G = 4.
template <int PREP_FAST_NODES, int G>
__device__ __forceinline__ void prep_graph_group(const PrepParams &p, int g0, int lane, int32_t *s_first_w)
{
    static_assert(G >= 1 && G <= 16, "group size");
    if (g0 > p.B)
        return;
    // entries g0 - 1 .. g0 + G of node_ptr (lanes 0 .. G + 1) and g0 .. g0 + G of edge_ptr (lanes 0 .. G), clamped to [0, B]
    const int npv = p.node_ptr[min(max(g0 - 1 + lane, 0), p.B)];
    const int epv = p.edge_ptr[min(g0 + lane, p.B)];
    PrepFetched f[G];
#pragma unroll
    for (int k = 0; k < G; k++) {
        f[k].np_m1 = __builtin_amdgcn_readlane(npv, k);
        f[k].np_0 = __builtin_amdgcn_readlane(npv, k + 1);
        f[k].np_p1 = __builtin_amdgcn_readlane(npv, k + 2);
        f[k].ep_0 = __builtin_amdgcn_readlane(epv, k);
        f[k].ep_p1 = __builtin_amdgcn_readlane(epv, k + 1);
        // the clamped edge range, exactly as prep_one_graph forms it (a malformed range is flagged there)
        const int e0 = min(max(f[k].ep_0, 0), p.E);
        const int ne = max(min(max(f[k].ep_p1, 0), p.E) - e0, 0);
        f[k].has_edge = g0 + k < p.B && ne <= 64; // (wave-uniform)
        f[k].edge = make_int2(0, 0);
        if (f[k].has_edge && lane < ne)
            f[k].edge = p.coo[e0 + lane];
    }
#pragma unroll
    for (int k = 0; k < G; k++) {
        const int g = g0 + k;
        if (g < p.B)
            prep_one_graph<PREP_FAST_NODES>(p, g, lane, s_first_w, &f[k]);
        else if (g == p.B)
            prep_one_graph<PREP_FAST_NODES>(p, g, lane, s_first_w);
    }
}

} // namespace gnnb
