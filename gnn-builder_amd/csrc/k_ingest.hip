// k_ingest.hip -- a PyG mini-batch on the device: edge_index [2, E] int64 + batch [N] int64 (or ptr [B+1] int64) -> the
// project's batch layout coo [E, 2] int32 grouped by graph (stable), node_ptr / edge_ptr [B+1] int32 (latency bound); and a
// GINE model's edge attributes carried along (k_edge_attr_order)
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
// What batching.from_pyg_batch does on the host (searchsorted, stable argsort, cumsum) without a device value ever being read
// back: the launch sequence depends on the host integers B, N, E only, so a captured graph replays on any batch of that shape.
//   k_ingest_nodes      node_ptr by boundary detection on `batch` (element i writes node_ptr[g] = i for g in (batch[i-1], batch[i]]),
//                       or the checked narrowing of `ptr`
//   k_ingest_classify   per edge: endpoints validated and narrowed, graph id of the destination (the sort key), coo and -- by
//                       the same boundary detection -- edge_ptr AS IF the keys were already non-decreasing; a key below its
//                       predecessor sets the state word "unsorted"
//   k_ingest_hist / _scan / _scatter   general path, one least-significant-digit radix pass of 8 bits over (key, edge index):
//                       per-tile digit counts, exclusive scan over (digit, tile), in-tile ranks by ballot matching -- stable, and
//                       no rank depends on the order in which an atomic lands (the LDS atomics only count)
//   k_ingest_finish     general path: coo gathered in sorted order, edge_ptr from the sorted keys
// Every kernel behind k_ingest_classify returns at once unless "unsorted" is set: Batch.from_data_list always gives grouped edges.
// Containment of malformed input (flag GNNB_FLAG_INGEST): endpoints are clamped into [0, N), graph ids into [0, B); the keys
// that are sorted are the clamped ones, so edge_ptr is monotone by construction; a broken `batch` / `ptr` gives node_ptr =
// {0, N, ..., N} (every node in graph 0): in range and monotone, the results of a flagged batch are unspecified.
//
// k_edge_attr_order: edge_attr_ord[i] = edge_attr[src(i)], src(i) = i on the ingest's grouped path and idx[i] on its general
// path (the sorted-position -> input-edge array k_ingest_finish consumes); the path is read from the ingest's state word, as
// the ingest's own kernels do: no read-back, the same launch for grouped and shuffled input.
// k_edge_type_order: its twin for an RGCNConv model's integer edge types (gnnb_rgcn.h), int64 in, int32 out, -1 for a value that
// does not fit.
#include <algorithm>

#include "gnnb_device.h"

namespace gnnb {

constexpr int IT = 256;              // threads per workgroup
constexpr int IR = INGEST_TILE / IT; // edges per thread: edge k * IT + t of the tile is thread t's k-th
constexpr int DIGITS = 1 << INGEST_DIGIT_BITS;
static_assert(DIGITS == IT, "one thread per digit in the scatter's prefix step");
static_assert(INGEST_TILE % IT == 0, "whole rounds");

// the validation flag of the workspace (what flag_batch is to graph prep): one lane per wave with something to report
__device__ __forceinline__ void ingest_flag(const IngestParams &p, bool bad)
{
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0)
        report_flag(p.err, p.err_host, GNNB_FLAG_INGEST);
}

// graph of node v in [0, N), always inside [0, B): batch[v] clamped, or the last g with ptr[g] <= v (ptr_search: inside
// ptr[1 .. B - 1] whatever the array holds), or 0 (neither: B == 1)
__device__ __forceinline__ int ingest_graph_of(const IngestParams &p, int v)
{
    if (p.batch)
        return (int)min(max(p.batch[v], 0ll), (long long)(p.B - 1));
    return p.ptr ? ptr_search(p.ptr, p.B, v) : 0;
}

// endpoints of input edge e narrowed into [0, N); true = one of them lay outside (negative, >= N, or beyond 32 bits)
__device__ __forceinline__ bool ingest_endpoints(const IngestParams &p, long long e, int &s, int &d)
{
    const unsigned long long us = (unsigned long long)p.src[e], ud = (unsigned long long)p.dst[e], n = (unsigned long long)p.N;
    s = us < n ? (int)us : 0;
    d = ud < n ? (int)ud : 0;
    return us >= n || ud >= n;
}

// sort key of input edge e: the graph of its destination
__device__ __forceinline__ int ingest_key(const IngestParams &p, long long e)
{
    int s, d;
    (void)ingest_endpoints(p, e, s, d);
    return ingest_graph_of(p, d);
}

// boundary detection: element i of a non-decreasing id sequence (ids in [0, B); virtual ids -1 in front and B behind) opens
// the graphs (prev, cur]
__device__ __forceinline__ void ingest_open_graphs(int32_t *ptr_out, int prev, int cur, int i)
{
    for (int g = prev + 1; g <= cur; g++)
        ptr_out[g] = i;
}

__global__ __launch_bounds__(IT) void k_ingest_nodes(IngestParams p)
{
    const long long i = (long long)blockIdx.x * IT + threadIdx.x;
    if (i == 0)
        p.state[INGEST_STATE_UNSORTED] = 0; // (set by k_ingest_classify, read by the kernels behind it)
    bool bad = false;
    if (p.batch) { // elements 0 .. N, the last one virtual
        if (i <= p.N) {
            auto id_at = [&](long long k) {
                const long long v = p.batch[k];
                bad |= v < 0 || v >= p.B;
                return (int)min(max(v, 0ll), (long long)(p.B - 1));
            };
            const int cur = i == p.N ? p.B : id_at(i);
            const int prev = i == 0 ? -1 : id_at(i - 1);
            bad |= cur < prev;
            ingest_open_graphs(p.node_ptr, prev, cur, (int)i);
        }
    } else if (i <= p.B) { // ptr, or neither (B == 1): entries 0 .. B
        long long v = i == 0 ? 0 : p.N;
        if (p.ptr) {
            v = p.ptr[i];
            bad = v < 0 || v > p.N || (i > 0 && v < p.ptr[i - 1]) || (i == 0 && v != 0) || (i == p.B && v != p.N);
        }
        p.node_ptr[i] = i == 0 ? 0 : i == p.B ? p.N : (int)min(max(v, 0ll), (long long)p.N);
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0)
        atomicOr(&p.state[INGEST_STATE_NODES_BROKEN], 1);
    ingest_flag(p, bad);
}

__global__ __launch_bounds__(IT) void k_ingest_classify(IngestParams p)
{
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0) { // a broken batch / ptr: every node in graph 0 (entries 0 and B are right already)
        const int broken = p.state[INGEST_STATE_NODES_BROKEN];
        __syncthreads();
        if (threadIdx.x == 0)
            p.state[INGEST_STATE_NODES_BROKEN] = 0; // (as the next ingest expects it)
        if (broken)
            for (int g = 1 + threadIdx.x; g < p.B; g += IT)
                p.node_ptr[g] = p.N;
    }
    bool bad = false, unsorted = false;
    const long long base = (long long)blockIdx.x * INGEST_TILE;
    for (int k = 0; k < IR; k++) { // elements 0 .. E, the last one virtual
        const long long e = base + k * IT + threadIdx.x;
        int key = p.B;
        if (e < p.E) {
            int s, d;
            bad |= ingest_endpoints(p, e, s, d);
            key = ingest_graph_of(p, d);
            bad |= ingest_graph_of(p, s) != key; // an edge between two graphs
            p.keys[0][e] = key;
            p.coo[e] = make_int2(s, d);
        }
        int prev = __shfl_up(key, 1, 64);
        if (e <= p.E) {
            if (lane == 0)
                prev = e == 0 ? -1 : ingest_key(p, e - 1);
            unsorted |= key < prev;
            ingest_open_graphs(p.edge_ptr, prev, key, (int)e); // (rewritten by k_ingest_finish when some key was out of order)
        }
    }
    if (__ballot(unsorted) != 0ull && lane == 0)
        atomicOr(&p.state[INGEST_STATE_UNSORTED], 1);
    ingest_flag(p, bad);
}

// ---- general path: the edges' graph ids are not grouped ---------------------------------------------------------------------
// hist[d * nb + b] = edges of tile b whose key has digit d at `shift`
__global__ __launch_bounds__(IT) void k_ingest_hist(IngestParams p, const int32_t *keys, int shift, int nb)
{
    if (!p.state[INGEST_STATE_UNSORTED])
        return;
    __shared__ int s_cnt[DIGITS];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * INGEST_TILE;
    for (int k = 0; k < IR; k++) {
        const long long e = base + k * IT + threadIdx.x;
        if (e < p.E)
            atomicAdd(&s_cnt[(keys[e] >> shift) & (DIGITS - 1)], 1);
    }
    __syncthreads();
    p.hist[(size_t)threadIdx.x * nb + blockIdx.x] = s_cnt[threadIdx.x];
}

// exclusive scan of hist[0 .. n) in place, one workgroup of 16 waves
__global__ __launch_bounds__(1024) void k_ingest_scan(IngestParams p, int n)
{
    if (!p.state[INGEST_STATE_UNSORTED])
        return;
    __shared__ int s_wave[1][16];
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int v[1] = {i < n ? p.hist[i] : 0};
        int excl[1], total[1];
        block_scan_excl<16, 1>(v, excl, total, s_wave);
        if (i < n)
            p.hist[i] = carry + excl[0];
        carry += total[0];
    }
}

// Tile b moves its (key, edge index) pairs to hist[digit * nb + b] + rank among the tile's pairs of that digit.  The rank of
// a pair counts the pairs in front of it in tile order (round, wave, lane): inside a wave by matching the lanes on the eight
// bits of the digit (wave_match; as prep_graph_small does for destinations), across waves and rounds by a prefix over the 16 (round,
// wave) counts of each digit.  idx_in == nullptr: the first pass, a pair's edge index is its position.
__global__ __launch_bounds__(IT) void k_ingest_scatter(IngestParams p, const int32_t *keys_in, const int32_t *idx_in, int32_t *keys_out,
                                                       int32_t *idx_out, int shift, int nb)
{
    if (!p.state[INGEST_STATE_UNSORTED])
        return;
    __shared__ int s_cnt[IR * (IT / 64)][DIGITS];
    const int wave = threadIdx.x >> 6;
    for (int q = 0; q < IR * (IT / 64); q++)
        s_cnt[q][threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * INGEST_TILE;
    int key[IR], rank[IR];
#pragma unroll
    for (int k = 0; k < IR; k++) {
        const long long e = base + k * IT + threadIdx.x;
        const bool keep = e < p.E;
        key[k] = keep ? keys_in[e] : 0;
        const int dig = (key[k] >> shift) & (DIGITS - 1);
        const unsigned long long same = wave_match(keep, dig, INGEST_DIGIT_BITS);
        rank[k] = __builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0));
        if (keep && rank[k] == 0)
            s_cnt[k * (IT / 64) + wave][dig] = __popcll(same);
    }
    __syncthreads();
    {
        int run = p.hist[(size_t)threadIdx.x * nb + blockIdx.x];
        for (int q = 0; q < IR * (IT / 64); q++) {
            const int c = s_cnt[q][threadIdx.x];
            s_cnt[q][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IR; k++) {
        const long long e = base + k * IT + threadIdx.x;
        if (e < p.E) {
            const int pos = s_cnt[k * (IT / 64) + wave][(key[k] >> shift) & (DIGITS - 1)] + rank[k];
            if ((unsigned)pos < (unsigned)p.E) { // (always, with counts and keys from one buffer: containment)
                keys_out[pos] = key[k];
                idx_out[pos] = idx_in ? idx_in[e] : (int)e;
            }
        }
    }
}

// sorted position i takes input edge idx[i]; edge_ptr from the sorted keys
__global__ __launch_bounds__(IT) void k_ingest_finish(IngestParams p, const int32_t *keys, const int32_t *idx)
{
    if (!p.state[INGEST_STATE_UNSORTED])
        return;
    const long long base = (long long)blockIdx.x * INGEST_TILE;
    for (int k = 0; k < IR; k++) { // positions 0 .. E, the last one virtual
        const long long i = base + k * IT + threadIdx.x;
        if (i > p.E)
            continue;
        int key = p.B;
        if (i < p.E) {
            key = min(max(keys[i], 0), p.B - 1);
            int s, d;
            (void)ingest_endpoints(p, min(max(idx[i], 0), p.E - 1), s, d);
            p.coo[i] = make_int2(s, d);
        }
        const int prev = i == 0 ? -1 : min(max(keys[i - 1], 0), p.B - 1);
        ingest_open_graphs(p.edge_ptr, prev, key, (int)i);
    }
}

int ingest_sort_passes(int num_graphs)
{
    int passes = 0;
    for (long long covered = 1; covered < num_graphs; covered <<= INGEST_DIGIT_BITS)
        passes++;
    return passes;
}

size_t ingest_place(char *blob, int max_graphs, int max_nodes, int max_edges, IngestParams &p)
{
    (void)max_nodes; // (no array of the ingest has one entry per node)
    const size_t B = (size_t)std::max(max_graphs, 0), E = (size_t)std::max(max_edges, 1), nb = (E + INGEST_TILE - 1) / INGEST_TILE;
    Arena a{blob};
    p.state = a.take<int32_t>(INGEST_STATE_WORDS); // (first: the words enable_ingest zeroes)
    p.node_ptr = a.take<int32_t>(B + 1);
    p.edge_ptr = a.take<int32_t>(B + 1);
    p.coo = a.take<int2>(E);
    for (int h = 0; h < 2; h++) {
        p.keys[h] = a.take<int32_t>(E);
        p.idx[h] = a.take<int32_t>(E);
    }
    p.hist = a.take<int32_t>(nb * DIGITS);
    return a.off;
}

hipError_t launch_ingest(const IngestParams &p, hipStream_t s)
{
    if (p.B <= 0) { // an empty batch: both ptr arrays are {0}
        (void)hipMemsetAsync(p.node_ptr, 0, 4, s);
        (void)hipMemsetAsync(p.edge_ptr, 0, 4, s);
        return hipGetLastError();
    }
    const long long node_elems = (p.batch ? (long long)p.N : (long long)p.B) + 1;
    const unsigned tiles_incl = (unsigned)(((long long)p.E + 1 + INGEST_TILE - 1) / INGEST_TILE); // elements 0 .. E
    hipLaunchKernelGGL(k_ingest_nodes, dim3((unsigned)((node_elems + IT - 1) / IT)), dim3(IT), 0, s, p);
    hipLaunchKernelGGL(k_ingest_classify, dim3(tiles_incl), dim3(IT), 0, s, p);
    const int passes = ingest_sort_passes(p.B);
    if (passes == 0 || p.E < 2) // one graph, or one edge: nothing can be out of order
        return hipGetLastError();
    const int nb = (p.E + INGEST_TILE - 1) / INGEST_TILE;
    int from = 0;
    for (int pass = 0; pass < passes; pass++, from ^= 1) {
        const int shift = pass * INGEST_DIGIT_BITS;
        // (pass 0 reads the keys k_ingest_classify wrote into half 0 and numbers the edges itself)
        hipLaunchKernelGGL(k_ingest_hist, dim3(nb), dim3(IT), 0, s, p, (const int32_t *)p.keys[from], shift, nb);
        hipLaunchKernelGGL(k_ingest_scan, dim3(1), dim3(1024), 0, s, p, nb * DIGITS);
        hipLaunchKernelGGL(k_ingest_scatter, dim3(nb), dim3(IT), 0, s, p, (const int32_t *)p.keys[from],
                           pass == 0 ? (const int32_t *)nullptr : (const int32_t *)p.idx[from], p.keys[from ^ 1], p.idx[from ^ 1], shift, nb);
    }
    hipLaunchKernelGGL(k_ingest_finish, dim3(tiles_incl), dim3(IT), 0, s, p, (const int32_t *)p.keys[from], (const int32_t *)p.idx[from]);
    return hipGetLastError();
}

// ---- the PyG ingest's edge attributes in COO row order ---------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_edge_attr_order(const float *__restrict__ edge_attr, const int32_t *__restrict__ idx,
                                                        const int32_t *__restrict__ state, float *__restrict__ out, int E, int ED)
{
    const long long i = (long long)blockIdx.x * WG + threadIdx.x; // one attribute value per thread
    if (i >= (long long)E * ED)
        return;
    const int row = (int)(i / ED), d = (int)(i - (long long)row * ED);
    // (idx is a permutation of the input edges by construction; clamped all the same, as k_ingest_finish clamps it)
    const int src = (idx && state[INGEST_STATE_UNSORTED]) ? min(max(idx[row], 0), E - 1) : row;
    out[i] = edge_attr[(size_t)src * ED + d];
}

hipError_t launch_edge_attr_order(const float *edge_attr, const int32_t *idx, const int32_t *state, float *out, int num_edges, int edge_dim,
                                  hipStream_t s)
{
    if (num_edges <= 0 || edge_dim <= 0)
        return hipSuccess;
    const long long n = (long long)num_edges * edge_dim;
    hipLaunchKernelGGL(k_edge_attr_order, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, s, edge_attr, idx, state, out, num_edges, edge_dim);
    return hipGetLastError();
}

// ---- ... and its edge types (gnnb_rgcn.h): int64 in, int32 out; a value that does not fit the int32 becomes -1, which k_rgcn_slots
// flags as any type outside [0, relations)
__global__ __launch_bounds__(WG) void k_edge_type_order(const long long *__restrict__ edge_type, const int32_t *__restrict__ idx,
                                                        const int32_t *__restrict__ state, int32_t *__restrict__ out, int E)
{
    const int i = blockIdx.x * WG + threadIdx.x; // one edge per thread
    if (i >= E)
        return;
    const int src = (idx && state[INGEST_STATE_UNSORTED]) ? min(max(idx[i], 0), E - 1) : i;
    const long long v = edge_type[src];
    out[i] = (v < 0 || v > 0x7fffffffll) ? -1 : (int32_t)v;
}

hipError_t launch_edge_type_order(const long long *edge_type, const int32_t *idx, const int32_t *state, int32_t *out, int num_edges, hipStream_t s)
{
    if (num_edges <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_edge_type_order, dim3((unsigned)((num_edges + WG - 1) / WG)), dim3(WG), 0, s, edge_type, idx, state, out, num_edges);
    return hipGetLastError();
}

} // namespace gnnb
