// k_order.hip -- the ingested batch (k_ingest.hip: coo grouped by graph, node_ptr / edge_ptr) with its oversized graphs LAST: the
// layout gnnb_workspace_set_large_segment asks for, on the device (latency bound)
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
// What batching.order_large_last does on the host (flatnonzero, cumsum, two gathers).  A graph is large when it has more than
// `limit` nodes; small graphs come first, large graphs last, both groups in input order.
//   k_order_graphs   one workgroup, two carried scans over the B graphs (count, nodes, edges of the SMALL group; the large
//                    group's running totals are the differences to i, node_ptr[i], edge_ptr[i]): perm, the new ptr arrays, per
//                    input graph its node / edge shift, and the triple (first large graph, its node row, its edge row) into
//                    a host-mapped block -- the three integers the large segment's launches are sized by
//   k_order_rows     x_ord[v + node_shift[graph of v]] = x[v]: 16-byte pieces where width and pointers allow, floats otherwise
//   k_order_edges    coo_ord[e + edge_shift[g]] = coo[e] + node_shift[g], g found in edge_ptr: the order inside a graph is kept
//   k_order_out      out[perm[i]] = out_ord[i]: the forward's rows back in the caller's graph order
// Containment: for a batch the ingest has flagged node_ptr / edge_ptr are still monotone from 0 to N / E and every coo entry is
// in [0, N).  Under exactly that every index formed here stays inside its array: a new offset is a sum of sizes of other graphs
// (<= N, <= E); the graph of a node taken from `batch` is used only if node_ptr agrees that the node lies in it; a renumbered
// endpoint is clamped into [0, N) (an edge that leaves its graph -- flagged -- could otherwise leave the batch).
#include <algorithm>
#include <type_traits>

#include "gnnb_device.h"

namespace gnnb {

constexpr int OG = 1024; // threads of k_order_graphs: one workgroup of 16 waves
constexpr int OT = 256;  // threads per workgroup of the other three (grid-stride copies: capped_grid)

struct Tri { // graphs, nodes, edges
    int c, n, e;
};
__device__ __forceinline__ Tri operator+(Tri a, Tri b) { return Tri{a.c + b.c, a.n + b.n, a.e + b.e}; }

// exclusive prefix of `v` over the workgroup's OG threads, and the workgroup's total: the three components in one block_scan_excl
__device__ __forceinline__ Tri order_block_scan(Tri v, Tri &total, int (*s_wave)[OG / 64])
{
    const int in[3] = {v.c, v.n, v.e};
    int excl[3], tot[3];
    block_scan_excl<OG / 64, 3>(in, excl, tot, s_wave);
    total = Tri{tot[0], tot[1], tot[2]};
    return Tri{excl[0], excl[1], excl[2]};
}

// graph i < B as a term of the small group's sums ({0, 0, 0} for a large one)
__device__ __forceinline__ Tri order_small_term(const OrderParams &p, int i, bool &small)
{
    const int n = p.node_ptr[i + 1] - p.node_ptr[i], e = p.edge_ptr[i + 1] - p.edge_ptr[i];
    small = !(p.limit > 0 && n > p.limit);
    return small ? Tri{1, n, e} : Tri{0, 0, 0};
}

__global__ __launch_bounds__(OG) void k_order_graphs(OrderParams p)
{
    __shared__ int s_wave[3][OG / 64];
    Tri all_small = {0, 0, 0}; // the small group as a whole: where the large group starts
    for (int base = 0; base < p.B; base += OG) {
        const int i = base + threadIdx.x;
        bool small = false;
        const Tri v = i < p.B ? order_small_term(p, i, small) : Tri{0, 0, 0};
        Tri total;
        (void)order_block_scan(v, total, s_wave);
        all_small = all_small + total;
    }
    Tri carry = {0, 0, 0};
    for (int base = 0; base < p.B; base += OG) {
        const int i = base + threadIdx.x;
        bool small = false;
        const Tri v = i < p.B ? order_small_term(p, i, small) : Tri{0, 0, 0};
        Tri total;
        const Tri excl = order_block_scan(v, total, s_wave);
        if (i < p.B) {
            const Tri sb = carry + excl; // the small graphs in front of graph i; the large ones in front of it are the rest
            const int n0 = p.node_ptr[i], e0 = p.edge_ptr[i];
            const int pos = small ? sb.c : all_small.c + (i - sb.c);
            const int noff = small ? sb.n : all_small.n + (n0 - sb.n);
            const int eoff = small ? sb.e : all_small.e + (e0 - sb.e);
            p.perm[pos] = i;
            p.node_ptr_ord[pos] = noff;
            p.edge_ptr_ord[pos] = eoff;
            p.node_shift[i] = noff - n0;
            p.edge_shift[i] = eoff - e0;
        }
        carry = carry + total;
    }
    if (threadIdx.x == 0) {
        p.node_ptr_ord[p.B] = p.N;
        p.edge_ptr_ord[p.B] = p.E;
        // (nothing large: all_small = (B, N, E), as order_large_last returns it)
        __hip_atomic_store(&p.triple[0], all_small.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&p.triple[1], all_small.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&p.triple[2], all_small.e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// graph of node v in [0, N): batch[v] where node_ptr agrees (always, on a well-formed batch), otherwise the search (ptr_search)
__device__ __forceinline__ int order_graph_of_node(const OrderParams &p, int v)
{
    if (p.batch) {
        const int g = (int)min(max(p.batch[v], 0ll), (long long)(p.B - 1));
        if (p.node_ptr[g] <= v && v < p.node_ptr[g + 1])
            return g;
    }
    return ptr_search(p.node_ptr, p.B, v);
}

// V floats per piece (4: a row is in_dim / 4 float4, both matrices 16-byte aligned); 64-bit indices: N * in_dim may pass 2^31
template <int V> __global__ __launch_bounds__(OT) void k_order_rows(OrderParams p)
{
    using T = typename std::conditional<V == 4, float4, float>::type;
    const long long q = p.in_dim / V, total = (long long)p.N * q;
    const T *src = (const T *)p.x;
    T *dst = (T *)p.x_ord;
    for (long long i = (long long)blockIdx.x * OT + threadIdx.x; i < total; i += (long long)gridDim.x * OT) {
        const int v = (int)(i / q);
        dst[i + (long long)p.node_shift[order_graph_of_node(p, v)] * q] = src[i];
    }
}

__global__ __launch_bounds__(OT) void k_order_edges(OrderParams p)
{
    for (long long e = (long long)blockIdx.x * OT + threadIdx.x; e < p.E; e += (long long)gridDim.x * OT) {
        const int g = ptr_search(p.edge_ptr, p.B, (int)e);
        const long long ns = p.node_shift[g], hi = p.N - 1;
        const int2 c = p.coo[e];
        p.coo_ord[e + p.edge_shift[g]] = make_int2((int)min(max(c.x + ns, 0ll), hi), (int)min(max(c.y + ns, 0ll), hi));
    }
}

__global__ __launch_bounds__(OT) void k_order_out(const float *out_ord, const int32_t *perm, float *out, int B, int width)
{
    const long long total = (long long)B * width;
    for (long long i = (long long)blockIdx.x * OT + threadIdx.x; i < total; i += (long long)gridDim.x * OT) {
        const long long row = i / width;
        out[(long long)perm[row] * width + (i - row * width)] = out_ord[i];
    }
}

size_t order_place(char *blob, int max_graphs, int max_nodes, int max_edges, int in_dim, int mlp_out, OrderParams &p)
{
    const size_t B = (size_t)std::max(max_graphs, 0), N = (size_t)std::max(max_nodes, 0), E = (size_t)std::max(max_edges, 1);
    Arena a{blob};
    p.x_ord = a.take<float>(N * (size_t)std::max(in_dim, 0));
    p.coo_ord = a.take<int2>(E);
    p.node_ptr_ord = a.take<int32_t>(B + 1);
    p.edge_ptr_ord = a.take<int32_t>(B + 1);
    p.perm = a.take<int32_t>(B);
    p.node_shift = a.take<int32_t>(B);
    p.edge_shift = a.take<int32_t>(B);
    p.out_ord = a.take<float>(B * (size_t)std::max(mlp_out, 0));
    return a.off;
}

hipError_t launch_order(const OrderParams &p, hipStream_t s)
{
    hipLaunchKernelGGL(k_order_graphs, dim3(1), dim3(OG), 0, s, p);
    const long long floats = (long long)p.N * p.in_dim;
    if (floats > 0) {
        if (p.in_dim % 4 == 0 && (((uintptr_t)p.x | (uintptr_t)p.x_ord) & 15) == 0)
            hipLaunchKernelGGL(k_order_rows<4>, dim3(capped_grid(floats / 4, OT)), dim3(OT), 0, s, p);
        else
            hipLaunchKernelGGL(k_order_rows<1>, dim3(capped_grid(floats, OT)), dim3(OT), 0, s, p);
    }
    if (p.E > 0)
        hipLaunchKernelGGL(k_order_edges, dim3(capped_grid(p.E, OT)), dim3(OT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_order_out(const float *out_ord, const int32_t *perm, float *out, int num_graphs, int width, hipStream_t s)
{
    const long long total = (long long)num_graphs * width;
    if (total > 0)
        hipLaunchKernelGGL(k_order_out, dim3(capped_grid(total, OT)), dim3(OT), 0, s, out_ord, perm, out, num_graphs, width);
    return hipGetLastError();
}

} // namespace gnnb
