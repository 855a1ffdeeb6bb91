// k_gine.hip -- GINE with the edge projection inside the aggregate (gnnb_edge.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_gine_aggregate (reference gine_conv_agg + the self term of gine_conv, gnn_builder_lib.h:1555-1742):
//   out_i = (1 + eps) x_i + sum_{j -> i} relu(x_j + p_e),   p_e = W_e e_ij + b_e,   e_ij = edge_attr[eid[slot]]  (COO row order)
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid).  k_aggregate_edges (k_aggregate.hip) reads p_e as an
// [E, width] matrix a GEMM wrote; here p_e is formed per lane from the edge's edge_dim <= 16 attributes and never reaches HBM.
//
// Work split.  A lane group of G = 2^glog2 lanes (the smallest power of two that covers the row's width / VEC vectors, at most a wave)
// owns a destination row; a lane owns VEC consecutive columns of it (16-byte accesses when width % 4 == 0 and x / out are aligned,
// scalar accesses otherwise -- a model's first layer runs at in_dim = 9, 11, ...: the scalar form is no corner case).  Rows wider
// than 64 vectors are walked in column passes.  The grid is a few workgroups per CU and every lane group walks its rows with a
// grid stride, so that what a lane holds for its columns is loaded once per lane and column pass, not per row or per edge:
//   W_e[c][0 .. edge_dim) and b_e[c] of the lane's VEC columns live in REGISTERS (VEC x edge_dim + VEC values: 20 at VEC 4,
//   edge_dim 4; 68 at edge_dim 16).  A lane's columns never change, so these are loop invariants of the lane; in LDS every edge would
//   cost VEC x edge_dim extra ds_reads per lane, where the fmas that consume them now take register operands.
// The edge's attribute row is read at an address that is the same in every lane of the group: one fetch serves the group.
// GINE_R neighbour rows (x_j and e_ij) are loaded before the first is consumed: up to four rows in flight per lane group, and the
// walk is software-pipelined over three steps (record of row it + 2, slots of row it + 1, rows of row `it`), so that a row of a
// molecule -- in-degree <= 4 -- exposes one memory latency instead of the dependent chain of three.
//
// Summation order (fixed: it depends on the batch, never on the launch shape):
//   p_c   = fma(W_e[c][edge_dim - 1], e[edge_dim - 1], ... fma(W_e[c][0], e[0], b_e[c]))           -- d increasing
//   chunk = a row's CSR slots in pieces of GINE_CHUNK = 64: a piece's messages are added in slot order, starting from 0
//   row   = the pieces' sums added in piece order, starting from 0 (a row of at most 64 in-edges IS its one piece: plain slot order)
//   out   = row + (1 + eps) x_i                                                                        -- the self term last
// Degree skew.  A row of more than GINE_CHUNK in-edges (a hub) is not walked by its own lane group: the workgroup's lane groups take
// its pieces round-robin, park the piece sums in LDS and the owner adds them in piece order -- the rule above, so a hub of in-degree
// 1200 costs its workgroup 19 pieces over 4 .. 256 lane groups instead of 1200 dependent steps of one.  Long rows are taken in a
// second walk behind the short ones: a workgroup without one pays ONE barrier per column pass.
#include "gnnb_device.h"

namespace gnnb {

constexpr int GINE_CHUNK = 64;      // CSR slots per piece of a row's sum
constexpr int GINE_R = 4;           // neighbour rows in flight per lane group
constexpr int GINE_WG_PER_CU = 8;   // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int GINE_MAX_EDGE_DIM = 16;

template <int VEC>
__device__ __forceinline__ void gine_store_vec(float *p, const float (&v)[VEC])
{
    if constexpr (VEC == 4)
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *p = v[0];
}

// relu(x_j + W_e e + b_e) of the first n of GINE_R loaded neighbours, added to acc in their order
template <int VEC, int ED>
__device__ __forceinline__ void gine_add_messages(const float (&xj)[GINE_R][VEC], const float (&e)[GINE_R][ED], int n,
                                                  const float (&wgt)[VEC][ED], const float (&bias)[VEC], float (&acc)[VEC])
{
#pragma unroll
    for (int r = 0; r < GINE_R; r++)
        if (r < n) {
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                float p = bias[v];
#pragma unroll
                for (int d = 0; d < ED; d++)
                    p = fmaf(wgt[v][d], e[r][d], p);
                acc[v] += fmaxf(xj[r][v] + p, 0.0f); // merge_sum_1d, activation_relu, sum_incremental
            }
        }
}

// ... and the first n of those neighbours' x_j (the lane's VEC columns from column fo) and attribute rows
template <int VEC, int ED>
__device__ __forceinline__ void gine_load_messages(const float *__restrict__ x, const float *__restrict__ ea, const int (&j)[GINE_R],
                                                   const int (&ei)[GINE_R], int n, int w, int fo, bool avec, float (&xj)[GINE_R][VEC],
                                                   float (&e)[GINE_R][ED])
{
#pragma unroll
    for (int r = 0; r < GINE_R; r++) {
#pragma unroll
        for (int v = 0; v < VEC; v++)
            xj[r][v] = 0.0f;
#pragma unroll
        for (int d = 0; d < ED; d++)
            e[r][d] = 0.0f;
        if (r < n) {
            row_load_vec<VEC>(x + (size_t)j[r] * w + fo, xj[r]);
            row_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e[r]);
        }
    }
}

// acc += the messages of the CSR slots [k0, k1), in slot order
template <int VEC, int ED>
__device__ __forceinline__ void gine_piece_sum(const float *__restrict__ x, const float *__restrict__ ea, const int32_t *__restrict__ col,
                                               const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int w, int fo, bool avec,
                                               const float (&wgt)[VEC][ED], const float (&bias)[VEC], float (&acc)[VEC])
{
    for (int k = k0; k < k1; k += GINE_R) {
        int j[GINE_R], ei[GINE_R];
        float xj[GINE_R][VEC], e[GINE_R][ED];
        row_load_slots(col, eid, k, k1, N, E, j, ei);
        gine_load_messages<VEC, ED>(x, ea, j, ei, k1 - k, w, fo, avec, xj, e);
        gine_add_messages<VEC, ED>(xj, e, k1 - k, wgt, bias, acc);
    }
}

template <int VEC, int ED>
__global__ __launch_bounds__(WG) void k_gine_aggregate(const float *__restrict__ x, const float *__restrict__ ea, const float *__restrict__ we,
                                                       int ldwe, const float *__restrict__ be, float *__restrict__ out,
                                                       const int4 *__restrict__ node_rec, const int32_t *__restrict__ col,
                                                       const int32_t *__restrict__ eid, int N, int E, int w, int glog2, float eps, int avec,
                                                       int iters)
{
    __shared__ float s_part[WG * VEC]; // piece sums of one round of a long row: [lane group][lane of the group][VEC]
    __shared__ int s_long[WG];         // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const int nvec = w / VEC;
    const float self = 1.0f + eps;
    // step `it` of this lane group: its row and that row's record (node = N, degree 0 past the batch or past the last step)
    auto row_of = [&](int it, int &node, int &rp0, int &deg) {
        node = it < iters ? (it * (int)gridDim.x + (int)blockIdx.x) * groups + grp : N;
        rp0 = 0, deg = 0;
        if (node < N)
            row_record(node_rec, node, E, rp0, deg);
        else
            node = N;
    };
    for (int fb = 0; fb < nvec; fb += G) { // column passes (one, up to 64 vectors per row)
        const bool active = fb + gl < nvec;
        const int fo = active ? (fb + gl) * VEC : 0;
        float wgt[VEC][ED], bias[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            bias[v] = active ? be[fo + v] : 0.0f;
#pragma unroll
            for (int d = 0; d < ED; d++)
                wgt[v][d] = active ? we[(size_t)(fo + v) * ldwe + d] : 0.0f;
        }
        auto finish = [&](int node, const float (&acc)[VEC], const float (&xi)[VEC]) { // the self term last
            float o[VEC];
#pragma unroll
            for (int v = 0; v < VEC; v++)
                o[v] = acc[v] + xi[v] * self;
            gine_store_vec<VEC>(out + (size_t)node * w + fo, o);
        };
        // ---- rows of at most GINE_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
        // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first GINE_R slots of step it + 1
        // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago
        int n0, rp_0, dg_0, n1, rp_1, dg_1;
        int j0[GINE_R], e0[GINE_R];
        row_of(0, n0, rp_0, dg_0);
        row_load_slots(col, eid, rp_0, rp_0 + (dg_0 <= GINE_CHUNK ? dg_0 : 0), N, E, j0, e0);
        row_of(1, n1, rp_1, dg_1);
        bool any_long = false;
        for (int it = 0; it < iters; it++) {
            int n2, rp_2, dg_2, j1[GINE_R], e1[GINE_R];
            row_of(it + 2, n2, rp_2, dg_2);
            row_load_slots(col, eid, rp_1, rp_1 + (dg_1 <= GINE_CHUNK ? dg_1 : 0), N, E, j1, e1);
            any_long |= dg_0 > GINE_CHUNK;
            if (n0 < N && dg_0 <= GINE_CHUNK && active) {
                float xi[VEC], xj[GINE_R][VEC], e[GINE_R][ED], acc[VEC];
                row_load_vec<VEC>(x + (size_t)n0 * w + fo, xi);
                gine_load_messages<VEC, ED>(x, ea, j0, e0, dg_0, w, fo, avec != 0, xj, e);
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[v] = 0.0f;
                gine_add_messages<VEC, ED>(xj, e, dg_0, wgt, bias, acc);
                if (dg_0 > GINE_R)
                    gine_piece_sum<VEC, ED>(x, ea, col, eid, rp_0 + GINE_R, rp_0 + dg_0, N, E, w, fo, avec != 0, wgt, bias, acc);
                finish(n0, acc, xi);
            }
            n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
            n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
            for (int r = 0; r < GINE_R; r++)
                j0[r] = j1[r], e0[r] = e1[r];
        }
        // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met
        // none is done with this column pass after ONE barrier
        if (!__syncthreads_or(any_long))
            continue;
        for (int it = 0; it < iters; it++) {
            int node, rp0, deg;
            row_of(it, node, rp0, deg);
            const bool is_long = deg > GINE_CHUNK;
            if (!__syncthreads_or(is_long))
                continue;
            // the long rows of this step, one after the other: pieces round-robin over the lane groups, sums through LDS
            if (gl == 0)
                s_long[grp] = is_long ? node : -1;
            __syncthreads();
            for (int g = 0; g < groups; g++) {
                const int ln = s_long[g];
                if (ln < 0)
                    continue;
                int lrp, ldeg;
                row_record(node_rec, ln, E, lrp, ldeg);
                const int npieces = (ldeg + GINE_CHUNK - 1) / GINE_CHUNK;
                float acc[VEC];
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[v] = 0.0f;
                for (int c0 = 0; c0 < npieces; c0 += groups) {
                    const int c = c0 + grp;
                    float part[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        part[v] = 0.0f;
                    if (c < npieces && active)
                        gine_piece_sum<VEC, ED>(x, ea, col, eid, lrp + c * GINE_CHUNK, lrp + min((c + 1) * GINE_CHUNK, ldeg), N, E, w, fo,
                                                avec != 0, wgt, bias, part);
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        s_part[threadIdx.x * VEC + v] = part[v];
                    __syncthreads();
                    if (grp == g) {
                        const int nq = min(groups, npieces - c0);
                        for (int q = 0; q < nq; q++)
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                acc[v] += s_part[((q << glog2) + gl) * VEC + v];
                    }
                    __syncthreads();
                }
                if (grp == g && active) {
                    float xi[VEC];
                    row_load_vec<VEC>(x + (size_t)ln * w + fo, xi);
                    finish(ln, acc, xi);
                }
            }
            __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
        }
    }
}

hipError_t launch_gine_aggregate(const BatchTables &t, const float *x, const float *edge_attr, int edge_dim, const float *we, int ldwe,
                                 const float *be, float *out, int width, float eps, hipStream_t s)
{
    if (edge_dim < 1 || edge_dim > GINE_MAX_EDGE_DIM || width < 1 || ldwe < edge_dim)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const bool v4 = (width % 4 == 0) && (((uintptr_t)x & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int avec = (edge_dim % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
    const int nvec = v4 ? width / 4 : width;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int steps = (t.num_nodes + groups - 1) / groups; // a step = `groups` rows, one per lane group of a workgroup
    auto launch = [&](auto vec, auto ed) {
        auto kern = k_gine_aggregate<decltype(vec)::value, decltype(ed)::value>;
        // the grid is what is resident at once (the kernel's own occupancy, at most GINE_WG_PER_CU per CU): every workgroup walks
        // `iters` steps, the steps of one sweep side by side in memory
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, GINE_WG_PER_CU);
        const int max_grid = std::max(occ.blocks * occ.cus, 1);
        const int iters = (steps + max_grid - 1) / max_grid;
        const int grid = (steps + iters - 1) / iters;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, x, edge_attr, we, ldwe, be, out, t.node_rec, t.col, t.eid, t.num_nodes,
                           t.num_edges, width, glog2, eps, avec, iters);
    };
    auto by_vec = [&](auto ed) {
        if (v4)
            launch(IntTag<4>{}, ed);
        else
            launch(IntTag<1>{}, ed);
    };
    switch (edge_dim) {
#define GNNB_GINE_ED(n) case n: by_vec(IntTag<n>{}); break;
    GNNB_GINE_ED(1) GNNB_GINE_ED(2) GNNB_GINE_ED(3) GNNB_GINE_ED(4) GNNB_GINE_ED(5) GNNB_GINE_ED(6) GNNB_GINE_ED(7) GNNB_GINE_ED(8)
    GNNB_GINE_ED(9) GNNB_GINE_ED(10) GNNB_GINE_ED(11) GNNB_GINE_ED(12) GNNB_GINE_ED(13) GNNB_GINE_ED(14) GNNB_GINE_ED(15) GNNB_GINE_ED(16)
#undef GNNB_GINE_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
