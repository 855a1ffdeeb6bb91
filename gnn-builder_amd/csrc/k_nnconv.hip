// k_nnconv.hip -- NNConv (the edge-conditioned convolution of Gilmer et al.'s MPNN) aggregated BEFORE the transform (gnnb_nnconv.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// The layer is out_i = root x_i + bias + aggr_{j -> i} x_j Theta(e_ij) with Theta(e) = nn(e).view(in, out).  nn's last linear
// (W2, b2) is linear in the per-edge COEFFICIENT VECTOR c_ij of length K' + 1,
//   (L) nn = Linear(d, in out):                          K' = d, c = [e_ij ; 1]
//   (H) nn = Linear(d, K) -> ReLU -> Linear(K, in out):  K' = K, c = [relu(W1 e_ij + b1) ; 1]
// so sum_j x_j Theta(e_ij) = A_i W_fold with
//   k_nnconv_aggregate:  A_i[k in + col] = sum_{j -> i} c_ijk x_j[col]      [N, (K' + 1) in], k-major
// and W_fold a permutation of (W2, b2) (gnnb_weights.h: nnconv_fold) that the layer's ONE GEMM applies together with the root
// term.  Per edge ONE row of the INPUT width is gathered -- the traffic of a plain sum --; Theta [E, in, out], the messages
// [E, out] and, for (H), the hidden activations [E, K] exist nowhere.
//
// Work split: k_gine_aggregate's row walk.  A lane group of G = 2^glog2 lanes owns a destination row, a lane owns VEC = 4 or 1
// consecutive columns (scalar form: width % 4 != 0 or x / A unaligned -- a first layer runs at in = 9, 11, ...), rows of more
// than 64 vectors take column passes, the grid is what is resident and walks the rows with a grid stride, NN_R neighbour rows and
// their attribute rows are in flight, and the walk is software-pipelined over three steps (record of row it + 2, slots of row
// it + 1, rows of row `it`).
// The inner step is the outer product c_ij (x) x_j in registers: acc[KP + 1][VEC] (68 floats at KP 16, VEC 4), (KP + 1) VEC FMAs per
// edge on the one gathered x_j vector; block KP -- the constant coefficient's -- is the plain neighbour sum.
//   (L) the coefficients are the attribute row itself: the same address in every lane of the group, one fetch serves the group.
//   (H) W1 [K, d] and b1 are staged in LDS once per workgroup, zero-padded to [KP, ED]; every lane forms relu(W1 e + b1) itself from
//       broadcast LDS reads, KP ED FMAs per edge (redundant across the group, no cross-lane exchange).
// KP and ED are template parameters from a padded ladder, so that every loop unrolls and the accumulators stay in registers: a padded
// coefficient is relu(0 e + 0) = 0 or a zero-filled attribute, adds exactly nothing, and its block is not stored.
//
// Summation order (fixed: it depends on the batch, never on the launch shape):
//   c_k   = relu(fma(W1[k][d - 1], e[d - 1], ... fma(W1[k][0], e[0], b1[k])))                       -- d increasing (H)
//   piece = a row's CSR slots in pieces of NN_CHUNK = 64: acc[k] = fma(c_k, x_j, acc[k]) in slot order, starting from 0
//   row   = the pieces' sums added in piece order, starting from 0 (a row of at most 64 in-edges IS its one piece)
//   A     = row * (1 / deg) for aggr = mean, last (in-degree 0: 0)
// A row of more than NN_CHUNK in-edges (a hub) is split over the workgroup's lane groups through LDS exactly as GINE's hub rule;
// the piece sums cross LDS one coefficient block at a time (WG VEC floats of LDS whatever KP).
// Every one of a lane's K' + 1 stores is a 16-byte piece of a stretch that is contiguous across the group; non-temporal, A is read
// next by the GEMM, not by this kernel.
#include "gnnb_device.h"

namespace gnnb {

constexpr int NN_CHUNK = 64;    // CSR slots per piece of a row's sum
constexpr int NN_R = 4;         // neighbour rows in flight per lane group
constexpr int NN_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most

// one edge's d <= ED attributes, zero-filled to ED; avec (wave-uniform): d == ED, rows of 16-byte pieces at aligned addresses
template <int ED>
__device__ __forceinline__ void nn_load_attr(const float *p, int d, bool avec, float (&e)[ED])
{
    if (avec) {
        row_load_attr<ED>(p, true, e);
        return;
    }
#pragma unroll
    for (int q = 0; q < ED; q++)
        e[q] = q < d ? p[q] : 0.0f;
}

// the first n of NN_R neighbours' x_j (the lane's VEC columns from column fo) and attribute rows
template <int VEC, int ED>
__device__ __forceinline__ void nn_load_messages(const float *__restrict__ x, const float *__restrict__ ea, const int (&j)[NN_R],
                                                 const int (&ei)[NN_R], int n, int w, int fo, int d, bool avec, float (&xj)[NN_R][VEC],
                                                 float (&e)[NN_R][ED])
{
#pragma unroll
    for (int r = 0; r < NN_R; r++) {
#pragma unroll
        for (int v = 0; v < VEC; v++)
            xj[r][v] = 0.0f;
#pragma unroll
        for (int q = 0; q < ED; q++)
            e[r][q] = 0.0f;
        if (r < n) {
            row_load_vec<VEC>(x + (size_t)j[r] * w + fo, xj[r]);
            nn_load_attr<ED>(ea + (size_t)ei[r] * d, d, avec, e[r]);
        }
    }
}

// acc += c (x) x_j of the first n of those neighbours, in their order.  HID: c = relu(W1 e + b1) from the LDS copy s_w1 [KP, ED],
// s_b1 [KP]; else c = e (KP == ED)
template <int VEC, int KP, int ED, int HID>
__device__ __forceinline__ void nn_add_messages(const float (&xj)[NN_R][VEC], const float (&e)[NN_R][ED], int n, const float *s_w1,
                                                const float *s_b1, float (&acc)[KP + 1][VEC])
{
#pragma unroll
    for (int r = 0; r < NN_R; r++)
        if (r < n) {
            // (an offset of 0 the compiler cannot see through: W1 is read from LDS per edge -- hoisted out of the edge loop as the loop
            // invariant it is, its KP ED values would take the registers the accumulators need)
            int z = 0;
            if constexpr (HID)
                asm volatile("" : "+v"(z));
#pragma unroll
            for (int k = 0; k < KP; k++) {
                float c;
                if constexpr (HID) {
                    c = s_b1[z + k];
#pragma unroll
                    for (int q = 0; q < ED; q++)
                        c = fmaf(s_w1[z + k * ED + q], e[r][q], c);
                    c = fmaxf(c, 0.0f);
                } else {
                    c = e[r][k];
                }
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[k][v] = fmaf(c, xj[r][v], acc[k][v]);
            }
#pragma unroll
            for (int v = 0; v < VEC; v++)
                acc[KP][v] += xj[r][v];
        }
}

// acc += the outer products of the CSR slots [k0, k1), in slot order
template <int VEC, int KP, int ED, int HID>
__device__ __forceinline__ void nn_piece_sum(const float *__restrict__ x, const float *__restrict__ ea, const int32_t *__restrict__ col,
                                             const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int w, int fo, int d, bool avec,
                                             const float *s_w1, const float *s_b1, float (&acc)[KP + 1][VEC])
{
    for (int k = k0; k < k1; k += NN_R) {
        int j[NN_R], ei[NN_R];
        float xj[NN_R][VEC], e[NN_R][ED];
        row_load_slots(col, eid, k, k1, N, E, j, ei);
        nn_load_messages<VEC, ED>(x, ea, j, ei, k1 - k, w, fo, d, avec, xj, e);
        nn_add_messages<VEC, KP, ED, HID>(xj, e, k1 - k, s_w1, s_b1, acc);
    }
}

// kq: K' (d for the linear variant, the hidden width K for the other), 1 <= kq <= KP; w1 [kq, d] / b1 [kq]: HID only
template <int VEC, int KP, int ED, int HID>
__global__ __launch_bounds__(WG) void k_nnconv_aggregate(const float *__restrict__ x, const float *__restrict__ ea, const float *__restrict__ w1,
                                                         const float *__restrict__ b1, float *__restrict__ out, int ldo,
                                                         const int4 *__restrict__ node_rec, const int32_t *__restrict__ col,
                                                         const int32_t *__restrict__ eid, int N, int E, int w, int glog2, int d, int kq,
                                                         int mean, int avec, int iters)
{
    static_assert(HID || KP == ED, "the linear variant's coefficients are the attribute row");
    __shared__ float s_part[WG * VEC];              // one coefficient block's piece sums of one round of a long row
    __shared__ int s_long[WG];                      // per lane group: the long row of its step, or -1
    __shared__ float s_w1[HID ? KP * ED : 1];       // W1, zero-padded to [KP, ED]
    __shared__ float s_b1[HID ? KP : 1];
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const int nvec = w / VEC;
    if constexpr (HID) {
        for (int i = threadIdx.x; i < KP * ED; i += WG) {
            const int k = i / ED, q = i % ED;
            s_w1[i] = (k < kq && q < d) ? w1[(size_t)k * d + q] : 0.0f;
        }
        for (int i = threadIdx.x; i < KP; i += WG)
            s_b1[i] = i < kq ? b1[i] : 0.0f;
        __syncthreads();
    }
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
        // 1 / deg last; blocks k < kq to their place, the constant coefficient's block behind them, padded blocks nowhere
        auto finish = [&](int node, int deg, float (&acc)[KP + 1][VEC]) {
            const float s = mean ? (deg > 0 ? 1.0f / (float)deg : 0.0f) : 1.0f;
            float *o = out + (size_t)node * ldo + fo;
#pragma unroll
            for (int k = 0; k <= KP; k++) {
                if (k < KP && k >= kq)
                    continue;
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    acc[k][v] *= s;
                row_store_nt<VEC>(o + (size_t)(k < KP ? k : kq) * w, acc[k]);
            }
        };
        // ---- rows of at most NN_CHUNK in-edges, no barrier; three steps in flight per lane group (k_gine.hip)
        int n0, rp_0, dg_0, n1, rp_1, dg_1;
        int j0[NN_R], e0[NN_R];
        row_of(0, n0, rp_0, dg_0);
        row_load_slots(col, eid, rp_0, rp_0 + (dg_0 <= NN_CHUNK ? dg_0 : 0), N, E, j0, e0);
        row_of(1, n1, rp_1, dg_1);
        bool any_long = false;
        for (int it = 0; it < iters; it++) {
            int n2, rp_2, dg_2, j1[NN_R], e1[NN_R];
            row_of(it + 2, n2, rp_2, dg_2);
            row_load_slots(col, eid, rp_1, rp_1 + (dg_1 <= NN_CHUNK ? dg_1 : 0), N, E, j1, e1);
            any_long |= dg_0 > NN_CHUNK;
            if (n0 < N && dg_0 <= NN_CHUNK && active) {
                float xj[NN_R][VEC], e[NN_R][ED], acc[KP + 1][VEC];
                nn_load_messages<VEC, ED>(x, ea, j0, e0, dg_0, w, fo, d, avec != 0, xj, e);
#pragma unroll
                for (int k = 0; k <= KP; k++)
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        acc[k][v] = 0.0f;
                nn_add_messages<VEC, KP, ED, HID>(xj, e, dg_0, s_w1, s_b1, acc);
                if (dg_0 > NN_R)
                    nn_piece_sum<VEC, KP, ED, HID>(x, ea, col, eid, rp_0 + NN_R, rp_0 + dg_0, N, E, w, fo, d, avec != 0, s_w1, s_b1, acc);
                finish(n0, dg_0, acc);
            }
            n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
            n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
            for (int r = 0; r < NN_R; r++)
                j0[r] = j1[r], e0[r] = e1[r];
        }
        // ---- long rows (every trip count and every barrier below is the same for the whole workgroup)
        if (!__syncthreads_or(any_long))
            continue;
        for (int it = 0; it < iters; it++) {
            int node, rp0, deg;
            row_of(it, node, rp0, deg);
            const bool is_long = deg > NN_CHUNK;
            if (!__syncthreads_or(is_long))
                continue;
            if (gl == 0)
                s_long[grp] = is_long ? node : -1;
            __syncthreads();
            for (int g = 0; g < groups; g++) {
                const int ln = s_long[g];
                if (ln < 0)
                    continue;
                int lrp, ldeg;
                row_record(node_rec, ln, E, lrp, ldeg);
                const int npieces = (ldeg + NN_CHUNK - 1) / NN_CHUNK;
                float acc[KP + 1][VEC];
#pragma unroll
                for (int k = 0; k <= KP; k++)
#pragma unroll
                    for (int v = 0; v < VEC; v++)
                        acc[k][v] = 0.0f;
                for (int c0 = 0; c0 < npieces; c0 += groups) {
                    const int c = c0 + grp;
                    float part[KP + 1][VEC];
#pragma unroll
                    for (int k = 0; k <= KP; k++)
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            part[k][v] = 0.0f;
                    if (c < npieces && active)
                        nn_piece_sum<VEC, KP, ED, HID>(x, ea, col, eid, lrp + c * NN_CHUNK, lrp + min((c + 1) * NN_CHUNK, ldeg), N, E, w, fo, d,
                                                       avec != 0, s_w1, s_b1, part);
                    const int nq = min(groups, npieces - c0);
#pragma unroll
                    for (int k = 0; k <= KP; k++) { // the piece sums of one coefficient block at a time, added in piece order
#pragma unroll
                        for (int v = 0; v < VEC; v++)
                            s_part[threadIdx.x * VEC + v] = part[k][v];
                        __syncthreads();
                        if (grp == g)
                            for (int q = 0; q < nq; q++)
#pragma unroll
                                for (int v = 0; v < VEC; v++)
                                    acc[k][v] += s_part[((q << glog2) + gl) * VEC + v];
                        __syncthreads();
                    }
                }
                if (grp == g && active)
                    finish(ln, ldeg, acc);
            }
            __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
        }
    }
}

// the padded ladder of K' (and of the linear variant's d): the smallest rung that covers n
static int nn_rung(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 12 ? 12 : 16; }

hipError_t launch_nnconv_aggregate(const BatchTables &t, const float *x, int width, const float *edge_attr, int edge_dim, const float *w1,
                                   const float *b1, int hidden, int mean, float *out, int ldo, hipStream_t s)
{
    const int kq = hidden > 0 ? hidden : edge_dim;
    if (edge_dim < 1 || edge_dim > NN_MAX_EDGE_DIM || hidden < 0 || hidden > NN_MAX_HIDDEN || width < 1 ||
        (int64_t)ldo < (int64_t)(kq + 1) * width || (hidden > 0 && (!w1 || !b1)))
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const bool v4 = (width % 4 == 0) && (ldo % 4 == 0) && (((uintptr_t)x & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int nvec = v4 ? width / 4 : width;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int steps = (t.num_nodes + groups - 1) / groups; // a step = `groups` rows, one per lane group of a workgroup
    auto launch = [&](auto vec, auto kp, auto ed, auto hid) {
        constexpr int ED = decltype(ed)::value;
        auto kern = k_nnconv_aggregate<decltype(vec)::value, decltype(kp)::value, ED, decltype(hid)::value>;
        const int avec = (edge_dim == ED) && (ED % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, NN_WG_PER_CU);
        const int max_grid = std::max(occ.blocks * occ.cus, 1);
        const int iters = (steps + max_grid - 1) / max_grid;
        const int grid = (steps + iters - 1) / iters;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, x, edge_attr, w1, b1, out, ldo, t.node_rec, t.col, t.eid, t.num_nodes, t.num_edges,
                           width, glog2, edge_dim, kq, mean, avec, iters);
    };
    auto by_vec = [&](auto kp, auto ed, auto hid) {
        if (v4)
            launch(IntTag<4>{}, kp, ed, hid);
        else
            launch(IntTag<1>{}, kp, ed, hid);
    };
    auto by_ed = [&](auto kp) { // (H): the attribute row padded to 4, 8 or 16
        if (edge_dim <= 4)
            by_vec(kp, IntTag<4>{}, IntTag<1>{});
        else if (edge_dim <= 8)
            by_vec(kp, IntTag<8>{}, IntTag<1>{});
        else
            by_vec(kp, IntTag<16>{}, IntTag<1>{});
    };
    switch (nn_rung(kq)) {
#define GNNB_NN_KP(n)                                                                                                                      \
    case n:                                                                                                                                 \
        if (hidden > 0)                                                                                                                     \
            by_ed(IntTag<n>{});                                                                                                             \
        else                                                                                                                                \
            by_vec(IntTag<n>{}, IntTag<n>{}, IntTag<0>{});                                                                                  \
        break;
    GNNB_NN_KP(1) GNNB_NN_KP(2) GNNB_NN_KP(4) GNNB_NN_KP(8) GNNB_NN_KP(12) GNNB_NN_KP(16)
#undef GNNB_NN_KP
    }
    return hipGetLastError();
}

} // namespace gnnb
