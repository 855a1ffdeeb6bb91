// k_gatv2.hip -- GATv2: the attention scores, their per-destination softmax and the weighted sum in ONE pass over the edges
// (gnnb_gat.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_gatv2_aggregate (models.py _GATv2Conv: PyG's GATv2Conv(concat=True, add_self_loops=True, share_weights=False)):
//   s_ij[h]  = sum_c att[h, c] * leaky_relu(xl_j[h, c] + xr_i[h, c])            j in N(i) u {i}
//   out_i[h] = act( sum_j softmax_j(s_ij[h]) * xl_j[h, :] + bias + skip_i )      softmax = exp(s - max) / (sum + 1e-16), as PyG
// on the CSR-by-destination tables of the prepared batch (node_rec, col) of a GCN workspace: graph prep has dropped the explicit
// (v, v) edges, the kernel adds the one self term itself.  The score is a function of the gathered row, so ONE gather of xl_j serves
// the score and the weighted sum; the softmax is online (running max m, running sum l, running weighted sum acc), so neither the
// [E, heads] scores nor the [E, width] messages ever reach HBM.
//
// Work split -- k_gine_aggregate's / k_pna_edge_aggregate's, with ONE difference: the unit of work is an ITEM = (destination row,
// head), item = row * heads + head, because the softmax of a head is independent of the other heads'.  A lane group of G = 2^glog2
// lanes owns an item, G >= C / VEC lanes (C = width / heads columns per head), at most a wave; a lane owns VEC consecutive
// columns of the head in each of T strides of G * VEC columns (T > 1: the scalar form at C > 64).  A lane group therefore holds
// columns of ONE head: the cross-lane sum of the score partials runs over the whole group, lanes past the head's columns add 0,
// and nothing can mix two heads whatever C / VEC is (3 lanes of 4 at C = 12, 65 columns over two strides of 64 at C = 65).
// 16-byte form (VEC = 4) when C % 4 == 0 and xl / xr / skip / out and the strides are 16-byte aligned, scalar form (VEC = 1)
// otherwise.  The grid is a few workgroups per CU, every lane group walks its items with a grid stride; att and xr_i of the lane's
// columns are registers for the whole item, bias and skip are read in the epilogue.  GAT_R neighbour rows are loaded before the
// first is consumed, and the walk is software-pipelined over three steps (record of item it + 2, slots of item it + 1, rows of
// item `it`).  Scores are summed across the lanes with DPP (inside 16 lanes) and wave shuffles (beyond): no LDS.
//
// Summation order (fixed: it depends on the batch and on the form -- VEC and G set how a score is split over lanes --, never on
// the grid or on which workgroup took an item):
//   score  = per lane sum_c fma(att_c, leaky_relu(xl_j[c] + xr_i[c]), .) over its columns, stride by stride, column increasing;
//            the lanes' partials added in a butterfly (distance 1, 2, 4, ... G / 2)
//   state  = (m, l, acc) starts from the self term: m = s_ii, l = 1, acc = xl_i
//   batch  = GAT_R = 4 consecutive CSR slots: m' = max(m, s_0 .. s_3); f = exp(m - m'); e_r = exp(s_r - m');
//            l = fma(l, f, ((e_0 + e_1) + e_2) + e_3) ; acc_c = fma(e_3, x_3c, fma(e_2, x_2c, fma(e_1, x_1c, fma(e_0, x_0c, acc_c * f))))
//            (slots past the row's end take no part: s = -inf, e = 0)
//   row    = of at most GAT_CHUNK = 64 in-edges: its batches in slot order onto the self state.  Longer (a hub): pieces of 64
//            slots, each piece's batches in slot order onto (-inf, 0, 0); the pieces merged in piece order onto the self state:
//            m' = max(m, m_p); l = l * exp(m - m') + l_p * exp(m_p - m'); acc likewise
//   out    = act((acc_c / (l + 1e-16) + bias_c) + skip_c)
// exp(x) is the hardware's exp2 of x * log2(e) (v_exp_f32, 1 ulp): the weights that matter have |x| small, where the scaled
// argument's rounding is a relative error of |x| * 2^-24 in the weight (tests/test_hip_gatv2.py holds it to the project's budget).
// Degree skew: a row of more than GAT_CHUNK in-edges is not walked by its own lane group.  The workgroup's lane groups take its
// pieces round-robin, park (m, l, acc) per piece in LDS and the owner merges them in piece order -- the rule above.  Long rows are
// taken in a second walk behind the short ones: a workgroup without one pays ONE barrier.
#include "gnnb_device.h"

namespace gnnb {

constexpr int GAT_CHUNK = 64;     // CSR slots per piece of a long row
constexpr int GAT_R = 4;          // neighbour rows in flight per lane group (one batch of the online softmax)
constexpr int GAT_WG_PER_CU = 8;  // workgroups per CU the grid is cut for at most (what is resident; more items than that: grid stride)
constexpr float GAT_LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ float gat_exp(float x) { return __builtin_amdgcn_exp2f(x * GAT_LOG2E); }

template <int VEC>
__device__ __forceinline__ void gat_load_vec(const float *p, float *v)
{
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

// non-temporal (a vector store with the nt bit): the output is not read again by this kernel and must not evict the xl rows the
// gathers hit in L2 (measured on k_pna_edge_aggregate)
template <int VEC>
__device__ __forceinline__ void gat_store_vec(float *p, const float *v)
{
    if constexpr (VEC == 4) {
        const agg_f32x4 t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<agg_f32x4 *>(p));
    } else {
        __builtin_nontemporal_store(v[0], p);
    }
}

// the sum of x over the 2^glog2 lanes of a lane group (aligned in the wave), the same bits in every lane: a butterfly of distance
// 1, 2 (quad permutes), 4, 8 (the half-row and row mirrors: every lane of the 4 / 8 lanes mirrored onto holds the same partial),
// 16, 32 (wave shuffles).  Every lane of the group must be active
__device__ __forceinline__ float gat_group_sum(float x, int glog2)
{
    if (glog2 >= 1)
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, false)); // quad_perm [1,0,3,2]
    if (glog2 >= 2)
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, false)); // quad_perm [2,3,0,1]
    if (glog2 >= 3)
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xf, 0xf, false)); // row_half_mirror
    if (glog2 >= 4)
        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xf, 0xf, false)); // row_mirror
    if (glog2 >= 5)
        x += __shfl_xor(x, 16, 64);
    if (glog2 >= 6)
        x += __shfl_xor(x, 32, 64);
    return x;
}

// a lane group's online-softmax state of one item: m and l are the same in every lane of the group, acc is the lane's columns'
template <int NC>
struct GatState {
    float m, l, acc[NC];
};

// the CSR slots [k, k + GAT_R) below k1: source rows clamped into [0, N) -- a malformed table cannot send a load outside; nothing
// is read for a slot at or past k1
__device__ __forceinline__ void gat_load_slots(const int32_t *__restrict__ col, int k, int k1, int N, int (&j)[GAT_R])
{
#pragma unroll
    for (int r = 0; r < GAT_R; r++) {
        j[r] = 0;
        if (k + r < k1)
            j[r] = min(max(col[k + r], 0), N - 1);
    }
}

// the lane's columns of row `row` of x (row stride ld, the head's first column at hc): stride t holds columns
// [(gl + t G) VEC, + VEC) of the head where that is below C, zeros elsewhere
template <int VEC, int T>
__device__ __forceinline__ void gat_load_row(const float *__restrict__ x, size_t row, int ld, int hc, int gl, int glog2, int C, float (&v)[T * VEC])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
        for (int u = 0; u < VEC; u++)
            v[t * VEC + u] = 0.0f;
        if (c < C)
            gat_load_vec<VEC>(x + row * (size_t)ld + hc + c, &v[t * VEC]);
    }
}

// the lane's part of the score of one gathered row: sum_c att_c * leaky_relu(xl_j[c] + xr_i[c]) (columns past the head: att = 0)
template <int NC>
__device__ __forceinline__ float gat_score_part(const float (&xj)[NC], const float (&xr)[NC], const float (&att)[NC], float slope)
{
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const float z = xj[c] + xr[c];
        s = fmaf(att[c], z > 0.0f ? z : z * slope, s);
    }
    return s;
}

// one batch: the first n (1 .. GAT_R) of the loaded neighbour rows taken into the state -- the rule of the header
template <int NC>
__device__ __forceinline__ void gat_take_batch(const float (&xj)[GAT_R][NC], int n, const float (&xr)[NC], const float (&att)[NC], float slope,
                                               int glog2, GatState<NC> &a)
{
    float s[GAT_R];
#pragma unroll
    for (int r = 0; r < GAT_R; r++)
        s[r] = gat_score_part<NC>(xj[r], xr, att, slope);
#pragma unroll
    for (int r = 0; r < GAT_R; r++)
        s[r] = gat_group_sum(s[r], glog2);
    float m1 = a.m;
#pragma unroll
    for (int r = 0; r < GAT_R; r++) {
        s[r] = r < n ? s[r] : -INFINITY;
        m1 = fmaxf(m1, s[r]);
    }
    // (m1 is finite: n >= 1 and a score is finite; a.m = -inf, the start of a long row's piece, gives f = exp2(-inf) = 0)
    const float f = gat_exp(a.m - m1);
    float e[GAT_R];
#pragma unroll
    for (int r = 0; r < GAT_R; r++)
        e[r] = gat_exp(s[r] - m1);
    a.m = m1;
    a.l = fmaf(a.l, f, ((e[0] + e[1]) + e[2]) + e[3]);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = a.acc[c] * f;
#pragma unroll
        for (int r = 0; r < GAT_R; r++)
            t = fmaf(e[r], xj[r][c], t);
        a.acc[c] = t;
    }
}

// the first n of GAT_R neighbours' xl rows (the lane's columns); the others zeros
template <int VEC, int T>
__device__ __forceinline__ void gat_load_rows(const float *__restrict__ xl, int ldl, const int (&j)[GAT_R], int n, int hc, int gl, int glog2, int C,
                                              float (&xj)[GAT_R][T * VEC])
{
#pragma unroll
    for (int r = 0; r < GAT_R; r++) {
        if (r < n)
            gat_load_row<VEC, T>(xl, (size_t)j[r], ldl, hc, gl, glog2, C, xj[r]);
        else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                xj[r][c] = 0.0f;
        }
    }
}

// the CSR slots [k0, k1) taken into the state in batches of GAT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void gat_piece(const float *__restrict__ xl, int ldl, const int32_t *__restrict__ col, int k0, int k1, int N, int hc, int gl,
                                          int glog2, int C, const float (&xr)[T * VEC], const float (&att)[T * VEC], float slope,
                                          GatState<T * VEC> &a)
{
    for (int k = k0; k < k1; k += GAT_R) {
        int j[GAT_R];
        float xj[GAT_R][T * VEC];
        gat_load_slots(col, k, k1, N, j);
        gat_load_rows<VEC, T>(xl, ldl, j, k1 - k, hc, gl, glog2, C, xj);
        gat_take_batch<T * VEC>(xj, min(k1 - k, GAT_R), xr, att, slope, glog2, a);
    }
}

// row's start and in-degree from its node record, clamped into the E slots of col
__device__ __forceinline__ void gat_row(const int4 *__restrict__ node_rec, int node, int E, int &rp0, int &deg)
{
    const int4 r0 = node_rec[2 * (size_t)node];
    rp0 = min(max(r0.x, 0), E);
    deg = min(max(r0.y, 0), E - rp0);
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_gatv2_aggregate(const float *__restrict__ xl, int ldl, const float *__restrict__ xr, int ldr,
                                                         const float *__restrict__ attw, const float *__restrict__ bias,
                                                         const float *__restrict__ skip, float *__restrict__ out,
                                                         const int4 *__restrict__ node_rec, const int32_t *__restrict__ col, int N, int E, int w,
                                                         int heads, int C, float slope, int glog2, int iters)
{
    constexpr int NC = T * VEC;
    __shared__ float s_part[WG * (NC + 2)]; // one round of a long row's pieces: [lane group][lane of the group][m, l, acc[NC]]
    __shared__ int s_long[WG];              // per lane group: the long item of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const int items = N * heads;
    // step `it` of this lane group: its item, the item's row and that row's record (item = items, degree 0 past the batch or past
    // the last step)
    auto item_of = [&](int it, int &item, int &node, int &rp0, int &deg) {
        item = it < iters ? (it * (int)gridDim.x + (int)blockIdx.x) * groups + grp : items;
        node = 0, rp0 = 0, deg = 0;
        if (item < items) {
            node = item / heads;
            gat_row(node_rec, node, E, rp0, deg);
        } else
            item = items;
    };
    // an item's loop invariants: att of the lane's columns of its head, xr_i, and the self-initialised state
    auto begin = [&](int node, int hc, float (&att)[NC], float (&xri)[NC], GatState<NC> &a) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
            for (int u = 0; u < VEC; u++)
                att[t * VEC + u] = c < C ? attw[hc + c + u] : 0.0f;
        }
        gat_load_row<VEC, T>(xr, (size_t)node, ldr, hc, gl, glog2, C, xri);
        gat_load_row<VEC, T>(xl, (size_t)node, ldl, hc, gl, glog2, C, a.acc);
        a.m = gat_group_sum(gat_score_part<NC>(a.acc, xri, att, slope), glog2);
        a.l = 1.0f;
    };
    auto finish = [&](int node, int hc, const GatState<NC> &a) {
        const float den = a.l + 1e-16f;
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < C) {
                float o[VEC], sk[VEC];
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = a.acc[t * VEC + u] / den;
                if (bias != nullptr) // (an absent term adds nothing, not + 0: the row keeps its bits)
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += bias[hc + c + u];
                if (skip != nullptr) {
                    gat_load_vec<VEC>(skip + (size_t)node * w + hc + c, sk);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = act_t<ACT>(o[u]);
                gat_store_vec<VEC>(out + (size_t)node * w + hc + c, o);
            }
        }
    };
    // ---- rows of at most GAT_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first GAT_R slots of step it + 1
    // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
    // same in all lanes of a lane group (the cross-lane sums need the whole group)
    int i0, n0, rp_0, dg_0, i1, n1, rp_1, dg_1;
    int j0[GAT_R];
    item_of(0, i0, n0, rp_0, dg_0);
    gat_load_slots(col, rp_0, rp_0 + (dg_0 <= GAT_CHUNK ? dg_0 : 0), N, j0);
    item_of(1, i1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int i2, n2, rp_2, dg_2, j1[GAT_R];
        item_of(it + 2, i2, n2, rp_2, dg_2);
        gat_load_slots(col, rp_1, rp_1 + (dg_1 <= GAT_CHUNK ? dg_1 : 0), N, j1);
        any_long |= dg_0 > GAT_CHUNK;
        if (i0 < items && dg_0 <= GAT_CHUNK) {
            const int hc = (i0 - n0 * heads) * C;
            float att[NC], xri[NC], xj[GAT_R][NC];
            GatState<NC> a;
            gat_load_rows<VEC, T>(xl, ldl, j0, dg_0, hc, gl, glog2, C, xj);
            begin(n0, hc, att, xri, a);
            if (dg_0 > 0)
                gat_take_batch<NC>(xj, min(dg_0, GAT_R), xri, att, slope, glog2, a);
            if (dg_0 > GAT_R)
                gat_piece<VEC, T>(xl, ldl, col, rp_0 + GAT_R, rp_0 + dg_0, N, hc, gl, glog2, C, xri, att, slope, a);
            finish(n0, hc, a);
        }
        i0 = i1, n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        i1 = i2, n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < GAT_R; r++)
            j0[r] = j1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE barrier
    if (!__syncthreads_or(any_long))
        return;
    for (int it = 0; it < iters; it++) {
        int item, node, rp0, deg;
        item_of(it, item, node, rp0, deg);
        const bool is_long = deg > GAT_CHUNK;
        if (!__syncthreads_or(is_long))
            continue;
        // the long items of this step, one after the other: pieces round-robin over the lane groups, partials through LDS
        if (gl == 0)
            s_long[grp] = is_long ? item : -1;
        __syncthreads();
        for (int g = 0; g < groups; g++) {
            const int li = s_long[g];
            if (li < 0)
                continue;
            const int ln = li / heads, hc = (li - ln * heads) * C;
            int lrp, ldeg;
            gat_row(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + GAT_CHUNK - 1) / GAT_CHUNK;
            float att[NC], xri[NC];
            GatState<NC> a; // (the owner's: the self state, then the pieces in their order; the others' copy is not used)
            begin(ln, hc, att, xri, a);
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                GatState<NC> part;
                part.m = -INFINITY, part.l = 0.0f;
#pragma unroll
                for (int q = 0; q < NC; q++)
                    part.acc[q] = 0.0f;
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gat_piece<VEC, T>(xl, ldl, col, lrp + c * GAT_CHUNK, lrp + min((c + 1) * GAT_CHUNK, ldeg), N, hc, gl, glog2, C, xri, att, slope, part);
                float *sp = s_part + (size_t)threadIdx.x * (NC + 2);
                sp[0] = part.m, sp[1] = part.l;
#pragma unroll
                for (int q = 0; q < NC; q++)
                    sp[2 + q] = part.acc[q];
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++) {
                        const float *pp = s_part + (size_t)((qq << glog2) + gl) * (NC + 2);
                        const float pm = pp[0], pl = pp[1];
                        const float m1 = fmaxf(a.m, pm); // (finite: a.m is -- the self score)
                        const float fa = gat_exp(a.m - m1), fp = gat_exp(pm - m1);
                        a.m = m1;
                        a.l = fmaf(pl, fp, a.l * fa);
#pragma unroll
                        for (int q = 0; q < NC; q++)
                            a.acc[q] = fmaf(pp[2 + q], fp, a.acc[q] * fa);
                    }
                }
                __syncthreads();
            }
            if (grp == g)
                finish(ln, hc, a);
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long item)
    }
}

hipError_t launch_gatv2_aggregate(const BatchTables &t, const float *xl, int ldl, const float *xr, int ldr, const float *att, const float *bias,
                                  const float *skip, int act, int heads, float slope, float *out, int width, hipStream_t s)
{
    if (heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH || width % heads != 0 || ldl < width || ldr < width ||
        (uint64_t)std::max(t.num_nodes, 0) * (uint64_t)heads > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const int C = width / heads;
    const bool v4 = (C % 4 == 0) && (ldl % 4 == 0) && (ldr % 4 == 0) && (((uintptr_t)xl & 15) == 0) && (((uintptr_t)xr & 15) == 0) &&
                    (((uintptr_t)skip & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int nvec = v4 ? C / 4 : C;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int64_t items = (int64_t)t.num_nodes * heads;
    const int steps = (int)((items + groups - 1) / groups); // a step = `groups` items, one per lane group of a workgroup
    auto launch = [&](auto vec, auto strides, auto a) {
        auto kern = k_gatv2_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
        // the grid is what is resident at once (the kernel's own occupancy, at most GAT_WG_PER_CU per CU): every workgroup walks
        // `iters` steps, the steps of one sweep side by side in memory
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, GAT_WG_PER_CU);
        const int max_grid = std::max(occ.blocks * occ.cus, 1);
        const int iters = (steps + max_grid - 1) / max_grid;
        const int grid = (steps + iters - 1) / iters;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, xl, ldl, xr, ldr, att, bias, skip, out, t.node_rec, t.col, t.num_nodes, t.num_edges,
                           width, heads, C, slope, glog2, iters);
    };
    auto by_form = [&](auto a) {
        if (v4)
            launch(IntTag<4>{}, IntTag<1>{}, a); // (C / 4 <= 64: one stride)
        else if (C <= 64)
            launch(IntTag<1>{}, IntTag<1>{}, a);
        else
            launch(IntTag<1>{}, IntTag<4>{}, a); // (C <= 256: four strides of a wave)
    };
    GNNB_DISPATCH_ACT(act, by_form);
    return hipGetLastError();
}

} // namespace gnnb
