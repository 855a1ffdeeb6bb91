// k_transformer.hip -- TransformerConv: the scaled dot-product scores, their per-destination softmax and the weighted sum of the
// value rows in ONE pass over the edges (gnnb_transformer.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the
// GNNBuilder hot path); wavefront = 64 lanes.
//
// k_transformer_aggregate (models.py _TransformerConv: PyG's TransformerConv(concat=True, beta=False, edge_dim=None, root_weight=True)):
//   s_ij[h]  = (sum_c q_i[h, c] * k_j[h, c]) * scale                             j in N(i) -- the input's edges as they are
//   out_i[h] = act( (sum_j softmax_j(s_ij[h]) * v_j[h, :] + root_i) + skip_i )    softmax = exp(s - max) / (sum + 1e-16), as PyG
// on the CSR-by-destination tables of the prepared batch (node_rec, col) of a workspace whose tables keep explicit (v, v) edges
// (any but a GCN description's): no self term is added and none is removed, a row without in-edges gets root_i alone.  The row
// that is scored (k_j) is not the row that is summed (v_j): TWO gathers per edge where k_gatv2_aggregate has one.  The softmax is
// online (running max m, running sum l, running weighted sum acc), so neither the [E, heads] scores nor the [E, width] messages
// ever reach HBM.
//
// Work split -- k_gatv2_aggregate's (k_gatv2.hip), reused as it stands: an ITEM = (destination row, head), item = row * heads +
// head, is owned by a lane group of G = 2^glog2 lanes, G >= C / VEC (C = width / heads columns per head), at most a wave; a lane
// owns VEC consecutive columns of the head in each of T strides of G * VEC columns (T > 1: the scalar form at C > 64).  A lane
// group holds columns of ONE head, so the cross-lane sum of the score partials cannot mix two heads; lanes past the head's columns
// add 0.  16-byte form (VEC = 4) when C % 4 == 0 and q / k / v / root / skip / out and the strides are 16-byte aligned, scalar
// form (VEC = 1) otherwise.  The grid is cut from the kernel's own occupancy (at most TF_WG_PER_CU workgroups per CU), every lane
// group walks its items with a grid stride.  q_i of the lane's columns -- as loaded, multiplied by nothing -- is the item's only
// invariant and stays in registers; root and skip are read in the epilogue.  TF_R neighbours are in flight per batch: their
// TF_R x 2 row loads (k_j and v_j of the lane's columns) are all issued before the first is consumed.  The walk is three deep
// (record of item it + 2, slots of item it + 1, rows of item `it`).  Scores are summed across the lanes with DPP (inside 16
// lanes) and wave shuffles (beyond): no LDS on the short-row path.  Stores are non-temporal.
//
// Summation order (fixed: it depends on the batch and on the form -- VEC and G set how a score is split over lanes --, never on
// the grid or on which workgroup took an item):
//   score  = per lane sum_c fma(q_c, k_jc, .) over its columns, stride by stride, column increasing; the lanes' partials added in a
//            butterfly (distance 1, 2, 4, ... G / 2); the sum times `scale`, ONE multiply per score ("dot, then scale")
//   state  = (m, l, acc) starts at (-inf, 0, 0): there is no self term
//   batch  = TF_R = 4 consecutive CSR slots: m' = max(m, s_0 .. s_3); f = exp(m - m'); e_r = exp(s_r - m');
//            l = fma(l, f, ((e_0 + e_1) + e_2) + e_3) ; acc_c = fma(e_3, v_3c, fma(e_2, v_2c, fma(e_1, v_1c, fma(e_0, v_0c, acc_c * f))))
//            (slots past the row's end take no part: s = -inf, e = 0; m = -inf in front of the first batch gives f = exp2(-inf) = 0)
//   row    = of at most TF_CHUNK = 64 in-edges: its batches in slot order.  Longer (a hub): pieces of 64 slots, each piece's batches
//            in slot order onto (-inf, 0, 0); the pieces merged in piece order onto (-inf, 0, 0):
//            m' = max(m, m_p); l = l * exp(m - m') + l_p * exp(m_p - m'); acc likewise
//   out    = act((acc_c / (l + 1e-16) + root_c) + skip_c); a row without in-edges takes nothing: act(root_c + skip_c) with root's
//            own bits (0 where root is absent)
// exp(x) is the hardware's exp2 of x * log2(e) (v_exp_f32, 1 ulp), as in k_gatv2_aggregate.
// Degree skew: k_gatv2_aggregate's second walk.  A row of more than TF_CHUNK in-edges is taken by the workgroup's lane groups in
// pieces round-robin, (m, l, acc) per piece parked in LDS, merged by the owner in piece order.  A workgroup without a long row
// pays ONE barrier.
#include "gnnb_device.h"

namespace gnnb {

constexpr int TF_CHUNK = 64;    // CSR slots per piece of a long row
constexpr int TF_R = 4;         // neighbours in flight per lane group (one batch of the online softmax): TF_R x 2 row loads
constexpr int TF_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more items than that: grid stride)
constexpr float TF_LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ float tf_exp(float x) { return __builtin_amdgcn_exp2f(x * TF_LOG2E); }

template <int VEC>
__device__ __forceinline__ void tf_load_vec(const float *p, float *v)
{
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

// non-temporal (a vector store with the nt bit): the output is not read again by this kernel and must not evict the k / v rows the
// gathers hit in L2 (measured on k_pna_edge_aggregate)
template <int VEC>
__device__ __forceinline__ void tf_store_vec(float *p, const float *v)
{
    if constexpr (VEC == 4) {
        const agg_f32x4 t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<agg_f32x4 *>(p));
    } else {
        __builtin_nontemporal_store(v[0], p);
    }
}

// the sum of x over the 2^glog2 lanes of a lane group (aligned in the wave), the same bits in every lane: k_gatv2.hip's butterfly
// of distance 1, 2 (quad permutes), 4, 8 (the half-row and row mirrors), 16, 32 (wave shuffles).  Every lane of the group must be
// active
__device__ __forceinline__ float tf_group_sum(float x, int glog2)
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
struct TfState {
    float m, l, acc[NC];
    __device__ __forceinline__ void clear()
    {
        m = -INFINITY, l = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++)
            acc[c] = 0.0f;
    }
};

// the CSR slots [k, k + TF_R) below k1: source rows clamped into [0, N) -- a malformed table cannot send a load outside; nothing
// is read for a slot at or past k1
__device__ __forceinline__ void tf_load_slots(const int32_t *__restrict__ col, int k, int k1, int N, int (&j)[TF_R])
{
#pragma unroll
    for (int r = 0; r < TF_R; r++) {
        j[r] = 0;
        if (k + r < k1)
            j[r] = min(max(col[k + r], 0), N - 1);
    }
}

// the lane's columns of row `row` of x (row stride ld, the head's first column at hc): stride t holds columns
// [(gl + t G) VEC, + VEC) of the head where that is below C, zeros elsewhere
template <int VEC, int T>
__device__ __forceinline__ void tf_load_row(const float *__restrict__ x, size_t row, int ld, int hc, int gl, int glog2, int C, float (&v)[T * VEC])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
        for (int u = 0; u < VEC; u++)
            v[t * VEC + u] = 0.0f;
        if (c < C)
            tf_load_vec<VEC>(x + row * (size_t)ld + hc + c, &v[t * VEC]);
    }
}

// the first n of TF_R neighbours' k and v rows (the lane's columns), all 2 TF_R loads issued side by side; the others zeros
template <int VEC, int T>
__device__ __forceinline__ void tf_load_rows(const float *__restrict__ kx, int ldk, const float *__restrict__ vx, int ldv, const int (&j)[TF_R], int n,
                                             int hc, int gl, int glog2, int C, float (&kj)[TF_R][T * VEC], float (&vj)[TF_R][T * VEC])
{
#pragma unroll
    for (int r = 0; r < TF_R; r++) {
        if (r < n) {
            tf_load_row<VEC, T>(kx, (size_t)j[r], ldk, hc, gl, glog2, C, kj[r]);
            tf_load_row<VEC, T>(vx, (size_t)j[r], ldv, hc, gl, glog2, C, vj[r]);
        } else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                kj[r][c] = 0.0f, vj[r][c] = 0.0f;
        }
    }
}

// one batch: the first n (1 .. TF_R) of the loaded neighbours taken into the state -- the rule of the header
template <int NC>
__device__ __forceinline__ void tf_take_batch(const float (&kj)[TF_R][NC], const float (&vj)[TF_R][NC], int n, const float (&q)[NC], float scale,
                                              int glog2, TfState<NC> &a)
{
    float s[TF_R];
#pragma unroll
    for (int r = 0; r < TF_R; r++) {
        float p = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++)
            p = fmaf(q[c], kj[r][c], p);
        s[r] = p;
    }
#pragma unroll
    for (int r = 0; r < TF_R; r++)
        s[r] = tf_group_sum(s[r], glog2) * scale;
    float m1 = a.m;
#pragma unroll
    for (int r = 0; r < TF_R; r++) {
        s[r] = r < n ? s[r] : -INFINITY;
        m1 = fmaxf(m1, s[r]);
    }
    // (m1 is finite: n >= 1 and a score is finite; a.m = -inf, the start of every row and piece, gives f = exp2(-inf) = 0)
    const float f = tf_exp(a.m - m1);
    float e[TF_R];
#pragma unroll
    for (int r = 0; r < TF_R; r++)
        e[r] = tf_exp(s[r] - m1);
    a.m = m1;
    a.l = fmaf(a.l, f, ((e[0] + e[1]) + e[2]) + e[3]);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = a.acc[c] * f;
#pragma unroll
        for (int r = 0; r < TF_R; r++)
            t = fmaf(e[r], vj[r][c], t);
        a.acc[c] = t;
    }
}

// the CSR slots [k0, k1) taken into the state in batches of TF_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void tf_piece(const float *__restrict__ kx, int ldk, const float *__restrict__ vx, int ldv, const int32_t *__restrict__ col,
                                         int k0, int k1, int N, int hc, int gl, int glog2, int C, const float (&q)[T * VEC], float scale,
                                         TfState<T * VEC> &a)
{
    for (int k = k0; k < k1; k += TF_R) {
        int j[TF_R];
        float kj[TF_R][T * VEC], vj[TF_R][T * VEC];
        tf_load_slots(col, k, k1, N, j);
        tf_load_rows<VEC, T>(kx, ldk, vx, ldv, j, k1 - k, hc, gl, glog2, C, kj, vj);
        tf_take_batch<T * VEC>(kj, vj, min(k1 - k, TF_R), q, scale, glog2, a);
    }
}

// row's start and in-degree from its node record, clamped into the E slots of col
__device__ __forceinline__ void tf_row(const int4 *__restrict__ node_rec, int node, int E, int &rp0, int &deg)
{
    const int4 r0 = node_rec[2 * (size_t)node];
    rp0 = min(max(r0.x, 0), E);
    deg = min(max(r0.y, 0), E - rp0);
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_transformer_aggregate(const float *__restrict__ qx, int ldq, const float *__restrict__ kx, int ldk,
                                                               const float *__restrict__ vx, int ldv, const float *__restrict__ root, int ldr,
                                                               const float *__restrict__ skip, float *__restrict__ out,
                                                               const int4 *__restrict__ node_rec, const int32_t *__restrict__ col, int N, int E,
                                                               int w, int heads, int C, float scale, int glog2, int iters)
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
            tf_row(node_rec, node, E, rp0, deg);
        } else
            item = items;
    };
    auto finish = [&](int node, int hc, const TfState<NC> &a) {
        const float den = a.l + 1e-16f;
        const bool took = a.l > 0.0f; // (in-degree 0: nothing was taken, the row is root's own bits -- not 0 + root, which loses a -0)
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < C) {
                float o[VEC], rt[VEC], sk[VEC];
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = a.acc[t * VEC + u] / den;
                if (root != nullptr) { // (an absent term adds nothing, not + 0: the row keeps its bits)
                    tf_load_vec<VEC>(root + (size_t)node * ldr + hc + c, rt);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] = took ? o[u] + rt[u] : rt[u];
                }
                if (skip != nullptr) {
                    tf_load_vec<VEC>(skip + (size_t)node * w + hc + c, sk);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = act_t<ACT>(o[u]);
                tf_store_vec<VEC>(out + (size_t)node * w + hc + c, o);
            }
        }
    };
    // ---- rows of at most TF_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first TF_R slots of step it + 1 are
    // requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
    // same in all lanes of a lane group (the cross-lane sums need the whole group)
    int i0, n0, rp_0, dg_0, i1, n1, rp_1, dg_1;
    int j0[TF_R];
    item_of(0, i0, n0, rp_0, dg_0);
    tf_load_slots(col, rp_0, rp_0 + (dg_0 <= TF_CHUNK ? dg_0 : 0), N, j0);
    item_of(1, i1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int i2, n2, rp_2, dg_2, j1[TF_R];
        item_of(it + 2, i2, n2, rp_2, dg_2);
        tf_load_slots(col, rp_1, rp_1 + (dg_1 <= TF_CHUNK ? dg_1 : 0), N, j1);
        any_long |= dg_0 > TF_CHUNK;
        if (i0 < items && dg_0 <= TF_CHUNK) {
            const int hc = (i0 - n0 * heads) * C;
            float q[NC], kj[TF_R][NC], vj[TF_R][NC];
            TfState<NC> a;
            tf_load_rows<VEC, T>(kx, ldk, vx, ldv, j0, dg_0, hc, gl, glog2, C, kj, vj);
            tf_load_row<VEC, T>(qx, (size_t)n0, ldq, hc, gl, glog2, C, q);
            a.clear();
            if (dg_0 > 0)
                tf_take_batch<NC>(kj, vj, min(dg_0, TF_R), q, scale, glog2, a);
            if (dg_0 > TF_R)
                tf_piece<VEC, T>(kx, ldk, vx, ldv, col, rp_0 + TF_R, rp_0 + dg_0, N, hc, gl, glog2, C, q, scale, a);
            finish(n0, hc, a);
        }
        i0 = i1, n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        i1 = i2, n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < TF_R; r++)
            j0[r] = j1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE barrier
    if (!__syncthreads_or(any_long))
        return;
    for (int it = 0; it < iters; it++) {
        int item, node, rp0, deg;
        item_of(it, item, node, rp0, deg);
        const bool is_long = deg > TF_CHUNK;
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
            tf_row(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + TF_CHUNK - 1) / TF_CHUNK;
            float q[NC];
            TfState<NC> a; // (the owner's: the pieces in their order onto the empty state; the others' copy is not used)
            tf_load_row<VEC, T>(qx, (size_t)ln, ldq, hc, gl, glog2, C, q);
            a.clear();
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                TfState<NC> part;
                part.clear();
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    tf_piece<VEC, T>(kx, ldk, vx, ldv, col, lrp + c * TF_CHUNK, lrp + min((c + 1) * TF_CHUNK, ldeg), N, hc, gl, glog2, C, q, scale,
                                     part);
                float *sp = s_part + (size_t)threadIdx.x * (NC + 2);
                sp[0] = part.m, sp[1] = part.l;
#pragma unroll
                for (int u = 0; u < NC; u++)
                    sp[2 + u] = part.acc[u];
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++) {
                        const float *pp = s_part + (size_t)((qq << glog2) + gl) * (NC + 2);
                        const float pm = pp[0], pl = pp[1];
                        const float m1 = fmaxf(a.m, pm); // (finite: pm is -- a piece that is read holds a slot; a.m = -inf: fa = 0)
                        const float fa = tf_exp(a.m - m1), fp = tf_exp(pm - m1);
                        a.m = m1;
                        a.l = fmaf(pl, fp, a.l * fa);
#pragma unroll
                        for (int u = 0; u < NC; u++)
                            a.acc[u] = fmaf(pp[2 + u], fp, a.acc[u] * fa);
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

hipError_t launch_transformer_aggregate(const BatchTables &t, const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                        const float *root, int ldr, const float *skip, int act, int heads, float scale, float *out, int width,
                                        hipStream_t s)
{
    if (heads < 1 || heads > TF_MAX_HEADS || width < 1 || width > TF_MAX_WIDTH || width % heads != 0 || ldq < width || ldk < width ||
        ldv < width || (root != nullptr && ldr < width) || (uint64_t)std::max(t.num_nodes, 0) * (uint64_t)heads > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const int C = width / heads;
    auto al = [](const float *p) { return ((uintptr_t)p & 15) == 0; };
    const bool v4 = (C % 4 == 0) && (ldq % 4 == 0) && (ldk % 4 == 0) && (ldv % 4 == 0) && (root == nullptr || ldr % 4 == 0) && al(q) && al(k) &&
                    al(v) && al(root) && al(skip) && al(out);
    const int nvec = v4 ? C / 4 : C;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int64_t items = (int64_t)t.num_nodes * heads;
    const int steps = (int)((items + groups - 1) / groups); // a step = `groups` items, one per lane group of a workgroup
    auto launch = [&](auto vec, auto strides, auto a) {
        auto kern = k_transformer_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
        // the grid is what is resident at once (the kernel's own occupancy, at most TF_WG_PER_CU per CU): every workgroup walks
        // `iters` steps, the steps of one sweep side by side in memory
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, TF_WG_PER_CU);
        const int max_grid = std::max(occ.blocks * occ.cus, 1);
        const int iters = (steps + max_grid - 1) / max_grid;
        const int grid = (steps + iters - 1) / iters;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, q, ldq, k, ldk, v, ldv, root, root != nullptr ? ldr : width, skip, out, t.node_rec,
                           t.col, t.num_nodes, t.num_edges, width, heads, C, scale, glog2, iters);
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
