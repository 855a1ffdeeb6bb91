// k_gatv2_edge.hip -- GATv2 with edge features: the edge projection, the attention scores, their per-destination softmax and the
// weighted sum in ONE pass over the edges (gnnb_gat_edge.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the
// GNNBuilder hot path); wavefront = 64 lanes.
//
// k_gatv2_edge_aggregate (models.py _GATv2EConv: PyG's GATv2Conv(concat=True, add_self_loops=True, share_weights=False,
// edge_dim=d, fill_value='mean')):
//   p_ij     = W_e e_ij                                                           e_ij = edge_attr[eid[slot]]  (COO row order)
//   s_ij[h]  = sum_c att[h, c] * leaky_relu(xl_j[h, c] + xr_i[h, c] + p_ij[h, c])  j in N(i) u {i}
//   out_i[h] = act( sum_j softmax_j(s_ij[h]) * xl_j[h, :] + bias + skip_i )        softmax = exp(s - max) / (sum + 1e-16), as PyG
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid) of a GCN workspace: graph prep has dropped the
// explicit (v, v) edges -- their attribute rows are never read --, the kernel adds the one self term itself, with
// e_ii = the mean of the row's e_ji (0 for a row without in-edges).  The edge term enters the score only; the message is xl_j.
// Neither the [E, width] projected edge term nor the [E, heads] scores nor the messages ever reach HBM.
//
// Work split -- k_gatv2_aggregate's (k_gatv2.hip): an ITEM = (destination row, head) is owned by a lane group of G = 2^glog2
// lanes, G >= C / VEC (C = width / heads columns per head); a lane owns VEC consecutive columns of the head in each of T strides
// of G * VEC columns; 16-byte form (VEC = 4) when C % 4 == 0 and xl / xr / skip / out and the strides are 16-byte aligned, scalar
// form otherwise (T = 4 at C > 64).  ONE difference in how items are dealt: lane group gid = blockIdx.x * groups + grp of the grid
// keeps ONE head, gid % heads, for its whole life and walks the rows it * RS + gid / heads (RS = grid * groups / heads rows per
// sweep), so that what a lane holds for its columns is loaded once per lane, not per item:
//   W_e[c][0 .. edge_dim) and att[c] of the lane's T * VEC columns live in REGISTERS, as in k_gine_aggregate (no bias: lin_edge has
//   none).  The kernel is instantiated on edge_dim.
// The edge's attribute row is read at edge_attr + eid[slot] * edge_dim, the same address in every lane of the group (16-byte pieces
// when edge_dim % 4 == 0 and edge_attr is aligned).  GAE_R = 4 neighbour rows (xl_j and e_ij) are loaded before the first is
// consumed, and the walk is software-pipelined over three steps (record of step it + 2, slots of step it + 1, rows of step `it`).
// Scores are summed across the lanes with DPP and wave shuffles: no LDS.
//
// Summation order (fixed: it depends on the batch and on the form -- VEC and G set how a score is split over lanes --, never on
// the grid or on which workgroup took an item):
//   p_c    = fma(W_e[c][d - 1], e[d - 1], ... fma(W_e[c][0], e[0], 0))                                      -- d increasing
//   score  = per lane sum_c fma(att_c, leaky_relu((xl_j[c] + xr_i[c]) + p_c), .) over its columns, stride by stride, column
//            increasing; the lanes' partials added in a butterfly (distance 1, 2, 4, ... G / 2)
//   state  = (m, l, acc) starts from (-inf, 0, 0); the row's attribute sum a[0 .. d) from 0
//   batch  = GAE_R = 4 consecutive CSR slots: m' = max(m, s_0 .. s_3); f = exp(m - m'); e_r = exp(s_r - m');
//            l = fma(l, f, ((e_0 + e_1) + e_2) + e_3) ; acc_c = fma(e_3, x_3c, fma(e_2, x_2c, fma(e_1, x_1c, fma(e_0, x_0c, acc_c * f))))
//            a[d] = (((a[d] + e_0[d]) + e_1[d]) + e_2[d]) + e_3[d]
//            (slots past the row's end take no part: s = -inf, e = 0, attributes + 0)
//   row    = of at most GAE_CHUNK = 64 in-edges: its batches in slot order.  Longer (a hub): pieces of 64 slots, each piece's
//            batches in slot order onto its own (-inf, 0, 0) and attribute sum 0; the pieces merged in piece order onto
//            (-inf, 0, 0): m' = max(m, m_p); l = l * exp(m - m') + l_p * exp(m_p - m'); acc likewise; a[d] += a_p[d]
//   self   = LAST: the self term's attribute is the row's mean, which is known only behind the row.  e_ii[d] = a[d] / deg (one
//            division per attribute; deg = 0: e_ii = 0), projected once as p above -- PyG's order of operations (mean of the
//            attributes, then lin_edge) --, then one more step of the softmax: m' = max(m, s_ii); f = exp(m - m');
//            e = exp(s_ii - m'); l = fma(l, f, e); acc_c = fma(e, xl_ic, acc_c * f)
//   out    = act((acc_c / (l + 1e-16) + bias_c) + skip_c)
// A row without in-edges: f = exp(-inf) = 0, e = exp(0) = 1, l = 1, acc = xl_i, so out = act(xl_i + bias + skip_i) bit for bit.
// exp(x) is the hardware's exp2 of x * log2(e), as in k_gatv2_aggregate.
// Degree skew: a row of more than GAE_CHUNK in-edges is not walked by its own lane group.  The workgroup's lane groups take its
// pieces round-robin (with the OWNER's head: att, W_e and xr_i of that head are loaded again, the short rows are done by then),
// park (m, l, acc) and the piece's attribute sum in LDS, and the owner merges them in piece order and takes the self term -- the
// rule above.  Long rows are taken in a second walk behind the short ones: a workgroup without one pays ONE barrier.
#include "gnnb_device.h"

namespace gnnb {

constexpr int GAE_CHUNK = 64;     // CSR slots per piece of a long row
constexpr int GAE_R = 4;          // neighbour rows in flight per lane group (one batch of the online softmax)
constexpr int GAE_WG_PER_CU = 8;  // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int GAE_MAX_EDGE_DIM = 16;
constexpr float GAE_LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ float gae_exp(float x) { return __builtin_amdgcn_exp2f(x * GAE_LOG2E); }

template <int VEC>
__device__ __forceinline__ void gae_load_vec(const float *p, float *v)
{
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

// non-temporal: the output is not read again by this kernel and must not evict the xl rows the gathers hit in L2
template <int VEC>
__device__ __forceinline__ void gae_store_vec(float *p, const float *v)
{
    if constexpr (VEC == 4) {
        const agg_f32x4 t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<agg_f32x4 *>(p));
    } else {
        __builtin_nontemporal_store(v[0], p);
    }
}

// one edge's attributes; avec (wave-uniform): rows of 16-byte pieces at 16-byte aligned addresses
template <int ED>
__device__ __forceinline__ void gae_load_attr(const float *p, bool avec, float (&e)[ED])
{
    if constexpr (ED % 4 == 0) {
        if (avec) {
#pragma unroll
            for (int q = 0; q < ED / 4; q++) {
                const float4 t = *reinterpret_cast<const float4 *>(p + 4 * q);
                e[4 * q] = t.x, e[4 * q + 1] = t.y, e[4 * q + 2] = t.z, e[4 * q + 3] = t.w;
            }
            return;
        }
    }
#pragma unroll
    for (int d = 0; d < ED; d++)
        e[d] = p[d];
}

// the sum of x over the 2^glog2 lanes of a lane group (aligned in the wave), the same bits in every lane: k_gatv2.hip's butterfly
// (quad permutes, the half-row and row mirrors, wave shuffles).  Every lane of the group must be active
__device__ __forceinline__ float gae_group_sum(float x, int glog2)
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

__device__ __forceinline__ float gae_act(int act, float v)
{
    switch (act) {
    case GNNB_ACT_RELU: return act_t<GNNB_ACT_RELU>(v);
    case GNNB_ACT_GELU: return act_t<GNNB_ACT_GELU>(v);
    case GNNB_ACT_SIGMOID: return act_t<GNNB_ACT_SIGMOID>(v);
    case GNNB_ACT_TANH: return act_t<GNNB_ACT_TANH>(v);
    default: return v;
    }
}

// a lane group's online-softmax state of one item: m and l are the same in every lane of the group, acc is the lane's columns'
template <int NC>
struct GaeState {
    float m, l, acc[NC];
};

// the CSR slots [k, k + GAE_R) below k1: source rows and COO rows, clamped into the buffers (col into [0, N), eid into [0, E)) --
// a malformed table cannot send a load outside; nothing is read for a slot at or past k1
__device__ __forceinline__ void gae_load_slots(const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int k, int k1, int N, int E,
                                               int (&j)[GAE_R], int (&ei)[GAE_R])
{
#pragma unroll
    for (int r = 0; r < GAE_R; r++) {
        j[r] = 0, ei[r] = 0;
        if (k + r < k1) {
            j[r] = min(max(col[k + r], 0), N - 1);
            ei[r] = min(max(eid[k + r], 0), E - 1);
        }
    }
}

// the lane's columns of row `row` of x (row stride ld, the head's first column at hc): stride t holds columns
// [(gl + t G) VEC, + VEC) of the head where that is below C, zeros elsewhere
template <int VEC, int T>
__device__ __forceinline__ void gae_load_row(const float *__restrict__ x, size_t row, int ld, int hc, int gl, int glog2, int C, float (&v)[T * VEC])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
        for (int u = 0; u < VEC; u++)
            v[t * VEC + u] = 0.0f;
        if (c < C)
            gae_load_vec<VEC>(x + row * (size_t)ld + hc + c, &v[t * VEC]);
    }
}

// the first n of GAE_R neighbours' xl rows (the lane's columns) and attribute rows; the others zeros
template <int VEC, int T, int ED>
__device__ __forceinline__ void gae_load_rows(const float *__restrict__ xl, int ldl, const float *__restrict__ ea, const int (&j)[GAE_R],
                                              const int (&ei)[GAE_R], int n, int hc, int gl, int glog2, int C, bool avec,
                                              float (&xj)[GAE_R][T * VEC], float (&e)[GAE_R][ED])
{
#pragma unroll
    for (int r = 0; r < GAE_R; r++) {
#pragma unroll
        for (int c = 0; c < T * VEC; c++)
            xj[r][c] = 0.0f;
#pragma unroll
        for (int d = 0; d < ED; d++)
            e[r][d] = 0.0f;
        if (r < n) {
            gae_load_row<VEC, T>(xl, (size_t)j[r], ldl, hc, gl, glog2, C, xj[r]);
            gae_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e[r]);
        }
    }
}

// the lane's part of the score of one gathered row with attributes e: sum_c att_c * leaky_relu((xl_j[c] + xr_i[c]) + p_c),
// p_c = W_e[c] . e, d increasing (columns past the head: att = 0, W_e = 0)
template <int NC, int ED>
__device__ __forceinline__ float gae_score_part(const float (&xj)[NC], const float (&xr)[NC], const float (&att)[NC], const float (&wgt)[NC][ED],
                                                const float (&e)[ED], float slope)
{
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float p = 0.0f;
#pragma unroll
        for (int d = 0; d < ED; d++)
            p = fmaf(wgt[c][d], e[d], p);
        const float z = (xj[c] + xr[c]) + p;
        s = fmaf(att[c], z > 0.0f ? z : z * slope, s);
    }
    return s;
}

// one batch: the first n (1 .. GAE_R) of the loaded neighbour rows taken into the state and their attributes into the row's
// attribute sum -- the rule of the header (rows past n were loaded as zeros: + 0 changes no bit of asum, which is never -0)
template <int NC, int ED>
__device__ __forceinline__ void gae_take_batch(const float (&xj)[GAE_R][NC], const float (&e)[GAE_R][ED], int n, const float (&xr)[NC],
                                               const float (&att)[NC], const float (&wgt)[NC][ED], float slope, int glog2, float (&asum)[ED],
                                               GaeState<NC> &a)
{
    float s[GAE_R];
#pragma unroll
    for (int r = 0; r < GAE_R; r++)
        s[r] = gae_score_part<NC, ED>(xj[r], xr, att, wgt, e[r], slope);
#pragma unroll
    for (int r = 0; r < GAE_R; r++)
#pragma unroll
        for (int d = 0; d < ED; d++)
            asum[d] += e[r][d];
#pragma unroll
    for (int r = 0; r < GAE_R; r++)
        s[r] = gae_group_sum(s[r], glog2);
    float m1 = a.m;
#pragma unroll
    for (int r = 0; r < GAE_R; r++) {
        s[r] = r < n ? s[r] : -INFINITY;
        m1 = fmaxf(m1, s[r]);
    }
    // (m1 is finite: n >= 1 and a score is finite; a.m = -inf, the start of a row or of a piece, gives f = exp2(-inf) = 0)
    const float f = gae_exp(a.m - m1);
    float w[GAE_R];
#pragma unroll
    for (int r = 0; r < GAE_R; r++)
        w[r] = gae_exp(s[r] - m1);
    a.m = m1;
    a.l = fmaf(a.l, f, ((w[0] + w[1]) + w[2]) + w[3]);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = a.acc[c] * f;
#pragma unroll
        for (int r = 0; r < GAE_R; r++)
            t = fmaf(w[r], xj[r][c], t);
        a.acc[c] = t;
    }
}

// the self term, last: its attribute is the mean of the row's deg attribute rows (asum / deg; deg = 0: 0), projected as an edge's
template <int NC, int ED>
__device__ __forceinline__ void gae_take_self(const float (&xi)[NC], const float (&xr)[NC], const float (&att)[NC], const float (&wgt)[NC][ED],
                                              const float (&asum)[ED], int deg, float slope, int glog2, GaeState<NC> &a)
{
    const float fd = (float)max(deg, 1);
    float em[ED];
#pragma unroll
    for (int d = 0; d < ED; d++)
        em[d] = asum[d] / fd;
    const float s = gae_group_sum(gae_score_part<NC, ED>(xi, xr, att, wgt, em, slope), glog2);
    const float m1 = fmaxf(a.m, s);
    const float f = gae_exp(a.m - m1), w = gae_exp(s - m1);
    a.m = m1;
    a.l = fmaf(a.l, f, w);
#pragma unroll
    for (int c = 0; c < NC; c++)
        a.acc[c] = fmaf(w, xi[c], a.acc[c] * f);
}

// the CSR slots [k0, k1) taken into the state in batches of GAE_R, in slot order
template <int VEC, int T, int ED>
__device__ __forceinline__ void gae_piece(const float *__restrict__ xl, int ldl, const float *__restrict__ ea, const int32_t *__restrict__ col,
                                          const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int hc, int gl, int glog2, int C, bool avec,
                                          const float (&xr)[T * VEC], const float (&att)[T * VEC], const float (&wgt)[T * VEC][ED], float slope,
                                          float (&asum)[ED], GaeState<T * VEC> &a)
{
    for (int k = k0; k < k1; k += GAE_R) {
        int j[GAE_R], ei[GAE_R];
        float xj[GAE_R][T * VEC], e[GAE_R][ED];
        gae_load_slots(col, eid, k, k1, N, E, j, ei);
        gae_load_rows<VEC, T, ED>(xl, ldl, ea, j, ei, k1 - k, hc, gl, glog2, C, avec, xj, e);
        gae_take_batch<T * VEC, ED>(xj, e, min(k1 - k, GAE_R), xr, att, wgt, slope, glog2, asum, a);
    }
}

// row's start and in-degree from its node record, clamped into the E slots of col / eid
__device__ __forceinline__ void gae_row(const int4 *__restrict__ node_rec, int node, int E, int &rp0, int &deg)
{
    const int4 r0 = node_rec[2 * (size_t)node];
    rp0 = min(max(r0.x, 0), E);
    deg = min(max(r0.y, 0), E - rp0);
}

template <int NC>
__device__ __forceinline__ void gae_empty(GaeState<NC> &a)
{
    a.m = -INFINITY, a.l = 0.0f;
#pragma unroll
    for (int q = 0; q < NC; q++)
        a.acc[q] = 0.0f;
}

template <int VEC, int T, int ED>
__global__ __launch_bounds__(WG) void k_gatv2_edge_aggregate(const float *__restrict__ xl, int ldl, const float *__restrict__ xr, int ldr,
                                                              const float *__restrict__ attw, const float *__restrict__ bias,
                                                              const float *__restrict__ skip, float *__restrict__ out,
                                                              const float *__restrict__ ea, const float *__restrict__ we, int ldwe,
                                                              const int4 *__restrict__ node_rec, const int32_t *__restrict__ col,
                                                              const int32_t *__restrict__ eid, int N, int E, int w, int heads, int C, float slope,
                                                              int act, int glog2, int avec_i, int iters)
{
    constexpr int NC = T * VEC;
    __shared__ float s_part[WG * (NC + 2)]; // one round of a long row's pieces: [lane group][lane of the group][m, l, acc[NC]]
    __shared__ float s_asum[WG * ED];       // ... and the pieces' attribute sums: [lane group][ED] (at most WG lane groups)
    __shared__ int s_long[WG];              // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const bool avec = avec_i != 0;
    // the lane group's place in the grid: ONE head for its life, and its slot among the RS rows of a sweep (the launcher makes
    // RS >= 1; the at most heads - 1 lane groups past RS * heads stay idle)
    const int RS = ((int)gridDim.x * groups) / heads;
    const int gid = (int)blockIdx.x * groups + grp;
    const int slot = gid / heads;
    // step `it` of this lane group: its row and that row's record (node = N, degree 0 past the batch or past the last step)
    auto row_of = [&](int it, int &node, int &rp0, int &deg) {
        node = (it < iters && slot < RS) ? it * RS + slot : N;
        rp0 = 0, deg = 0;
        if (node < N)
            gae_row(node_rec, node, E, rp0, deg);
        else
            node = N;
    };
    // what a lane holds of a head (first column hc) for its columns: att and W_e's rows
    float att[NC], wgt[NC][ED];
    auto load_head = [&](int hc) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
            for (int u = 0; u < VEC; u++) {
                att[t * VEC + u] = c < C ? attw[hc + c + u] : 0.0f;
#pragma unroll
                for (int d = 0; d < ED; d++)
                    wgt[t * VEC + u][d] = c < C ? we[(size_t)(hc + c + u) * ldwe + d] : 0.0f;
            }
        }
    };
    auto finish = [&](int node, int hc, const GaeState<NC> &a) {
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
                    gae_load_vec<VEC>(skip + (size_t)node * w + hc + c, sk);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = gae_act(act, o[u]);
                gae_store_vec<VEC>(out + (size_t)node * w + hc + c, o);
            }
        }
    };
    const int hc_own = (gid % heads) * C;
    load_head(hc_own);
    // ---- rows of at most GAE_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first GAE_R slots of step it + 1
    // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
    // same in all lanes of a lane group (the cross-lane sums need the whole group)
    int n0, rp_0, dg_0, n1, rp_1, dg_1;
    int j0[GAE_R], e0[GAE_R];
    row_of(0, n0, rp_0, dg_0);
    gae_load_slots(col, eid, rp_0, rp_0 + (dg_0 <= GAE_CHUNK ? dg_0 : 0), N, E, j0, e0);
    row_of(1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int n2, rp_2, dg_2, j1[GAE_R], e1[GAE_R];
        row_of(it + 2, n2, rp_2, dg_2);
        gae_load_slots(col, eid, rp_1, rp_1 + (dg_1 <= GAE_CHUNK ? dg_1 : 0), N, E, j1, e1);
        any_long |= dg_0 > GAE_CHUNK;
        if (n0 < N && dg_0 <= GAE_CHUNK) {
            float xri[NC], xi[NC], xj[GAE_R][NC], e[GAE_R][ED], asum[ED];
            GaeState<NC> a;
            gae_load_rows<VEC, T, ED>(xl, ldl, ea, j0, e0, dg_0, hc_own, gl, glog2, C, avec, xj, e);
            gae_load_row<VEC, T>(xr, (size_t)n0, ldr, hc_own, gl, glog2, C, xri);
            gae_load_row<VEC, T>(xl, (size_t)n0, ldl, hc_own, gl, glog2, C, xi);
            gae_empty<NC>(a);
#pragma unroll
            for (int d = 0; d < ED; d++)
                asum[d] = 0.0f;
            if (dg_0 > 0)
                gae_take_batch<NC, ED>(xj, e, min(dg_0, GAE_R), xri, att, wgt, slope, glog2, asum, a);
            if (dg_0 > GAE_R)
                gae_piece<VEC, T, ED>(xl, ldl, ea, col, eid, rp_0 + GAE_R, rp_0 + dg_0, N, E, hc_own, gl, glog2, C, avec, xri, att, wgt, slope, asum, a);
            gae_take_self<NC, ED>(xi, xri, att, wgt, asum, dg_0, slope, glog2, a);
            finish(n0, hc_own, a);
        }
        n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < GAE_R; r++)
            j0[r] = j1[r], e0[r] = e1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE barrier
    if (!__syncthreads_or(any_long))
        return;
    for (int it = 0; it < iters; it++) {
        int node, rp0, deg;
        row_of(it, node, rp0, deg);
        const bool is_long = deg > GAE_CHUNK;
        if (!__syncthreads_or(is_long))
            continue;
        // the long items of this step, one after the other: pieces round-robin over the lane groups, partials through LDS
        if (gl == 0)
            s_long[grp] = is_long ? node : -1;
        __syncthreads();
        for (int g = 0; g < groups; g++) {
            const int ln = s_long[g];
            if (ln < 0)
                continue;
            const int hc = (((int)blockIdx.x * groups + g) % heads) * C; // (the owner's head)
            int lrp, ldeg;
            gae_row(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + GAE_CHUNK - 1) / GAE_CHUNK;
            float xri[NC], asum[ED];
            GaeState<NC> a; // (the owner's: the pieces in their order, then the self term; the others' copy is not used)
            load_head(hc);
            gae_load_row<VEC, T>(xr, (size_t)ln, ldr, hc, gl, glog2, C, xri);
            gae_empty<NC>(a);
#pragma unroll
            for (int d = 0; d < ED; d++)
                asum[d] = 0.0f;
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                GaeState<NC> part;
                float psum[ED];
                gae_empty<NC>(part);
#pragma unroll
                for (int d = 0; d < ED; d++)
                    psum[d] = 0.0f;
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gae_piece<VEC, T, ED>(xl, ldl, ea, col, eid, lrp + c * GAE_CHUNK, lrp + min((c + 1) * GAE_CHUNK, ldeg), N, E, hc, gl, glog2, C, avec,
                                          xri, att, wgt, slope, psum, part);
                float *sp = s_part + (size_t)threadIdx.x * (NC + 2);
                sp[0] = part.m, sp[1] = part.l;
#pragma unroll
                for (int q = 0; q < NC; q++)
                    sp[2 + q] = part.acc[q];
                if (gl == 0)
#pragma unroll
                    for (int d = 0; d < ED; d++)
                        s_asum[grp * ED + d] = psum[d];
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++) {
                        const float *pp = s_part + (size_t)((qq << glog2) + gl) * (NC + 2);
                        const float pm = pp[0], pl = pp[1];
                        const float m1 = fmaxf(a.m, pm); // (finite: pm is -- a piece that is read holds a slot)
                        const float fa = gae_exp(a.m - m1), fp = gae_exp(pm - m1);
                        a.m = m1;
                        a.l = fmaf(pl, fp, a.l * fa);
#pragma unroll
                        for (int q = 0; q < NC; q++)
                            a.acc[q] = fmaf(pp[2 + q], fp, a.acc[q] * fa);
#pragma unroll
                        for (int d = 0; d < ED; d++)
                            asum[d] += s_asum[qq * ED + d];
                    }
                }
                __syncthreads();
            }
            if (grp == g) {
                float xi[NC];
                gae_load_row<VEC, T>(xl, (size_t)ln, ldl, hc, gl, glog2, C, xi);
                gae_take_self<NC, ED>(xi, xri, att, wgt, asum, ldeg, slope, glog2, a);
                finish(ln, hc, a);
            }
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long item)
    }
}

hipError_t launch_gatv2_edge_aggregate(const BatchTables &t, const float *xl, int ldl, const float *xr, int ldr, const float *att,
                                       const float *bias, const float *skip, int act, int heads, float slope, const float *edge_attr, int edge_dim,
                                       const float *we, int ldwe, float *out, int width, hipStream_t s)
{
    if (heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH || width % heads != 0 || ldl < width || ldr < width ||
        edge_dim < 1 || edge_dim > GAE_MAX_EDGE_DIM || ldwe < edge_dim || (t.num_edges > 0 && edge_attr == nullptr) ||
        (uint64_t)std::max(t.num_nodes, 0) * (uint64_t)heads > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const int C = width / heads;
    const bool v4 = (C % 4 == 0) && (ldl % 4 == 0) && (ldr % 4 == 0) && (((uintptr_t)xl & 15) == 0) && (((uintptr_t)xr & 15) == 0) &&
                    (((uintptr_t)skip & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int avec = (edge_dim % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
    const int nvec = v4 ? C / 4 : C;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int N = t.num_nodes;
    auto launch = [&](auto vec, auto strides, auto ed) {
        auto kern = k_gatv2_edge_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(ed)::value>;
        // the grid is what is resident at once (the kernel's own occupancy, at most GAE_WG_PER_CU per CU).  A sweep of the grid
        // takes RS = grid * groups / heads rows (a lane group keeps one head), every lane group walks `iters` sweeps; the grid is
        // then cut down to what `iters` sweeps need.  grid * groups >= heads always: RS >= 1
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, GAE_WG_PER_CU);
        const int64_t min_grid = (heads + groups - 1) / groups;
        const int64_t max_grid = std::max<int64_t>((int64_t)occ.blocks * occ.cus, min_grid);
        const int64_t rs_max = max_grid * groups / heads;
        const int iters = (int)((N + rs_max - 1) / rs_max);
        const int64_t rs = (N + iters - 1) / iters; // rows a sweep must take
        const int grid = (int)std::max<int64_t>((rs * heads + groups - 1) / groups, min_grid);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, xl, ldl, xr, ldr, att, bias, skip, out, edge_attr, we, ldwe, t.node_rec, t.col, t.eid,
                           N, t.num_edges, width, heads, C, slope, act, glog2, avec, iters);
    };
    auto by_form = [&](auto ed) {
        if (v4)
            launch(IntTag<4>{}, IntTag<1>{}, ed); // (C / 4 <= 64: one stride)
        else if (C <= 64)
            launch(IntTag<1>{}, IntTag<1>{}, ed);
        else
            launch(IntTag<1>{}, IntTag<4>{}, ed); // (C <= 256: four strides of a wave)
    };
    switch (edge_dim) {
#define GNNB_GAE_ED(n) case n: by_form(IntTag<n>{}); break;
    GNNB_GAE_ED(1) GNNB_GAE_ED(2) GNNB_GAE_ED(3) GNNB_GAE_ED(4) GNNB_GAE_ED(5) GNNB_GAE_ED(6) GNNB_GAE_ED(7) GNNB_GAE_ED(8)
    GNNB_GAE_ED(9) GNNB_GAE_ED(10) GNNB_GAE_ED(11) GNNB_GAE_ED(12) GNNB_GAE_ED(13) GNNB_GAE_ED(14) GNNB_GAE_ED(15) GNNB_GAE_ED(16)
#undef GNNB_GAE_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
