// gnnb_attn.h -- what the attention aggregates share: k_gatv2_aggregate (k_gatv2.hip), k_gatv2_edge_aggregate (k_gatv2_edge.hip)
// and k_transformer_aggregate (k_transformer.hip) compute the online softmax of a destination row's scores fused with the weighted
// sum of the gathered rows.  Here, once: their contract (below), the softmax core -- the batch rule (att_softmax_batch) and a long
// row's park / merge (att_park, att_merge) --, the device primitives, and the host side's launch plan.  A unit keeps its formulae
// (its score, its self term, its epilogue) and its two walks -- written to this contract; one walk over a policy per kernel gave
// the same bits and was slower, DESIGN 3.2f -- and states in its header only where it differs.  (The row-walk primitives that
// k_gine.hip and k_pna_edge.hip use as well -- row_load_vec, row_store_nt, row_load_attr, row_load_slots, row_record -- are in
// gnnb_device.h.  Moving those left k_gine's and k_pna_edge's kernels the same machine code, for which row_store_nt takes its
// values as an array, not as a pointer: the pointer form changes k_pna_edge_aggregate<4, *>.)
//
// Work split.  An ITEM = (destination row, head) is owned by a lane group of G = 2^glog2 lanes, G >= C / VEC (C = width / heads
// columns per head), at most a wave; a lane owns VEC consecutive columns of the head in each of T strides of G * VEC columns
// (T > 1: the scalar form at C > 64).  A lane group holds columns of ONE head: the cross-lane sum of the score partials runs over
// the whole group, lanes past the head's columns add 0, and nothing can mix two heads whatever C / VEC is (3 lanes of 4 at C = 12,
// 65 columns over two strides of 64 at C = 65).  16-byte form (VEC = 4) when C % 4 == 0 and every row operand and stride is
// 16-byte aligned, scalar form (VEC = 1) otherwise (att_form).  The grid is cut from the kernel's own occupancy, at most the
// unit's *_WG_PER_CU workgroups per CU; every lane group walks its steps with a grid stride.  Which (row, head) a step of a lane
// group is: item = row * heads + head over the lane groups of the grid (att_item_steps, att_grid), unless a unit deals its own.
// What a lane keeps for an item is registers for the whole item.  ATT_R neighbours are in flight per batch: all their row loads
// are issued before the first is consumed.  The walk is three deep (record of step it + 2, slots of step it + 1, rows of step
// `it`).  Scores are summed across the lanes with DPP (inside 16 lanes) and wave shuffles (beyond): no LDS on the short-row path.
// Stores are non-temporal.
//
// Summation order (fixed: it depends on the batch and on the form -- VEC and G set how a score is split over lanes --, never on
// the grid or on which workgroup took an item):
//   score  = the unit's: per lane a sum over its columns, stride by stride, column increasing; the lanes' partials added in a
//            butterfly (distance 1, 2, 4, ... G / 2)
//   state  = (m, l, acc): the unit says what the owner's first one is -- a self term, or the empty state (-inf, 0, 0)
//   batch  = ATT_R = 4 consecutive CSR slots: m' = max(m, s_0 .. s_3); f = exp(m - m'); e_r = exp(s_r - m');
//            l = fma(l, f, ((e_0 + e_1) + e_2) + e_3) ; acc_c = fma(e_3, x_3c, fma(e_2, x_2c, fma(e_1, x_1c, fma(e_0, x_0c, acc_c * f))))
//            (slots past the row's end take no part: s = -inf, e = 0; m = -inf in front of a first batch gives f = exp2(-inf) = 0)
//   row    = of at most ATT_CHUNK = 64 in-edges: its batches in slot order onto the first state.  Longer (a hub): pieces of 64
//            slots, each piece's batches in slot order onto (-inf, 0, 0); the pieces merged in piece order onto the first state:
//            m' = max(m, m_p); l = fma(l_p, exp(m_p - m'), l * exp(m - m')); acc likewise
//   out    = the unit's epilogue: acc_c / (l + 1e-16), then its own terms; an absent term adds nothing, not + 0
// exp(x) is the hardware's exp2 of x * log2(e) (v_exp_f32, 1 ulp): the weights that matter have |x| small, where the scaled
// argument's rounding is a relative error of |x| * 2^-24 in the weight (tests/test_hip_gatv2.py holds it to the project's budget).
// Degree skew: a row of more than ATT_CHUNK in-edges is not walked by its own lane group.  The workgroup's lane groups take its
// pieces round-robin, park (m, l, acc) per piece in LDS and the owner merges them in piece order -- the rule above.  Long rows are
// taken in a second walk behind the short ones: a workgroup without one pays ONE barrier.
#ifndef GNNB_ATTN_H
#define GNNB_ATTN_H
#include <initializer_list>

#include "gnnb_device.h"

namespace gnnb {

constexpr int ATT_CHUNK = 64;    // CSR slots per piece of a long row
constexpr int ATT_R = 4;         // neighbours in flight per lane group (one batch of the online softmax)
constexpr float ATT_LOG2E = 1.44269504088896340736f;

__device__ __forceinline__ float att_exp(float x) { return __builtin_amdgcn_exp2f(x * ATT_LOG2E); }

// the sum of x over the 2^glog2 lanes of a lane group (aligned in the wave), the same bits in every lane: a butterfly of distance
// 1, 2 (quad permutes), 4, 8 (the half-row and row mirrors: every lane of the 4 / 8 lanes mirrored onto holds the same partial),
// 16, 32 (wave shuffles).  Every lane of the group must be active
__device__ __forceinline__ float att_group_sum(float x, int glog2)
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
struct AttState {
    float m, l, acc[NC];
    __device__ __forceinline__ void clear()
    {
        m = -INFINITY, l = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++)
            acc[c] = 0.0f;
    }
};

// the lane's columns of row `row` of x (row stride ld, the head's first column at hc): stride t holds columns
// [(gl + t G) VEC, + VEC) of the head where that is below C, zeros elsewhere
template <int VEC, int T>
__device__ __forceinline__ void att_load_row(const float *__restrict__ x, size_t row, int ld, int hc, int gl, int glog2, int C, float (&v)[T * VEC])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
        for (int u = 0; u < VEC; u++)
            v[t * VEC + u] = 0.0f;
        if (c < C)
            row_load_vec<VEC>(x + row * (size_t)ld + hc + c, &v[t * VEC]);
    }
}

// one batch: the first n (1 .. ATT_R) of the group-summed scores s and of the rows that are summed, taken into the state -- the
// batch rule of the header
template <int NC>
__device__ __forceinline__ void att_softmax_batch(float (&s)[ATT_R], int n, const float (&rows)[ATT_R][NC], AttState<NC> &a)
{
    float m1 = a.m;
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        s[r] = r < n ? s[r] : -INFINITY;
        m1 = fmaxf(m1, s[r]);
    }
    // (m1 is finite: n >= 1 and a score is finite; a.m = -inf, the empty state, gives f = exp2(-inf) = 0)
    const float f = att_exp(a.m - m1);
    float e[ATT_R];
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
        e[r] = att_exp(s[r] - m1);
    a.m = m1;
    a.l = fmaf(a.l, f, ((e[0] + e[1]) + e[2]) + e[3]);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = a.acc[c] * f;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            t = fmaf(e[r], rows[r][c], t);
        a.acc[c] = t;
    }
}

// a piece's state parked by its lane: s_part is [lane of the workgroup][m, l, acc[NC]], WG * (NC + 2) floats
template <int NC>
__device__ __forceinline__ void att_park(float *s_part, const AttState<NC> &p)
{
    float *sp = s_part + (size_t)threadIdx.x * (NC + 2);
    sp[0] = p.m, sp[1] = p.l;
#pragma unroll
    for (int u = 0; u < NC; u++)
        sp[2 + u] = p.acc[u];
}

// ... and the piece that lane group q parked merged onto a (a piece that is read holds a slot: its m is finite, so is m1;
// a.m = -inf gives fa = 0)
template <int NC>
__device__ __forceinline__ void att_merge(const float *s_part, int q, int gl, int glog2, AttState<NC> &a)
{
    const float *pp = s_part + (size_t)((q << glog2) + gl) * (NC + 2);
    const float pm = pp[0], pl = pp[1];
    const float m1 = fmaxf(a.m, pm);
    const float fa = att_exp(a.m - m1), fp = att_exp(pm - m1);
    a.m = m1;
    a.l = fmaf(pl, fp, a.l * fa);
#pragma unroll
    for (int u = 0; u < NC; u++)
        a.acc[u] = fmaf(pp[2 + u], fp, a.acc[u] * fa);
}

// ---- the launch plan (host)
// the form of a launch: 16-byte accesses when a head's C columns, every row stride and every operand's address allow them (an
// absent operand, nullptr, allows them), and the lane group of that form
struct AttForm {
    bool v4;
    int glog2, groups;
};
inline AttForm att_form(int C, std::initializer_list<const void *> operands, std::initializer_list<int> strides)
{
    bool v4 = C % 4 == 0;
    for (const void *p : operands)
        v4 = v4 && ((uintptr_t)p & 15) == 0;
    for (int ld : strides)
        v4 = v4 && ld % 4 == 0;
    const int glog2 = lane_group_log2(v4 ? C / 4 : C);
    return AttForm{v4, glog2, WG >> glog2};
}

// calls f(IntTag<VEC>{}, IntTag<T>{}) with the instantiation of the form
template <class F>
inline void att_by_form(const AttForm &fm, int C, F &&f)
{
    if (fm.v4)
        f(IntTag<4>{}, IntTag<1>{}); // (C / 4 <= 64: one stride)
    else if (C <= 64)
        f(IntTag<1>{}, IntTag<1>{});
    else
        f(IntTag<1>{}, IntTag<4>{}); // (C <= 256: four strides of a wave)
}

// the steps of a walk that deals items: a step = `groups` items, one per lane group of a workgroup
inline int att_item_steps(int num_nodes, int heads, const AttForm &fm)
{
    return (int)(((int64_t)num_nodes * heads + fm.groups - 1) / fm.groups);
}

// the grid is what is resident at once (the kernel's own occupancy, at most wg_per_cu -- the unit's own constant -- per CU):
// every workgroup walks `iters` steps, the steps of one sweep side by side in memory
struct AttGrid {
    int grid, iters;
};
template <class K>
inline AttGrid att_grid(K kern, int steps, int wg_per_cu)
{
    const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, wg_per_cu);
    const int max_grid = std::max(occ.blocks * occ.cus, 1);
    const int iters = (steps + max_grid - 1) / max_grid;
    return AttGrid{(steps + iters - 1) / iters, iters};
}

} // namespace gnnb
#endif
