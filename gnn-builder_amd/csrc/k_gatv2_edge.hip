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
// Work split, summation order, exp and the long rows' second walk: the contract at the top of gnnb_attn.h.  What is this kernel's:
//   dealing = its OWN: lane group gid = blockIdx.x * groups + grp of the grid keeps ONE head, gid % heads, for its whole life and
//             walks the rows it * RS + gid / heads (RS = grid * groups / heads rows per sweep), so that what a lane holds of a head
//             for its columns is loaded once per lane, not per item: W_e[c][0 .. edge_dim) and att[c] of the lane's T * VEC columns
//             live in REGISTERS, as in k_gine_aggregate (no bias: lin_edge has none).  The kernel is instantiated on edge_dim.  A
//             long row is taken with its OWNER's head: att, W_e and xr_i of that head are loaded again (the short rows are done
//             by then)
//   gathers = xl_j and the edge's attribute row, read at edge_attr + eid[slot] * edge_dim, the same address in every lane of the
//             group (16-byte pieces when edge_dim % 4 == 0 and edge_attr is aligned): a batch's slot records carry eid
//   p_c     = fma(W_e[c][d - 1], e[d - 1], ... fma(W_e[c][0], e[0], 0))                                      -- d increasing
//   score   = per lane sum_c fma(att_c, leaky_relu((xl_j[c] + xr_i[c]) + p_c), .)
//   state   = starts from (-inf, 0, 0), and beside it the row's attribute sum a[0 .. d) from 0: per batch
//             a[d] = (((a[d] + e_0[d]) + e_1[d]) + e_2[d]) + e_3[d] (slots past the row's end: + 0); a piece's sum is parked beside
//             its (m, l, acc) and added in piece order, a[d] += a_p[d]
//   self    = LAST: the self term's attribute is the row's mean, which is known only behind the row.  e_ii[d] = a[d] / deg (one
//             division per attribute; deg = 0: e_ii = 0), projected once as p above -- PyG's order of operations (mean of the
//             attributes, then lin_edge) --, then one more step of the softmax: m' = max(m, s_ii); f = exp(m - m');
//             e = exp(s_ii - m'); l = fma(l, f, e); acc_c = fma(e, xl_ic, acc_c * f)
//   out     = act((acc_c / (l + 1e-16) + bias_c) + skip_c), `act` at run time: the instantiations are over edge_dim
// A row without in-edges: f = exp(-inf) = 0, e = exp(0) = 1, l = 1, acc = xl_i, so out = act(xl_i + bias + skip_i) bit for bit.
// 16-byte form when xl / xr / skip / out and both strides allow it.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int GAE_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)

constexpr int GAE_MAX_EDGE_DIM = 16;

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

// the first n of ATT_R neighbours' xl rows (the lane's columns) and attribute rows; the others zeros
template <int VEC, int T, int ED>
__device__ __forceinline__ void gae_load_rows(const float *__restrict__ xl, int ldl, const float *__restrict__ ea, const int (&j)[ATT_R],
                                              const int (&ei)[ATT_R], int n, int hc, int gl, int glog2, int C, bool avec,
                                              float (&xj)[ATT_R][T * VEC], float (&e)[ATT_R][ED])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
#pragma unroll
        for (int c = 0; c < T * VEC; c++)
            xj[r][c] = 0.0f;
#pragma unroll
        for (int d = 0; d < ED; d++)
            e[r][d] = 0.0f;
        if (r < n) {
            att_load_row<VEC, T>(xl, (size_t)j[r], ldl, hc, gl, glog2, C, xj[r]);
            row_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e[r]);
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

// one batch: the first n (1 .. ATT_R) of the loaded neighbour rows taken into the state and their attributes into the row's
// attribute sum: their scores, the sum, then att_softmax_batch (rows past n were loaded as zeros: + 0 changes no bit of asum, which is never -0)
template <int NC, int ED>
__device__ __forceinline__ void gae_take_batch(const float (&xj)[ATT_R][NC], const float (&e)[ATT_R][ED], int n, const float (&xr)[NC],
                                               const float (&att)[NC], const float (&wgt)[NC][ED], float slope, int glog2, float (&asum)[ED],
                                               AttState<NC> &a)
{
    float s[ATT_R];
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
        s[r] = gae_score_part<NC, ED>(xj[r], xr, att, wgt, e[r], slope);
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
#pragma unroll
        for (int d = 0; d < ED; d++)
            asum[d] += e[r][d];
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
        s[r] = att_group_sum(s[r], glog2);
    att_softmax_batch<NC>(s, n, xj, a);
}

// the self term, last: its attribute is the mean of the row's deg attribute rows (asum / deg; deg = 0: 0), projected as an edge's
template <int NC, int ED>
__device__ __forceinline__ void gae_take_self(const float (&xi)[NC], const float (&xr)[NC], const float (&att)[NC], const float (&wgt)[NC][ED],
                                              const float (&asum)[ED], int deg, float slope, int glog2, AttState<NC> &a)
{
    const float fd = (float)max(deg, 1);
    float em[ED];
#pragma unroll
    for (int d = 0; d < ED; d++)
        em[d] = asum[d] / fd;
    const float s = att_group_sum(gae_score_part<NC, ED>(xi, xr, att, wgt, em, slope), glog2);
    const float m1 = fmaxf(a.m, s);
    const float f = att_exp(a.m - m1), w = att_exp(s - m1);
    a.m = m1;
    a.l = fmaf(a.l, f, w);
#pragma unroll
    for (int c = 0; c < NC; c++)
        a.acc[c] = fmaf(w, xi[c], a.acc[c] * f);
}

// the CSR slots [k0, k1) taken into the state in batches of ATT_R, in slot order
template <int VEC, int T, int ED>
__device__ __forceinline__ void gae_piece(const float *__restrict__ xl, int ldl, const float *__restrict__ ea, const int32_t *__restrict__ col,
                                          const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int hc, int gl, int glog2, int C, bool avec,
                                          const float (&xr)[T * VEC], const float (&att)[T * VEC], const float (&wgt)[T * VEC][ED], float slope,
                                          float (&asum)[ED], AttState<T * VEC> &a)
{
    for (int k = k0; k < k1; k += ATT_R) {
        int j[ATT_R], ei[ATT_R];
        float xj[ATT_R][T * VEC], e[ATT_R][ED];
        row_load_slots(col, eid, k, k1, N, E, j, ei);
        gae_load_rows<VEC, T, ED>(xl, ldl, ea, j, ei, k1 - k, hc, gl, glog2, C, avec, xj, e);
        gae_take_batch<T * VEC, ED>(xj, e, min(k1 - k, ATT_R), xr, att, wgt, slope, glog2, asum, a);
    }
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
            row_record(node_rec, node, E, rp0, deg);
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
    auto finish = [&](int node, int hc, const AttState<NC> &a) {
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
                    row_load_vec<VEC>(skip + (size_t)node * w + hc + c, sk);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = gae_act(act, o[u]);
                row_store_nt<VEC>(out + (size_t)node * w + hc + c, o);
            }
        }
    };
    const int hc_own = (gid % heads) * C;
    load_head(hc_own);
    // ---- rows of at most ATT_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1
    // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
    // same in all lanes of a lane group (the cross-lane sums need the whole group)
    int n0, rp_0, dg_0, n1, rp_1, dg_1;
    int j0[ATT_R], e0[ATT_R];
    row_of(0, n0, rp_0, dg_0);
    row_load_slots(col, eid, rp_0, rp_0 + (dg_0 <= ATT_CHUNK ? dg_0 : 0), N, E, j0, e0);
    row_of(1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int n2, rp_2, dg_2, j1[ATT_R], e1[ATT_R];
        row_of(it + 2, n2, rp_2, dg_2);
        row_load_slots(col, eid, rp_1, rp_1 + (dg_1 <= ATT_CHUNK ? dg_1 : 0), N, E, j1, e1);
        any_long |= dg_0 > ATT_CHUNK;
        if (n0 < N && dg_0 <= ATT_CHUNK) {
            float xri[NC], xi[NC], xj[ATT_R][NC], e[ATT_R][ED], asum[ED];
            AttState<NC> a;
            gae_load_rows<VEC, T, ED>(xl, ldl, ea, j0, e0, dg_0, hc_own, gl, glog2, C, avec, xj, e);
            att_load_row<VEC, T>(xr, (size_t)n0, ldr, hc_own, gl, glog2, C, xri);
            att_load_row<VEC, T>(xl, (size_t)n0, ldl, hc_own, gl, glog2, C, xi);
            a.clear();
#pragma unroll
            for (int d = 0; d < ED; d++)
                asum[d] = 0.0f;
            if (dg_0 > 0)
                gae_take_batch<NC, ED>(xj, e, min(dg_0, ATT_R), xri, att, wgt, slope, glog2, asum, a);
            if (dg_0 > ATT_R)
                gae_piece<VEC, T, ED>(xl, ldl, ea, col, eid, rp_0 + ATT_R, rp_0 + dg_0, N, E, hc_own, gl, glog2, C, avec, xri, att, wgt, slope, asum, a);
            gae_take_self<NC, ED>(xi, xri, att, wgt, asum, dg_0, slope, glog2, a);
            finish(n0, hc_own, a);
        }
        n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            j0[r] = j1[r], e0[r] = e1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE barrier
    if (!__syncthreads_or(any_long))
        return;
    for (int it = 0; it < iters; it++) {
        int node, rp0, deg;
        row_of(it, node, rp0, deg);
        const bool is_long = deg > ATT_CHUNK;
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
            row_record(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + ATT_CHUNK - 1) / ATT_CHUNK;
            float xri[NC], asum[ED];
            AttState<NC> a; // (the owner's: the pieces in their order, then the self term; the others' copy is not used)
            load_head(hc);
            att_load_row<VEC, T>(xr, (size_t)ln, ldr, hc, gl, glog2, C, xri);
            a.clear();
#pragma unroll
            for (int d = 0; d < ED; d++)
                asum[d] = 0.0f;
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                AttState<NC> part;
                float psum[ED];
                part.clear();
#pragma unroll
                for (int d = 0; d < ED; d++)
                    psum[d] = 0.0f;
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gae_piece<VEC, T, ED>(xl, ldl, ea, col, eid, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, E, hc, gl, glog2, C, avec,
                                          xri, att, wgt, slope, psum, part);
                att_park<NC>(s_part, part);
                if (gl == 0)
#pragma unroll
                    for (int d = 0; d < ED; d++)
                        s_asum[grp * ED + d] = psum[d];
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++) {
                        att_merge<NC>(s_part, qq, gl, glog2, a);
#pragma unroll
                        for (int d = 0; d < ED; d++)
                            asum[d] += s_asum[qq * ED + d];
                    }
                }
                __syncthreads();
            }
            if (grp == g) {
                float xi[NC];
                att_load_row<VEC, T>(xl, (size_t)ln, ldl, hc, gl, glog2, C, xi);
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
    const AttForm fm = att_form(C, {xl, xr, skip, out}, {ldl, ldr});
    const int avec = (edge_dim % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
    const int groups = fm.groups;
    const int N = t.num_nodes;
    auto by_ed = [&](auto ed) {
        att_by_form(fm, C, [&](auto vec, auto strides) {
            auto kern = k_gatv2_edge_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(ed)::value>;
            // the grid is what is resident at once (the kernel's own occupancy, at most GAE_WG_PER_CU per CU).  A sweep of the grid
            // takes RS = grid * groups / heads rows (a lane group keeps one head), every lane group walks `iters` sweeps; the grid
            // is then cut down to what `iters` sweeps need.  grid * groups >= heads always: RS >= 1
            const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, GAE_WG_PER_CU);
            const int64_t min_grid = (heads + groups - 1) / groups;
            const int64_t max_grid = std::max<int64_t>((int64_t)occ.blocks * occ.cus, min_grid);
            const int64_t rs_max = max_grid * groups / heads;
            const int iters = (int)((N + rs_max - 1) / rs_max);
            const int64_t rs = (N + iters - 1) / iters; // rows a sweep must take
            const int grid = (int)std::max<int64_t>((rs * heads + groups - 1) / groups, min_grid);
            hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, xl, ldl, xr, ldr, att, bias, skip, out, edge_attr, we, ldwe, t.node_rec, t.col,
                               t.eid, N, t.num_edges, width, heads, C, slope, act, fm.glog2, avec, iters);
        });
    };
    switch (edge_dim) {
#define GNNB_GAE_ED(n) case n: by_ed(IntTag<n>{}); break;
    GNNB_GAE_ED(1) GNNB_GAE_ED(2) GNNB_GAE_ED(3) GNNB_GAE_ED(4) GNNB_GAE_ED(5) GNNB_GAE_ED(6) GNNB_GAE_ED(7) GNNB_GAE_ED(8)
    GNNB_GAE_ED(9) GNNB_GAE_ED(10) GNNB_GAE_ED(11) GNNB_GAE_ED(12) GNNB_GAE_ED(13) GNNB_GAE_ED(14) GNNB_GAE_ED(15) GNNB_GAE_ED(16)
#undef GNNB_GAE_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
