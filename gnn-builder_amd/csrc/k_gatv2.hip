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
// Work split, summation order, exp and the long rows' second walk: the contract at the top of gnnb_attn.h, on its dealing of
// items (item = row * heads + head).  What is this kernel's:
//   gathers = ONE per edge: the score is a function of the gathered row xl_j, which is also the row that is summed
//   kept    = att and xr_i of the lane's columns, registers for the whole item; bias and skip are read in the epilogue
//   score   = per lane sum_c fma(att_c, leaky_relu(xl_j[c] + xr_i[c]), .) (columns past the head: att = 0)
//   state   = starts from the self term, FIRST: m = s_ii, l = 1, acc = xl_i -- no row is ever empty; a long row's pieces are
//             merged onto it
//   out     = act((acc_c / (l + 1e-16) + bias_c) + skip_c)
// 16-byte form when xl / xr / skip / out and both strides allow it.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int GAT_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more items than that: grid stride)

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

// one batch: the first n (1 .. ATT_R) of the loaded neighbour rows taken into the state: their scores, then att_softmax_batch
template <int NC>
__device__ __forceinline__ void gat_take_batch(const float (&xj)[ATT_R][NC], int n, const float (&xr)[NC], const float (&att)[NC], float slope,
                                               int glog2, AttState<NC> &a)
{
    float s[ATT_R];
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
        s[r] = gat_score_part<NC>(xj[r], xr, att, slope);
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
        s[r] = att_group_sum(s[r], glog2);
    att_softmax_batch<NC>(s, n, xj, a);
}

// the first n of ATT_R neighbours' xl rows (the lane's columns); the others zeros
template <int VEC, int T>
__device__ __forceinline__ void gat_load_rows(const float *__restrict__ xl, int ldl, const int (&j)[ATT_R], int n, int hc, int gl, int glog2, int C,
                                              float (&xj)[ATT_R][T * VEC])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        if (r < n)
            att_load_row<VEC, T>(xl, (size_t)j[r], ldl, hc, gl, glog2, C, xj[r]);
        else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                xj[r][c] = 0.0f;
        }
    }
}

// the CSR slots [k0, k1) taken into the state in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void gat_piece(const float *__restrict__ xl, int ldl, const int32_t *__restrict__ col, int k0, int k1, int N, int hc, int gl,
                                          int glog2, int C, const float (&xr)[T * VEC], const float (&att)[T * VEC], float slope,
                                          AttState<T * VEC> &a)
{
    for (int k = k0; k < k1; k += ATT_R) {
        int j[ATT_R];
        float xj[ATT_R][T * VEC];
        row_load_slots(col, k, k1, N, j);
        gat_load_rows<VEC, T>(xl, ldl, j, k1 - k, hc, gl, glog2, C, xj);
        gat_take_batch<T * VEC>(xj, min(k1 - k, ATT_R), xr, att, slope, glog2, a);
    }
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
            row_record(node_rec, node, E, rp0, deg);
        } else
            item = items;
    };
    // an item's loop invariants: att of the lane's columns of its head, xr_i, and the self-initialised state
    auto begin = [&](int node, int hc, float (&att)[NC], float (&xri)[NC], AttState<NC> &a) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
            for (int u = 0; u < VEC; u++)
                att[t * VEC + u] = c < C ? attw[hc + c + u] : 0.0f;
        }
        att_load_row<VEC, T>(xr, (size_t)node, ldr, hc, gl, glog2, C, xri);
        att_load_row<VEC, T>(xl, (size_t)node, ldl, hc, gl, glog2, C, a.acc);
        a.m = att_group_sum(gat_score_part<NC>(a.acc, xri, att, slope), glog2);
        a.l = 1.0f;
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
                    o[u] = act_t<ACT>(o[u]);
                row_store_nt<VEC>(out + (size_t)node * w + hc + c, o);
            }
        }
    };
    // ---- rows of at most ATT_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1
    // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
    // same in all lanes of a lane group (the cross-lane sums need the whole group)
    int i0, n0, rp_0, dg_0, i1, n1, rp_1, dg_1;
    int j0[ATT_R];
    item_of(0, i0, n0, rp_0, dg_0);
    row_load_slots(col, rp_0, rp_0 + (dg_0 <= ATT_CHUNK ? dg_0 : 0), N, j0);
    item_of(1, i1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int i2, n2, rp_2, dg_2, j1[ATT_R];
        item_of(it + 2, i2, n2, rp_2, dg_2);
        row_load_slots(col, rp_1, rp_1 + (dg_1 <= ATT_CHUNK ? dg_1 : 0), N, j1);
        any_long |= dg_0 > ATT_CHUNK;
        if (i0 < items && dg_0 <= ATT_CHUNK) {
            const int hc = (i0 - n0 * heads) * C;
            float att[NC], xri[NC], xj[ATT_R][NC];
            AttState<NC> a;
            gat_load_rows<VEC, T>(xl, ldl, j0, dg_0, hc, gl, glog2, C, xj);
            begin(n0, hc, att, xri, a);
            if (dg_0 > 0)
                gat_take_batch<NC>(xj, min(dg_0, ATT_R), xri, att, slope, glog2, a);
            if (dg_0 > ATT_R)
                gat_piece<VEC, T>(xl, ldl, col, rp_0 + ATT_R, rp_0 + dg_0, N, hc, gl, glog2, C, xri, att, slope, a);
            finish(n0, hc, a);
        }
        i0 = i1, n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        i1 = i2, n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            j0[r] = j1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE barrier
    if (!__syncthreads_or(any_long))
        return;
    for (int it = 0; it < iters; it++) {
        int item, node, rp0, deg;
        item_of(it, item, node, rp0, deg);
        const bool is_long = deg > ATT_CHUNK;
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
            row_record(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + ATT_CHUNK - 1) / ATT_CHUNK;
            float att[NC], xri[NC];
            AttState<NC> a; // (the owner's: the self state, then the pieces in their order; the others' copy is not used)
            begin(ln, hc, att, xri, a);
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                AttState<NC> part;
                part.clear();
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gat_piece<VEC, T>(xl, ldl, col, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, hc, gl, glog2, C, xri, att, slope, part);
                att_park<NC>(s_part, part);
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++)
                        att_merge<NC>(s_part, qq, gl, glog2, a); // (onto the self state: a.m is finite)
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
    const AttForm fm = att_form(C, {xl, xr, skip, out}, {ldl, ldr});
    const int steps = att_item_steps(t.num_nodes, heads, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, C, [&](auto vec, auto strides) {
            auto kern = k_gatv2_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, GAT_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, xl, ldl, xr, ldr, att, bias, skip, out, t.node_rec, t.col, t.num_nodes,
                               t.num_edges, width, heads, C, slope, fm.glog2, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
