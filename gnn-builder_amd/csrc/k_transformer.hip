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
// Work split, summation order, exp and the long rows' second walk: the contract at the top of gnnb_attn.h, on its dealing of
// items (item = row * heads + head).  What is this kernel's:
//   gathers = TWO per edge: the row that is scored (k_j) is not the row that is summed (v_j); the ATT_R x 2 row loads of a batch
//             are all issued before the first is consumed
//   kept    = q_i of the lane's columns -- as loaded, multiplied by nothing --, registers for the whole item; root and skip are
//             read in the epilogue
//   score   = per lane sum_c fma(q_c, k_jc, .); the group's sum times `scale`, ONE multiply per score ("dot, then scale")
//   state   = starts at (-inf, 0, 0): there is no self term; a long row's pieces are merged onto (-inf, 0, 0)
//   out     = act((acc_c / (l + 1e-16) + root_c) + skip_c); a row without in-edges takes nothing: act(root_c + skip_c) with root's
//             own bits (0 where root is absent)
// 16-byte form when q / k / v / root / skip / out and the four strides allow it.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int TF_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more items than that: grid stride)

// the first n of ATT_R neighbours' k and v rows (the lane's columns), all 2 ATT_R loads issued side by side; the others zeros
template <int VEC, int T>
__device__ __forceinline__ void tf_load_rows(const float *__restrict__ kx, int ldk, const float *__restrict__ vx, int ldv, const int (&j)[ATT_R], int n,
                                             int hc, int gl, int glog2, int C, float (&kj)[ATT_R][T * VEC], float (&vj)[ATT_R][T * VEC])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        if (r < n) {
            att_load_row<VEC, T>(kx, (size_t)j[r], ldk, hc, gl, glog2, C, kj[r]);
            att_load_row<VEC, T>(vx, (size_t)j[r], ldv, hc, gl, glog2, C, vj[r]);
        } else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                kj[r][c] = 0.0f, vj[r][c] = 0.0f;
        }
    }
}

// one batch: the first n (1 .. ATT_R) of the loaded neighbours taken into the state: their scores, then att_softmax_batch
template <int NC>
__device__ __forceinline__ void tf_take_batch(const float (&kj)[ATT_R][NC], const float (&vj)[ATT_R][NC], int n, const float (&q)[NC], float scale,
                                              int glog2, AttState<NC> &a)
{
    float s[ATT_R];
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        float p = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; c++)
            p = fmaf(q[c], kj[r][c], p);
        s[r] = p;
    }
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
        s[r] = att_group_sum(s[r], glog2) * scale;
    att_softmax_batch<NC>(s, n, vj, a);
}

// the CSR slots [k0, k1) taken into the state in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void tf_piece(const float *__restrict__ kx, int ldk, const float *__restrict__ vx, int ldv, const int32_t *__restrict__ col,
                                         int k0, int k1, int N, int hc, int gl, int glog2, int C, const float (&q)[T * VEC], float scale,
                                         AttState<T * VEC> &a)
{
    for (int k = k0; k < k1; k += ATT_R) {
        int j[ATT_R];
        float kj[ATT_R][T * VEC], vj[ATT_R][T * VEC];
        row_load_slots(col, k, k1, N, j);
        tf_load_rows<VEC, T>(kx, ldk, vx, ldv, j, k1 - k, hc, gl, glog2, C, kj, vj);
        tf_take_batch<T * VEC>(kj, vj, min(k1 - k, ATT_R), q, scale, glog2, a);
    }
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
            row_record(node_rec, node, E, rp0, deg);
        } else
            item = items;
    };
    auto finish = [&](int node, int hc, const AttState<NC> &a) {
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
                    row_load_vec<VEC>(root + (size_t)node * ldr + hc + c, rt);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] = took ? o[u] + rt[u] : rt[u];
                }
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
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1 are
    // requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
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
            float q[NC], kj[ATT_R][NC], vj[ATT_R][NC];
            AttState<NC> a;
            tf_load_rows<VEC, T>(kx, ldk, vx, ldv, j0, dg_0, hc, gl, glog2, C, kj, vj);
            att_load_row<VEC, T>(qx, (size_t)n0, ldq, hc, gl, glog2, C, q);
            a.clear();
            if (dg_0 > 0)
                tf_take_batch<NC>(kj, vj, min(dg_0, ATT_R), q, scale, glog2, a);
            if (dg_0 > ATT_R)
                tf_piece<VEC, T>(kx, ldk, vx, ldv, col, rp_0 + ATT_R, rp_0 + dg_0, N, hc, gl, glog2, C, q, scale, a);
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
            float q[NC];
            AttState<NC> a; // (the owner's: the pieces in their order onto the empty state; the others' copy is not used)
            att_load_row<VEC, T>(qx, (size_t)ln, ldq, hc, gl, glog2, C, q);
            a.clear();
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                AttState<NC> part;
                part.clear();
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    tf_piece<VEC, T>(kx, ldk, vx, ldv, col, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, hc, gl, glog2, C, q, scale,
                                     part);
                att_park<NC>(s_part, part);
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++)
                        att_merge<NC>(s_part, qq, gl, glog2, a);
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
    const AttForm fm = att_form(C, {q, k, v, root, skip, out}, {ldq, ldk, ldv, root != nullptr ? ldr : 0});
    const int steps = att_item_steps(t.num_nodes, heads, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, C, [&](auto vec, auto strides) {
            auto kern = k_transformer_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, TF_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, q, ldq, k, ldk, v, ldv, root, root != nullptr ? ldr : width, skip, out,
                               t.node_rec, t.col, t.num_nodes, t.num_edges, width, heads, C, scale, fm.glog2, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
