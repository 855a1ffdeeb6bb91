// k_gat.hip -- GAT (v1): the per-destination softmax of per-node scores and the weighted sum in ONE pass over the edges
// (gnnb_gatconv.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_gat_aggregate (models.py _GATConv: PyG's GATConv(concat=True, add_self_loops=True, edge_dim=None, residual=False)):
//   s_ij[h]  = leaky_relu(ssrc_j[h] + sdst_i[h])                                  j in N(i) u {i}
//   out_i[h] = act( sum_j softmax_j(s_ij[h]) * xl_j[h, :] + bias + skip_i )        softmax = exp(s - max) / (sum + 1e-16), as PyG
// on the CSR-by-destination tables of the prepared batch (node_rec, col) of a GCN workspace: graph prep has dropped the explicit
// (v, v) edges, the kernel adds the one self term itself.  ssrc_j[h] = att_src[h] . xl_j[h] and sdst_i[h] = att_dst[h] . xl_i[h] are
// per-NODE scalars and linear in x: the layer's GEMM delivers them as 2 heads extra columns (gnnb_weights.h: w_gat), so an edge
// costs one scalar load, one add and one leaky_relu per head in front of the softmax -- no per-column score work and no cross-lane
// sum.  The softmax is online (gnnb_attn.h's core), so neither the [E, heads] weights nor the [E, width] messages reach HBM.
//
// Work split: k_resgated_aggregate's.  A destination ROW (all its heads) is owned by a lane group of G = 2^glog2 lanes,
// G >= width / VEC, at most a wave; a lane owns VEC consecutive columns in each of T strides of G * VEC columns (T > 1: the scalar
// form at width > 64).  16-byte form (VEC = 4) when C = width / heads is a multiple of 4 -- a lane's four columns then share a head;
// width % 4 == 0 is not enough: width 24 with 8 heads is scalar -- and xl / skip / out and xl's stride are 16-byte aligned; scalar
// form otherwise.  The walk is gnnb_attn.h's: three deep, ATT_R = 4 neighbours in flight per batch (their row loads and their score
// loads all issued before the first is consumed), rows of more than ATT_CHUNK in-edges in a second walk through att_park /
// att_merge, non-temporal stores, the grid from att_grid.
//
// State.  One softmax state per stride of a lane, AttState<VEC>, T of them; the state's head is (its first column) / C.  Lanes of
// one head hold equal (m, l): each forms them from the same scalars in the same order, nothing is exchanged between lanes.  Every
// lane of a head loads the head's score itself: the lanes' addresses coincide, one request serves them (the alternative, one lane
// loading and a DPP broadcast, was not measured: DESIGN 8).
//
// Summation order: gnnb_attn.h's batch rule, piece rule and exp, per (row, head) -- att_softmax_batch, att_park and att_merge
// unchanged.  What is this kernel's:
//   score   = z = ssrc_j[h] + sdst_i[h]; s = z > 0 ? z : z * slope -- two roundings, no sum over columns
//   state   = starts from the self term, FIRST: m = s_ii, l = 1, acc = xl_i -- no row is ever empty; a long row's pieces are
//             merged onto it
//   out     = act((acc_c / (l + 1e-16) + bias_c) + skip_c); an absent term adds nothing; a row without in-edges is
//             act(xl_i + bias + skip_i) bit for bit (l + 1e-16 is 1)
// A column's bits depend on the batch and on VEC only: never on the grid, on G, or on heads beyond which scalar the column reads.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int GAT1_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)

__device__ __forceinline__ float gat1_score(float ssrc, float sdst, float slope)
{
    const float z = ssrc + sdst;
    return z > 0.0f ? z : z * slope;
}

// the first n of ATT_R neighbours: their xl rows (the lane's columns, per stride) and their source scores of the strides' heads,
// all loads issued side by side; the others zeros
template <int VEC, int T>
__device__ __forceinline__ void gat1_load(const float *__restrict__ xl, int ldl, const float *__restrict__ ssrc, int lds, const int (&j)[ATT_R], int n,
                                          int gl, int glog2, int w, const int (&hd)[T], float (&xj)[T][ATT_R][VEC], float (&sj)[T][ATT_R])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
#pragma unroll
            for (int u = 0; u < VEC; u++)
                xj[t][r][u] = 0.0f;
            sj[t][r] = 0.0f;
            if (r < n) {
                if (c < w)
                    row_load_vec<VEC>(xl + (size_t)j[r] * ldl + c, xj[t][r]);
                sj[t][r] = ssrc[(size_t)j[r] * lds + hd[t]];
            }
        }
    }
}

// one batch: the first n (1 .. ATT_R) of the loaded neighbours taken into the states, stride by stride
template <int VEC, int T>
__device__ __forceinline__ void gat1_take_batch(const float (&xj)[T][ATT_R][VEC], const float (&sj)[T][ATT_R], int n, const float (&sd)[T], float slope,
                                                AttState<VEC> (&a)[T])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        float s[ATT_R];
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            s[r] = gat1_score(sj[t][r], sd[t], slope);
        att_softmax_batch<VEC>(s, n, xj[t], a[t]);
    }
}

// the CSR slots [k0, k1) taken into the states in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void gat1_piece(const float *__restrict__ xl, int ldl, const float *__restrict__ ssrc, int lds, const int32_t *__restrict__ col,
                                           int k0, int k1, int N, int gl, int glog2, int w, const int (&hd)[T], const float (&sd)[T], float slope,
                                           AttState<VEC> (&a)[T])
{
    for (int k = k0; k < k1; k += ATT_R) {
        int j[ATT_R];
        float xj[T][ATT_R][VEC], sj[T][ATT_R];
        row_load_slots(col, k, k1, N, j);
        gat1_load<VEC, T>(xl, ldl, ssrc, lds, j, k1 - k, gl, glog2, w, hd, xj, sj);
        gat1_take_batch<VEC, T>(xj, sj, min(k1 - k, ATT_R), sd, slope, a);
    }
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_gat_aggregate(const float *__restrict__ xl, int ldl, const float *__restrict__ ssrc, int lds,
                                                       const float *__restrict__ sdst, int ldd, const float *__restrict__ bias,
                                                       const float *__restrict__ skip, float *__restrict__ out,
                                                       const int4 *__restrict__ node_rec, const int32_t *__restrict__ col, int N, int E, int w,
                                                       int C, float slope, int glog2, int iters)
{
    constexpr int PS = WG * (VEC + 2);  // one stride's parked states: [lane of the workgroup][m, l, acc[VEC]]
    __shared__ float s_part[T * PS];    // one round of a long row's pieces, stride by stride
    __shared__ int s_long[WG];          // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    // the head of each of the lane's strides (a stride past the width reads head 0's scores and stores nothing)
    int hd[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (gl + (t << glog2)) * VEC;
        hd[t] = c < w ? c / C : 0;
    }
    // step `it` of this lane group: its row and that row's record (node = N, degree 0 past the batch or past the last step)
    auto row_of = [&](int it, int &node, int &rp0, int &deg) {
        node = it < iters ? (it * (int)gridDim.x + (int)blockIdx.x) * groups + grp : N;
        rp0 = 0, deg = 0;
        if (node < N)
            row_record(node_rec, node, E, rp0, deg);
        else
            node = N;
    };
    // a row's loop invariants: sdst_i of the strides' heads, and the self-initialised states
    auto begin = [&](int node, float (&sd)[T], AttState<VEC> (&a)[T]) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            sd[t] = sdst[(size_t)node * ldd + hd[t]];
            const float si = ssrc[(size_t)node * lds + hd[t]];
#pragma unroll
            for (int u = 0; u < VEC; u++)
                a[t].acc[u] = 0.0f;
            if (c < w)
                row_load_vec<VEC>(xl + (size_t)node * ldl + c, a[t].acc);
            a[t].m = gat1_score(si, sd[t], slope);
            a[t].l = 1.0f;
        }
    };
    auto finish = [&](int node, const AttState<VEC> (&a)[T]) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < w) {
                const float den = a[t].l + 1e-16f;
                float o[VEC], sk[VEC];
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = a[t].acc[u] / den;
                if (bias != nullptr) // (an absent term adds nothing, not + 0: the row keeps its bits)
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += bias[c + u];
                if (skip != nullptr) {
                    row_load_vec<VEC>(skip + (size_t)node * w + c, sk);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = act_t<ACT>(o[u]);
                row_store_nt<VEC>(out + (size_t)node * w + c, o);
            }
        }
    };
    // ---- rows of at most ATT_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1 are
    // requested in front of the rows of step `it`, whose own record and slots arrived a step ago
    int n0, rp_0, dg_0, n1, rp_1, dg_1;
    int j0[ATT_R];
    row_of(0, n0, rp_0, dg_0);
    row_load_slots(col, rp_0, rp_0 + (dg_0 <= ATT_CHUNK ? dg_0 : 0), N, j0);
    row_of(1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int n2, rp_2, dg_2, j1[ATT_R];
        row_of(it + 2, n2, rp_2, dg_2);
        row_load_slots(col, rp_1, rp_1 + (dg_1 <= ATT_CHUNK ? dg_1 : 0), N, j1);
        any_long |= dg_0 > ATT_CHUNK;
        if (n0 < N && dg_0 <= ATT_CHUNK) {
            float sd[T], xj[T][ATT_R][VEC], sj[T][ATT_R];
            AttState<VEC> a[T];
            gat1_load<VEC, T>(xl, ldl, ssrc, lds, j0, dg_0, gl, glog2, w, hd, xj, sj);
            begin(n0, sd, a);
            if (dg_0 > 0)
                gat1_take_batch<VEC, T>(xj, sj, min(dg_0, ATT_R), sd, slope, a);
            if (dg_0 > ATT_R)
                gat1_piece<VEC, T>(xl, ldl, ssrc, lds, col, rp_0 + ATT_R, rp_0 + dg_0, N, gl, glog2, w, hd, sd, slope, a);
            finish(n0, a);
        }
        n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            j0[r] = j1[r];
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
        // the long rows of this step, one after the other: pieces round-robin over the lane groups, partials through LDS
        if (gl == 0)
            s_long[grp] = is_long ? node : -1;
        __syncthreads();
        for (int g = 0; g < groups; g++) {
            const int ln = s_long[g];
            if (ln < 0)
                continue;
            int lrp, ldeg;
            row_record(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + ATT_CHUNK - 1) / ATT_CHUNK;
            float sd[T];
            AttState<VEC> a[T]; // (the owner's: the self states, then the pieces in their order; the others' copy is not used)
            begin(ln, sd, a);
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                AttState<VEC> part[T];
#pragma unroll
                for (int t = 0; t < T; t++)
                    part[t].clear();
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gat1_piece<VEC, T>(xl, ldl, ssrc, lds, col, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, gl, glog2, w, hd, sd,
                                       slope, part);
#pragma unroll
                for (int t = 0; t < T; t++)
                    att_park<VEC>(s_part + t * PS, part[t]);
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++)
#pragma unroll
                        for (int t = 0; t < T; t++)
                            att_merge<VEC>(s_part + t * PS, qq, gl, glog2, a[t]); // (onto the self state: a.m is finite)
                }
                __syncthreads();
            }
            if (grp == g)
                finish(ln, a);
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
    }
}

hipError_t launch_gat_aggregate(const BatchTables &t, const float *xl, int ldl, const float *ssrc, int lds, const float *sdst, int ldd,
                                const float *bias, const float *skip, int act, int heads, float slope, float *out, int width, hipStream_t s)
{
    if (heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH || width % heads != 0 || ldl < width || lds < heads ||
        ldd < heads || (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const int C = width / heads;
    // the form by a head's columns (a lane's four columns share a head), the lane group by the ROW's
    AttForm fm = att_form(C, {xl, skip, out}, {ldl});
    fm.glog2 = lane_group_log2(fm.v4 ? width / 4 : width);
    fm.groups = WG >> fm.glog2;
    const int steps = att_item_steps(t.num_nodes, 1, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, width, [&](auto vec, auto strides) {
            auto kern = k_gat_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, GAT1_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, xl, ldl, ssrc, lds, sdst, ldd, bias, skip, out, t.node_rec, t.col, t.num_nodes,
                               t.num_edges, width, C, slope, fm.glog2, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
