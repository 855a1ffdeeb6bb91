// k_gat_edge.hip -- GAT (v1) with edge features: the per-edge score term, the per-destination softmax and the weighted sum in ONE
// pass over the edges (gnnb_gatconv_edge.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot
// path); wavefront = 64 lanes.
//
// k_gat_edge_aggregate (models.py _GATEConv: PyG's GATConv(concat=True, add_self_loops=True, edge_dim=d, fill_value='mean',
// residual=False)):
//   t_ij[h]  = ae[h] . e_ij                                                       e_ij = edge_attr[eid[slot]]  (COO row order)
//   s_ij[h]  = leaky_relu(ssrc_j[h] + sdst_i[h] + t_ij[h])                         j in N(i) u {i}
//   out_i[h] = act( sum_j softmax_j(s_ij[h]) * xl_j[h, :] + bias + skip_i )        softmax = exp(s - max) / (sum + 1e-16), as PyG
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid) of a GCN workspace: graph prep has dropped the explicit
// (v, v) edges -- their attribute rows are never read --, the kernel adds the one self term itself.  ae [heads, d] is att_edge folded
// into lin_edge at upload (gnnb_weights.h: gat_edge_fold): a_edge[h] . (W_e e)[h] = (A_edge W_e)[h, :] . e, so the edge attribute
// costs d FMAs per (edge, head) in front of k_gat_aggregate's add and leaky_relu -- no per-column score work, no cross-lane sum, no
// [E, width] term.  The self loop's attribute is the mean of the row's (PyG's fill_value='mean'); the term is linear, so
// t_ii[h] = (sum_j t_ij[h]) / in-degree: ONE float of state per (row, head), not a d-wide attribute sum.
//
// Work split, the three-deep walk, ATT_R, the long rows' second walk, the 16-byte / scalar forms: k_gat.hip's, unchanged.  What is
// this kernel's:
//   tables  = the slot records carry eid (row_load_slots(col, eid, ..)); the attribute row is edge_attr + eid * d, the same address
//             in every lane of a lane group: one request serves them.  It is read in pieces of 4 floats -- one 16-byte load when
//             d % 4 == 0 and edge_attr is aligned, scalar loads (none at or past d) otherwise -- and each piece is consumed into the
//             T * ATT_R accumulators t as it arrives: a lane never holds ATT_R * d attribute floats, only ATT_R * 4
//   ae      = staged in LDS once per workgroup, [GAT_MAX_HEADS][GATE_LDAE] with zeros past heads and d: 512 bytes, read 16 bytes
//             at a time at the stride's head.  d is a run-time loop bound (one instantiation per form and activation, as k_gat)
//   t       = fma(ae[h][d - 1], e[d - 1], ... fma(ae[h][0], e[0], 0))                                     -- d increasing
//   score   = z = (ssrc_j[h] + sdst_i[h]) + t; s = z > 0 ? z : z * slope
//   state   = starts from (-inf, 0, 0), and beside it tsum = 0 per stride: per batch tsum = (((tsum + t_0) + t_1) + t_2) + t_3 in slot
//             order (slots past the row's end take no part); a piece's tsum is parked beside its (m, l, acc) and added in piece
//             order, tsum += tsum_p
//   self    = LAST: t_ii = tsum / in-degree (0 at in-degree 0), known only behind the row; then one more step of the softmax:
//             m' = max(m, s_ii); f = exp(m - m'); e = exp(s_ii - m'); l = fma(l, f, e); acc_c = fma(e, xl_ic, acc_c * f)
//   out     = act((acc_c / (l + 1e-16) + bias_c) + skip_c); an absent term adds nothing
// A row without in-edges: f = exp(-inf) = 0, e = exp(0) = 1, l = 1, acc = xl_i, so out = act(xl_i + bias + skip_i) bit for bit.
// A column's bits depend on the batch and on VEC only: never on the grid, on G, or on heads beyond which scalars the column reads.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int GATE_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int GATE_MAX_EDGE_DIM = 16;
constexpr int GATE_LDAE = 16;     // row stride of the staged ae table: GATE_MAX_EDGE_DIM, whole 16-byte pieces

__device__ __forceinline__ float gate_score(float ssrc, float sdst, float t, float slope)
{
    const float z = (ssrc + sdst) + t;
    return z > 0.0f ? z : z * slope;
}

// the piece [q, q + 4) of the attribute row p of d floats: one 16-byte load, or scalar loads of what is below d and zeros behind
__device__ __forceinline__ void gate_load_piece(const float *__restrict__ p, int q, int d, bool avec, float (&e)[4])
{
    if (avec) {
        const float4 v = *reinterpret_cast<const float4 *>(p + q);
        e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; u++)
            e[u] = q + u < d ? p[q + u] : 0.0f;
    }
}

// ... of the first n of ATT_R edges, side by side; the others zeros (nothing is read for them)
__device__ __forceinline__ void gate_load_pieces(const float *__restrict__ ea, const int (&ei)[ATT_R], int n, int q, int d, bool avec,
                                                 float (&e)[ATT_R][4])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
#pragma unroll
        for (int u = 0; u < 4; u++)
            e[r][u] = 0.0f;
        if (r < n)
            gate_load_piece(ea + (size_t)ei[r] * d, q, d, avec, e[r]);
    }
}

// one piece taken into the edge terms of every stride: t = fma(ae[h][q + u], e[q + u], t), u increasing, nothing at or past d
template <int T>
__device__ __forceinline__ void gate_take_piece(const float *s_ae, const int (&hd)[T], int q, int d, const float (&e)[ATT_R][4], float (&tj)[T][ATT_R])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        const float4 a4 = *reinterpret_cast<const float4 *>(s_ae + hd[t] * GATE_LDAE + q);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (q + u < d)
#pragma unroll
                for (int r = 0; r < ATT_R; r++)
                    tj[t][r] = fmaf(a[u], e[r][u], tj[t][r]);
    }
}

// the first n of ATT_R neighbours: their xl rows (the lane's columns, per stride) and their source scores of the strides' heads, all
// loads issued side by side; then the edge terms t, the attribute rows' pieces loaded and consumed one after the other behind
// them (loads return in order: the first piece's wait is the rows' wait; a row's further pieces lie in the cache line the first
// brought).  Loading the first piece in front of the rows held 16 more floats across their issue: 136 VGPRs and 3 waves per
// SIMD in the 16-byte form against 111 and 4.  Neighbours at or past n: zeros
template <int VEC, int T>
__device__ __forceinline__ void gate_load(const float *__restrict__ xl, int ldl, const float *__restrict__ ssrc, int lds, const float *__restrict__ ea,
                                          int d, bool avec, const float *s_ae, const int (&j)[ATT_R], const int (&ei)[ATT_R], int n, int gl, int glog2,
                                          int w, const int (&hd)[T], float (&xj)[T][ATT_R][VEC], float (&sj)[T][ATT_R], float (&tj)[T][ATT_R])
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
            tj[t][r] = 0.0f;
            if (r < n) {
                if (c < w)
                    row_load_vec<VEC>(xl + (size_t)j[r] * ldl + c, xj[t][r]);
                sj[t][r] = ssrc[(size_t)j[r] * lds + hd[t]];
            }
        }
    }
    for (int q = 0; q < d; q += 4) {
        float e[ATT_R][4];
        gate_load_pieces(ea, ei, n, q, d, avec, e);
        gate_take_piece<T>(s_ae, hd, q, d, e, tj);
    }
}

// one batch: the first n (1 .. ATT_R) of the loaded neighbours taken into the states and their edge terms into tsum, stride by stride
template <int VEC, int T>
__device__ __forceinline__ void gate_take_batch(const float (&xj)[T][ATT_R][VEC], const float (&sj)[T][ATT_R], const float (&tj)[T][ATT_R], int n,
                                                const float (&sd)[T], float slope, float (&tsum)[T], AttState<VEC> (&a)[T])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        float s[ATT_R];
#pragma unroll
        for (int r = 0; r < ATT_R; r++) {
            s[r] = gate_score(sj[t][r], sd[t], tj[t][r], slope);
            tsum[t] = r < n ? tsum[t] + tj[t][r] : tsum[t];
        }
        att_softmax_batch<VEC>(s, n, xj[t], a[t]);
    }
}

// the CSR slots [k0, k1) taken into the states in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void gate_piece(const float *__restrict__ xl, int ldl, const float *__restrict__ ssrc, int lds, const float *__restrict__ ea,
                                           int d, bool avec, const float *s_ae, const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int k0,
                                           int k1, int N, int E, int gl, int glog2, int w, const int (&hd)[T], const float (&sd)[T], float slope,
                                           float (&tsum)[T], AttState<VEC> (&a)[T])
{
    for (int k = k0; k < k1; k += ATT_R) {
        int j[ATT_R], ei[ATT_R];
        float xj[T][ATT_R][VEC], sj[T][ATT_R], tj[T][ATT_R];
        row_load_slots(col, eid, k, k1, N, E, j, ei);
        gate_load<VEC, T>(xl, ldl, ssrc, lds, ea, d, avec, s_ae, j, ei, min(k1 - k, ATT_R), gl, glog2, w, hd, xj, sj, tj);
        gate_take_batch<VEC, T>(xj, sj, tj, min(k1 - k, ATT_R), sd, slope, tsum, a);
    }
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_gat_edge_aggregate(const float *__restrict__ xl, int ldl, const float *__restrict__ ssrc, int lds,
                                                            const float *__restrict__ sdst, int ldd, const float *__restrict__ bias,
                                                            const float *__restrict__ skip, float *__restrict__ out,
                                                            const float *__restrict__ ea, const float *__restrict__ ae, int ldae, int d,
                                                            const int4 *__restrict__ node_rec, const int32_t *__restrict__ col,
                                                            const int32_t *__restrict__ eid, int N, int E, int w, int heads, int C, float slope,
                                                            int glog2, int avec_i, int iters)
{
    constexpr int PS = WG * (VEC + 2);  // one stride's parked states: [lane of the workgroup][m, l, acc[VEC]]
    __shared__ float s_part[T * PS];    // one round of a long row's pieces, stride by stride
    __shared__ float s_tsum[T * WG];    // ... and the pieces' edge-term sums: [stride][lane of the workgroup]
    __shared__ int s_long[WG];          // per lane group: the long row of its step, or -1
    __shared__ __attribute__((aligned(16))) float s_ae[GAT_MAX_HEADS * GATE_LDAE]; // ae, zeros past heads and d
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const bool avec = avec_i != 0;
    for (int i = threadIdx.x; i < GAT_MAX_HEADS * GATE_LDAE; i += WG) {
        const int h = i / GATE_LDAE, k = i % GATE_LDAE;
        s_ae[i] = (h < heads && k < d) ? ae[(size_t)h * ldae + k] : 0.0f;
    }
    __syncthreads();
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
    // a row's loop invariants: sdst_i of the strides' heads, and the empty states
    auto begin = [&](int node, float (&sd)[T], float (&tsum)[T], AttState<VEC> (&a)[T]) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            sd[t] = sdst[(size_t)node * ldd + hd[t]];
            tsum[t] = 0.0f;
            a[t].clear();
        }
    };
    // the self term, last: its edge term is the mean of the row's deg edge terms (tsum / deg; deg = 0: 0)
    auto take_self = [&](int node, int deg, const float (&sd)[T], const float (&tsum)[T], AttState<VEC> (&a)[T]) {
        const float fd = (float)max(deg, 1);
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            float xi[VEC];
#pragma unroll
            for (int u = 0; u < VEC; u++)
                xi[u] = 0.0f;
            if (c < w)
                row_load_vec<VEC>(xl + (size_t)node * ldl + c, xi);
            const float si = ssrc[(size_t)node * lds + hd[t]];
            const float s = gate_score(si, sd[t], tsum[t] / fd, slope);
            const float m1 = fmaxf(a[t].m, s);
            const float f = att_exp(a[t].m - m1), e = att_exp(s - m1);
            a[t].m = m1;
            a[t].l = fmaf(a[t].l, f, e);
#pragma unroll
            for (int u = 0; u < VEC; u++)
                a[t].acc[u] = fmaf(e, xi[u], a[t].acc[u] * f);
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
            float sd[T], tsum[T], xj[T][ATT_R][VEC], sj[T][ATT_R], tj[T][ATT_R];
            AttState<VEC> a[T];
            gate_load<VEC, T>(xl, ldl, ssrc, lds, ea, d, avec, s_ae, j0, e0, min(dg_0, ATT_R), gl, glog2, w, hd, xj, sj, tj);
            begin(n0, sd, tsum, a);
            if (dg_0 > 0)
                gate_take_batch<VEC, T>(xj, sj, tj, min(dg_0, ATT_R), sd, slope, tsum, a);
            if (dg_0 > ATT_R)
                gate_piece<VEC, T>(xl, ldl, ssrc, lds, ea, d, avec, s_ae, col, eid, rp_0 + ATT_R, rp_0 + dg_0, N, E, gl, glog2, w, hd, sd, slope,
                                   tsum, a);
            take_self(n0, dg_0, sd, tsum, a);
            finish(n0, a);
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
            float sd[T], tsum[T];
            AttState<VEC> a[T]; // (the owner's: the pieces in their order, then the self term; the others' copy is not used)
            begin(ln, sd, tsum, a);
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                AttState<VEC> part[T];
                float psum[T];
#pragma unroll
                for (int t = 0; t < T; t++)
                    part[t].clear(), psum[t] = 0.0f;
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gate_piece<VEC, T>(xl, ldl, ssrc, lds, ea, d, avec, s_ae, col, eid, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N,
                                       E, gl, glog2, w, hd, sd, slope, psum, part);
#pragma unroll
                for (int t = 0; t < T; t++) {
                    att_park<VEC>(s_part + t * PS, part[t]);
                    s_tsum[t * WG + threadIdx.x] = psum[t];
                }
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++)
#pragma unroll
                        for (int t = 0; t < T; t++) {
                            att_merge<VEC>(s_part + t * PS, qq, gl, glog2, a[t]);
                            tsum[t] += s_tsum[t * WG + (qq << glog2) + gl];
                        }
                }
                __syncthreads();
            }
            if (grp == g) {
                take_self(ln, ldeg, sd, tsum, a);
                finish(ln, a);
            }
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
    }
}

hipError_t launch_gat_edge_aggregate(const BatchTables &t, const float *xl, int ldl, const float *ssrc, int lds, const float *sdst, int ldd,
                                     const float *bias, const float *skip, int act, int heads, float slope, const float *edge_attr, int edge_dim,
                                     const float *ae, int ldae, float *out, int width, hipStream_t s)
{
    if (heads < 1 || heads > GAT_MAX_HEADS || width < 1 || width > GAT_MAX_WIDTH || width % heads != 0 || ldl < width || lds < heads ||
        ldd < heads || edge_dim < 1 || edge_dim > GATE_MAX_EDGE_DIM || ldae < edge_dim || ae == nullptr ||
        (t.num_edges > 0 && edge_attr == nullptr) || (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const int C = width / heads;
    // the form by a head's columns (a lane's four columns share a head), the lane group by the ROW's
    AttForm fm = att_form(C, {xl, skip, out}, {ldl});
    fm.glog2 = lane_group_log2(fm.v4 ? width / 4 : width);
    fm.groups = WG >> fm.glog2;
    const int avec = (edge_dim % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
    const int steps = att_item_steps(t.num_nodes, 1, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, width, [&](auto vec, auto strides) {
            auto kern = k_gat_edge_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, GATE_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, xl, ldl, ssrc, lds, sdst, ldd, bias, skip, out, edge_attr, ae, ldae, edge_dim,
                               t.node_rec, t.col, t.eid, t.num_nodes, t.num_edges, width, heads, C, slope, fm.glog2, avec, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
