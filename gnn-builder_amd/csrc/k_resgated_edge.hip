// k_resgated_edge.hip -- ResGatedGraphConv with edge features: the per-edge sigmoid gate with its edge term and the gated sum of
// the value rows with theirs in ONE pass over the edges (gnnb_resgated_edge.h).  Part of libgnnb_hip.so (hand-written gfx950 /
// CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_resgated_edge_aggregate (models.py _ResGatedGraphEConv: PyG's ResGatedGraphConv(act=Sigmoid(), edge_dim=d, root_weight=True)).
// lin_key, lin_query and lin_value see [x | e_ij]; everything in front of the sigmoid is linear, so with W = [W_x | W_e]:
//   s_ijc = (k_ic + q_jc) + sum_d wg[c][d] e_ij[d]                            wg = W_ke + W_qe, an OPERAND
//   u_ijc = v_jc + sum_d wv[c][d] e_ij[d]                                     wv = W_ve, an operand of its own
//   out_ic = act( (sum_j sigmoid(s_ijc) * u_ijc + root_ic) + skip_ic )        j in N(i) -- the input's edges as they are
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid) of a workspace whose tables keep explicit (v, v)
// edges: such an edge is an ordinary edge and so is its attribute row.  The gate is nonlinear per COLUMN, so the edge term cannot be
// moved out of the per-edge work (k_transformer_edge's trick has no counterpart): it costs 2 edge_dim FMAs per (edge, column),
// formed here from the edge's attributes; neither projected [E, width] term, nor the gate, nor the gated message reaches HBM.
//
// Work split, the three-deep walk, ATT_R = 4 neighbours in flight, the long rows' second walk through LDS, the grid and the
// non-temporal stores: k_resgated.hip's, on gnnb_attn.h's lane groups with one head.  What is this kernel's:
//   gathers = THREE per edge: q_j, v_j and the attribute row at edge_attr + eid[slot] * edge_dim, the same address in every lane of
//             the group (16-byte pieces when edge_dim % 4 == 0 and edge_attr is aligned, scalar loads otherwise: the same values); a
//             batch's slot records carry eid; all 3 ATT_R loads of a batch are issued before the first is consumed
//   weights = wg and wv, staged in LDS once per workgroup as [edge_dim][2][width] -- a lane's columns of one d are one 16-byte
//             piece, consecutive lanes consecutive pieces: no bank conflict --, behind ONE barrier, and read once per (batch, d):
//             2 LDS reads feed 2 ATT_R NC FMAs.  Measured against k_gine's way, 2 NC edge_dim registers per lane read once per
//             workgroup: 9 % (edge_dim 4) and 7 % (edge_dim 16) faster at the C3t batch, same bits
//   order   = per (edge, column), fixed: s = k_c + q_jc; s = fma(wg[c][d], e[d], s), d increasing; u = v_jc;
//             u = fma(wv[c][d], e[d], u), d increasing; g = rcp(1 + exp2(s * -log2(e))) (k_resgated's gate: 0 and 1 exactly at
//             saturation, no NaN from finite inputs); acc = fma(g, u, acc)
// The batch rule (a slot past the row's end takes no part: its q, v and e are zeros, so u = 0 and fma(g, 0, acc) is acc), the piece
// rule and the epilogue rule (an absent term adds nothing; a row without in-edges is act(root_c + skip_c) with root's own bits) are
// k_resgated's.  With all-zero edge_attr every s and every u has k_resgated_aggregate's value: fma(w, 0, s) = s.  A repeat launch,
// another grid or other neighbours in the batch give a row the same bits; so do the two attribute forms.
// Instantiated over edge_dim, `act` at run time (k_transformer_edge's way).
#include "gnnb_attn.h"

namespace gnnb {

constexpr int RGE_WG_PER_CU = 8;   // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int RGE_LDS_AHEAD = 4;   // values of d whose staged weights are in flight at once

__device__ __forceinline__ float rge_gate(float s) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * -ATT_LOG2E)); }

__device__ __forceinline__ float rge_act(int act, float v)
{
    switch (act) {
    case GNNB_ACT_RELU: return act_t<GNNB_ACT_RELU>(v);
    case GNNB_ACT_GELU: return act_t<GNNB_ACT_GELU>(v);
    case GNNB_ACT_SIGMOID: return act_t<GNNB_ACT_SIGMOID>(v);
    case GNNB_ACT_TANH: return act_t<GNNB_ACT_TANH>(v);
    default: return v;
    }
}

// wg[.][d] and wv[.][d] of the lane's columns from the workgroup's LDS copy s[(2 d + m) w + column] (m = 0: wg, 1: wv)
template <int VEC, int T>
__device__ __forceinline__ void rge_weights(const float *s, int d, int gl, int glog2, int w, float (&g)[T * VEC], float (&v)[T * VEC])
{
#pragma unroll
    for (int t = 0; t < T; t++) {
        // (no branch: a lane past the width reads the last columns' weights; its rows are zeros and it stores nothing.  A guarded
        // read is a block of its own per d, which the scheduling fence of rge_take_batch cannot order)
        const int c = min((gl + (t << glog2)) * VEC, w - VEC);
        row_load_vec<VEC>(s + (2 * d) * w + c, &g[t * VEC]);
        row_load_vec<VEC>(s + (2 * d + 1) * w + c, &v[t * VEC]);
    }
}

// the first n of ATT_R neighbours' q and v rows (the lane's columns) and attribute rows (whole), all 3 ATT_R loads issued side by
// side; the others zeros
template <int VEC, int T, int ED>
__device__ __forceinline__ void rge_load_rows(const float *__restrict__ qx, int ldq, const float *__restrict__ vx, int ldv,
                                              const float *__restrict__ ea, const int (&j)[ATT_R], const int (&ei)[ATT_R], int n, int gl, int glog2,
                                              int w, bool avec, float (&qj)[ATT_R][T * VEC], float (&vj)[ATT_R][T * VEC], float (&e)[ATT_R][ED])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        if (r < n) {
            att_load_row<VEC, T>(qx, (size_t)j[r], ldq, 0, gl, glog2, w, qj[r]);
            att_load_row<VEC, T>(vx, (size_t)j[r], ldv, 0, gl, glog2, w, vj[r]);
            row_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e[r]);
        } else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                qj[r][c] = 0.0f, vj[r][c] = 0.0f;
#pragma unroll
            for (int d = 0; d < ED; d++)
                e[r][d] = 0.0f;
        }
    }
}

// one batch: the loaded neighbours taken into the accumulator -- the order of the header (s forms in qj, u in vj; the d loop is
// outermost so that a weight is fetched once per batch: every (edge, column) chain keeps its own order)
template <int VEC, int T, int ED>
__device__ __forceinline__ void rge_take_batch(float (&qj)[ATT_R][T * VEC], float (&vj)[ATT_R][T * VEC], const float (&e)[ATT_R][ED],
                                               const float (&k)[T * VEC], const float *W, int gl, int glog2, int w, float (&acc)[T * VEC])
{
    constexpr int NC = T * VEC;
#pragma unroll
    for (int r = 0; r < ATT_R; r++)
#pragma unroll
        for (int c = 0; c < NC; c++)
            qj[r][c] = k[c] + qj[r][c];
#pragma unroll
    for (int d = 0; d < ED; d++) {
        float g[NC], v[NC];
        // (the staged weights do not change during the walk, so left to itself the compiler issues all 2 ED reads of a batch up
        // front or reads them ONCE in front of the edge loop -- registers by another road: 256 VGPRs + 87 AGPRs at edge_dim
        // 16.  A compiler-only fence and a scheduling fence -- neither is an instruction -- in front of every RGE_LDS_AHEAD
        // values of d keep the reads where they are written: 256 + 12)
        if (d % RGE_LDS_AHEAD == 0) {
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_sched_barrier(0);
        }
        rge_weights<VEC, T>(W, d, gl, glog2, w, g, v);
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
#pragma unroll
            for (int c = 0; c < NC; c++) {
                qj[r][c] = fmaf(g[c], e[r][d], qj[r][c]);
                vj[r][c] = fmaf(v[c], e[r][d], vj[r][c]);
            }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = acc[c];
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            t = fmaf(rge_gate(qj[r][c]), vj[r][c], t);
        acc[c] = t;
    }
}

// the CSR slots [k0, k1) taken into the accumulator in batches of ATT_R, in slot order
template <int VEC, int T, int ED>
__device__ __forceinline__ void rge_piece(const float *__restrict__ qx, int ldq, const float *__restrict__ vx, int ldv, const float *__restrict__ ea,
                                          const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int gl,
                                          int glog2, int w, bool avec, const float (&k)[T * VEC], const float *W, float (&acc)[T * VEC])
{
    for (int s = k0; s < k1; s += ATT_R) {
        int j[ATT_R], ei[ATT_R];
        float qj[ATT_R][T * VEC], vj[ATT_R][T * VEC], e[ATT_R][ED];
        row_load_slots(col, eid, s, k1, N, E, j, ei);
        rge_load_rows<VEC, T, ED>(qx, ldq, vx, ldv, ea, j, ei, k1 - s, gl, glog2, w, avec, qj, vj, e);
        rge_take_batch<VEC, T, ED>(qj, vj, e, k, W, gl, glog2, w, acc);
    }
}

extern __shared__ __attribute__((aligned(16))) float rge_s_w[]; // [ED][2][w], 2 w ED floats (the launch's dynamic LDS)

template <int VEC, int T, int ED>
__global__ __launch_bounds__(WG) void k_resgated_edge_aggregate(const float *__restrict__ kx, int ldk, const float *__restrict__ qx, int ldq,
                                                                 const float *__restrict__ vx, int ldv, const float *__restrict__ root, int ldr,
                                                                 const float *__restrict__ skip, float *__restrict__ out,
                                                                 const float *__restrict__ ea, const float *__restrict__ wg, int ldwg,
                                                                 const float *__restrict__ wv, int ldwv, const int4 *__restrict__ node_rec,
                                                                 const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int N, int E,
                                                                 int w, int act, int glog2, int avec_i, int iters)
{
    constexpr int NC = T * VEC;
    __shared__ float s_part[WG * NC]; // one round of a long row's pieces: [lane group][lane of the group][acc[NC]]
    __shared__ int s_long[WG];        // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const bool avec = avec_i != 0;
    const float *W = rge_s_w;
    for (int i = threadIdx.x; i < w * ED; i += WG) {
        const int c = i / ED, d = i - c * ED;
        rge_s_w[(size_t)(2 * d) * w + c] = wg[(size_t)c * ldwg + d];
        rge_s_w[(size_t)(2 * d + 1) * w + c] = wv[(size_t)c * ldwv + d];
    }
    __syncthreads(); // (the one barrier of the short-row path: every batch below reads the staged weights)
    // step `it` of this lane group: its row and that row's record (node = N, degree 0 past the batch or past the last step)
    auto row_of = [&](int it, int &node, int &rp0, int &deg) {
        node = it < iters ? (it * (int)gridDim.x + (int)blockIdx.x) * groups + grp : N;
        rp0 = 0, deg = 0;
        if (node < N)
            row_record(node_rec, node, E, rp0, deg);
        else
            node = N;
    };
    auto finish = [&](int node, bool took, const float (&acc)[NC]) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < w) {
                float o[VEC], rt[VEC], sk[VEC];
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = acc[t * VEC + u];
                if (root != nullptr) { // (an absent term adds nothing, not + 0: the row keeps its bits)
                    row_load_vec<VEC>(root + (size_t)node * ldr + c, rt);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] = took ? o[u] + rt[u] : rt[u]; // (in-degree 0: root's own bits -- not 0 + root, which loses a -0)
                }
                if (skip != nullptr) {
                    row_load_vec<VEC>(skip + (size_t)node * w + c, sk);
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = rge_act(act, o[u]);
                row_store_nt<VEC>(out + (size_t)node * w + c, o);
            }
        }
    };
    // ---- rows of at most ATT_CHUNK in-edges, no further barrier.  Three steps are in flight per lane group, so that a step exposes
    // ONE memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1
    // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago
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
            float k[NC], qj[ATT_R][NC], vj[ATT_R][NC], e[ATT_R][ED], acc[NC];
            rge_load_rows<VEC, T, ED>(qx, ldq, vx, ldv, ea, j0, e0, dg_0, gl, glog2, w, avec, qj, vj, e);
            att_load_row<VEC, T>(kx, (size_t)n0, ldk, 0, gl, glog2, w, k);
#pragma unroll
            for (int c = 0; c < NC; c++)
                acc[c] = 0.0f;
            if (dg_0 > 0)
                rge_take_batch<VEC, T, ED>(qj, vj, e, k, W, gl, glog2, w, acc);
            if (dg_0 > ATT_R)
                rge_piece<VEC, T, ED>(qx, ldq, vx, ldv, ea, col, eid, rp_0 + ATT_R, rp_0 + dg_0, N, E, gl, glog2, w, avec, k, W, acc);
            finish(n0, dg_0 > 0, acc);
        }
        n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            j0[r] = j1[r], e0[r] = e1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE more barrier
    if (!__syncthreads_or(any_long))
        return;
    for (int it = 0; it < iters; it++) {
        int node, rp0, deg;
        row_of(it, node, rp0, deg);
        const bool is_long = deg > ATT_CHUNK;
        if (!__syncthreads_or(is_long))
            continue;
        // the long rows of this step, one after the other: pieces round-robin over the lane groups, partial sums through LDS
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
            float k[NC], acc[NC]; // (acc: the owner's, the pieces in their order onto 0; the others' copy is not used)
            att_load_row<VEC, T>(kx, (size_t)ln, ldk, 0, gl, glog2, w, k);
#pragma unroll
            for (int c = 0; c < NC; c++)
                acc[c] = 0.0f;
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                float part[NC];
#pragma unroll
                for (int u = 0; u < NC; u++)
                    part[u] = 0.0f;
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    rge_piece<VEC, T, ED>(qx, ldq, vx, ldv, ea, col, eid, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, E, gl,
                                                glog2, w, avec, k, W, part);
#pragma unroll
                for (int u = 0; u < NC; u++)
                    s_part[(size_t)threadIdx.x * NC + u] = part[u];
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked as zeros and are not read)
                    for (int qq = 0; qq < nq; qq++) {
                        const float *pp = s_part + (size_t)((qq << glog2) + gl) * NC;
#pragma unroll
                        for (int u = 0; u < NC; u++)
                            acc[u] += pp[u];
                    }
                }
                __syncthreads();
            }
            if (grp == g)
                finish(ln, true, acc);
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
    }
}

hipError_t launch_resgated_edge_aggregate(const BatchTables &t, const float *k, int ldk, const float *q, int ldq, const float *v, int ldv,
                                          const float *root, int ldr, const float *skip, int act, const float *edge_attr, int edge_dim,
                                          const float *wg, int ldwg, const float *wv, int ldwv, float *out, int width, hipStream_t s)
{
    if (width < 1 || width > RG_MAX_WIDTH || ldk < width || ldq < width || ldv < width || (root != nullptr && ldr < width) || edge_dim < 1 ||
        edge_dim > RGE_MAX_EDGE_DIM || wg == nullptr || wv == nullptr || ldwg < edge_dim || ldwv < edge_dim ||
        (t.num_edges > 0 && edge_attr == nullptr) || (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const AttForm fm = att_form(width, {k, q, v, root, skip, out}, {ldk, ldq, ldv, root != nullptr ? ldr : 0});
    const int avec = edge_dim % 4 == 0 && ((uintptr_t)edge_attr & 15) == 0 ? 1 : 0;
    const int steps = att_item_steps(t.num_nodes, 1, fm);
    auto by_ed = [&](auto ed) {
        constexpr int ED = decltype(ed)::value;
        const size_t lds = (size_t)2 * width * ED * sizeof(float); // (at most 32 KiB: width 256, edge_dim 16)
        att_by_form(fm, width, [&](auto vec, auto strides) {
            auto kern = k_resgated_edge_aggregate<decltype(vec)::value, decltype(strides)::value, ED>;
            // (att_grid's rule with the launch's dynamic LDS counted in the occupancy)
            const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, lds, RGE_WG_PER_CU);
            const int max_grid = std::max(occ.blocks * occ.cus, 1);
            const int iters = (steps + max_grid - 1) / max_grid;
            const int grid = (steps + iters - 1) / iters;
            hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), lds, s, k, ldk, q, ldq, v, ldv, root, root != nullptr ? ldr : width, skip, out,
                               edge_attr, wg, ldwg, wv, ldwv, t.node_rec, t.col, t.eid, t.num_nodes, t.num_edges, width, act, fm.glog2, avec,
                               iters);
        });
    };
    switch (edge_dim) {
#define GNNB_RGE_ED(n) case n: by_ed(IntTag<n>{}); break;
    GNNB_RGE_ED(1) GNNB_RGE_ED(2) GNNB_RGE_ED(3) GNNB_RGE_ED(4) GNNB_RGE_ED(5) GNNB_RGE_ED(6) GNNB_RGE_ED(7) GNNB_RGE_ED(8)
    GNNB_RGE_ED(9) GNNB_RGE_ED(10) GNNB_RGE_ED(11) GNNB_RGE_ED(12) GNNB_RGE_ED(13) GNNB_RGE_ED(14) GNNB_RGE_ED(15) GNNB_RGE_ED(16)
#undef GNNB_RGE_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
