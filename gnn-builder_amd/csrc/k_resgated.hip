// k_resgated.hip -- ResGatedGraphConv: the per-edge sigmoid gate and the gated sum of the value rows in ONE pass over the edges
// (gnnb_resgated.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_resgated_aggregate (models.py _ResGatedGraphConv: PyG's ResGatedGraphConv(act=Sigmoid(), edge_dim=None, root_weight=True)):
//   g_ijc = 1 / (1 + exp(-(k_ic + q_jc)))                                     j in N(i) -- the input's edges as they are
//   out_ic = act( (sum_j g_ijc * v_jc + root_ic) + skip_ic )
// on the CSR-by-destination tables of the prepared batch (node_rec, col) of a workspace whose tables keep explicit (v, v) edges
// (any but a GCN description's): no self term is added and none is removed, a row without in-edges gets root_i alone.  The gate is
// per COLUMN: there is no score, no cross-lane sum, no running max or sum and no head -- the attention aggregates' row walk
// (gnnb_attn.h) with the softmax state removed.  Neither the gathered q_j, nor the gate, nor the gated message [E, width] ever
// reaches HBM.
//
// Work split.  A destination row is owned by a lane group of G = 2^glog2 lanes, G >= width / VEC, at most a wave; a lane owns VEC
// consecutive columns in each of T strides of G * VEC columns (T > 1: the scalar form at width > 64) and keeps k_i of its columns
// and its accumulator in registers for the whole row.  16-byte form (VEC = 4) when width % 4 == 0 and every row operand and stride
// is 16-byte aligned, scalar form otherwise (att_form with one head of `width` columns).  The grid is cut from the kernel's own
// occupancy (att_grid), at most RG_WG_PER_CU workgroups per CU; every lane group walks its steps with a grid stride, three deep
// (record of step it + 2, slots of step it + 1, rows of step `it`).  ATT_R = 4 neighbours are in flight per batch: their 2 ATT_R
// row loads (q_j, v_j) are all issued before the first is consumed.  Stores are non-temporal.
//
// Gate.  s = k_c + q_jc forms first, in fp32; g = rcp(1 + exp2(s * -log2(e))) with the hardware's v_exp_f32 and v_rcp_f32 (1 ulp
// each).  The scaled argument's rounding is a relative error of |s| * 2^-24 in exp(-s), which reaches the gate times g (1 - g):
// at most 0.23 * 2^-24 absolute (tests/test_hip_resgated.py holds the whole to the project's budget).  Saturation is clean:
// s = -200 gives exp2(+288) = inf, 1 + inf = inf and rcp(inf) = 0 exactly; s = +200 gives exp2(-288) = 0 and rcp(1) = 1 exactly; no
// inf - inf and no 0 * inf is formed, so a finite input gives no NaN.
//
// Summation order (fixed: it depends on the batch and on the form, never on the grid or on which workgroup took a row):
//   batch = ATT_R = 4 consecutive CSR slots: acc_c = fma(g_3, v_3c, fma(g_2, v_2c, fma(g_1, v_1c, fma(g_0, v_0c, acc_c))))
//           (slots past the row's end take no part: their q and v are zeros, and fma(0.5, 0, acc) is acc)
//   row   = of at most ATT_CHUNK = 64 in-edges: its batches in slot order onto 0.  Longer (a hub): pieces of 64 slots taken
//           round-robin by the workgroup's lane groups in a second walk behind the short rows (gnnb_attn.h's scheme), each
//           piece's batches in slot order onto 0, parked in LDS; the owner adds the pieces in piece order onto 0 -- a plain sum
//   out   = act((acc_c + root_c) + skip_c); an absent term adds nothing, not + 0; a row without in-edges takes nothing:
//           act(root_c + skip_c) with root's own bits (0 where root is absent)
// A repeat launch, another grid or other neighbours in the batch give a row the same bits.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int RG_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)

__device__ __forceinline__ float rg_gate(float s) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * -ATT_LOG2E)); }

// the first n of ATT_R neighbours' q and v rows (the lane's columns), all 2 ATT_R loads issued side by side; the others zeros
template <int VEC, int T>
__device__ __forceinline__ void rg_load_rows(const float *__restrict__ qx, int ldq, const float *__restrict__ vx, int ldv, const int (&j)[ATT_R], int n,
                                             int gl, int glog2, int w, float (&qj)[ATT_R][T * VEC], float (&vj)[ATT_R][T * VEC])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        if (r < n) {
            att_load_row<VEC, T>(qx, (size_t)j[r], ldq, 0, gl, glog2, w, qj[r]);
            att_load_row<VEC, T>(vx, (size_t)j[r], ldv, 0, gl, glog2, w, vj[r]);
        } else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                qj[r][c] = 0.0f, vj[r][c] = 0.0f;
        }
    }
}

// one batch: the loaded neighbours taken into the accumulator -- the batch rule of the header (a slot past the row's end adds 0)
template <int NC>
__device__ __forceinline__ void rg_take_batch(const float (&qj)[ATT_R][NC], const float (&vj)[ATT_R][NC], const float (&k)[NC], float (&acc)[NC])
{
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = acc[c];
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            t = fmaf(rg_gate(k[c] + qj[r][c]), vj[r][c], t);
        acc[c] = t;
    }
}

// the CSR slots [k0, k1) taken into the accumulator in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void rg_piece(const float *__restrict__ qx, int ldq, const float *__restrict__ vx, int ldv, const int32_t *__restrict__ col,
                                         int k0, int k1, int N, int gl, int glog2, int w, const float (&k)[T * VEC], float (&acc)[T * VEC])
{
    for (int s = k0; s < k1; s += ATT_R) {
        int j[ATT_R];
        float qj[ATT_R][T * VEC], vj[ATT_R][T * VEC];
        row_load_slots(col, s, k1, N, j);
        rg_load_rows<VEC, T>(qx, ldq, vx, ldv, j, k1 - s, gl, glog2, w, qj, vj);
        rg_take_batch<T * VEC>(qj, vj, k, acc);
    }
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_resgated_aggregate(const float *__restrict__ kx, int ldk, const float *__restrict__ qx, int ldq,
                                                            const float *__restrict__ vx, int ldv, const float *__restrict__ root, int ldr,
                                                            const float *__restrict__ skip, float *__restrict__ out,
                                                            const int4 *__restrict__ node_rec, const int32_t *__restrict__ col, int N, int E,
                                                            int w, int glog2, int iters)
{
    constexpr int NC = T * VEC;
    __shared__ float s_part[WG * NC]; // one round of a long row's pieces: [lane group][lane of the group][acc[NC]]
    __shared__ int s_long[WG];        // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
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
            float k[NC], qj[ATT_R][NC], vj[ATT_R][NC], acc[NC];
            rg_load_rows<VEC, T>(qx, ldq, vx, ldv, j0, dg_0, gl, glog2, w, qj, vj);
            att_load_row<VEC, T>(kx, (size_t)n0, ldk, 0, gl, glog2, w, k);
#pragma unroll
            for (int c = 0; c < NC; c++)
                acc[c] = 0.0f;
            if (dg_0 > 0)
                rg_take_batch<NC>(qj, vj, k, acc);
            if (dg_0 > ATT_R)
                rg_piece<VEC, T>(qx, ldq, vx, ldv, col, rp_0 + ATT_R, rp_0 + dg_0, N, gl, glog2, w, k, acc);
            finish(n0, dg_0 > 0, acc);
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
                    rg_piece<VEC, T>(qx, ldq, vx, ldv, col, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, gl, glog2, w, k, part);
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

hipError_t launch_resgated_aggregate(const BatchTables &t, const float *k, int ldk, const float *q, int ldq, const float *v, int ldv,
                                     const float *root, int ldr, const float *skip, int act, float *out, int width, hipStream_t s)
{
    if (width < 1 || width > RG_MAX_WIDTH || ldk < width || ldq < width || ldv < width || (root != nullptr && ldr < width) ||
        (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const AttForm fm = att_form(width, {k, q, v, root, skip, out}, {ldk, ldq, ldv, root != nullptr ? ldr : 0});
    const int steps = att_item_steps(t.num_nodes, 1, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, width, [&](auto vec, auto strides) {
            auto kern = k_resgated_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, RG_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, k, ldk, q, ldq, v, ldv, root, root != nullptr ? ldr : width, skip, out,
                               t.node_rec, t.col, t.num_nodes, t.num_edges, width, fm.glog2, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
