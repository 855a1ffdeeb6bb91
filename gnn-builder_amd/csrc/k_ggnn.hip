// k_ggnn.hip -- GatedGraphConv: the sum of the neighbours' folded messages and the whole GRU cell in ONE pass over the edges
// (gnnb_ggnn.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_ggnn_aggregate (models.py _GatedGraphConv: PyG's GatedGraphConv(aggr='add', bias=True), one step behind its GEMM h -> [p | gh]):
//   acc_g = sum_{j in N(i)} p_j[g]                  g in r, z, n: the three column blocks of the gathered row
//   gi_g  = acc_g + b_ih[g]                         once per row, behind the sum
//   r = sigmoid(gi_r + gh_r),  z = sigmoid(gi_z + gh_z),  n = tanh(fma(r, gh_n, gi_n)),  u = fma(z, h - n, n)
//   out_ic = act(u + skip_ic)
// on the CSR-by-destination tables of the prepared batch (node_rec, col) of a workspace whose tables keep explicit (v, v) edges
// (any but a GCN description's): no self term is added and none is removed, a row without in-edges gets GRUCell(0, h_i).  p = the
// message weight folded into the GRU's input weight (gnnb_weights.h ggnn_fold), so neither the messages [E, width], nor the
// aggregated message [N, width], nor the input side's gate pre-activations [N, 3 width] ever reach HBM.  No score, no cross-lane
// sum, no head: k_resgated_aggregate's row walk (gnnb_attn.h) with three gathered blocks per neighbour and the gates in the
// epilogue instead of per edge.
//
// Work split.  A destination row is owned by a lane group of G = 2^glog2 lanes, G >= width / VEC, at most a wave; a lane owns VEC
// consecutive columns in each of T strides of G * VEC columns (T > 1: the scalar form at width > 64) and keeps the three
// accumulators of its columns in registers for the whole row.  16-byte form (VEC = 4) when width % 4 == 0, h_width % 4 == 0 and
// every operand and stride is 16-byte aligned, scalar form otherwise (att_form with one head of `width` columns).  The grid is cut
// from the kernel's own occupancy (att_grid), at most GG_WG_PER_CU workgroups per CU; every lane group walks its steps with a grid
// stride, three deep (record of step it + 2, slots of step it + 1, rows of step `it`).  ATT_R = 4 neighbours are in flight per
// batch: their 3 ATT_R block loads are all issued before the first is consumed; the row's own gh and h are requested with the first
// batch.  h has h_width <= width columns: those at or beyond h_width are 0 and are not loaded (step 0 of a layer with in < out).
// Stores are non-temporal.
//
// Gates.  sigmoid(s) = rcp(1 + exp2(s * -log2(e))) and tanh(s) = fma(-2, rcp(1 + exp2(s * 2 log2(e))), 1), with the hardware's
// v_exp_f32 and v_rcp_f32 (1 ulp each).  Both saturate exactly: s = -200 gives exp2(+288) = inf, 1 + inf = inf, rcp(inf) = 0 -- a
// gate of exactly 0, and a tanh of fma(-2, 1, 1) = -1 from exp2(-577) = 0; s = +200 gives a gate of rcp(1 + 0) = 1 and a tanh of
// fma(-2, 0, 1) = 1.  No inf - inf and no 0 * inf is formed, so a finite input gives no NaN.  Near 0 the tanh form loses relative,
// not absolute accuracy: its error is a few 2^-24 whatever s is (tests/test_hip_ggnn.py holds the whole to the project's budget).
//
// Summation order (fixed: it depends on the batch and on the form, never on the grid or on which workgroup took a row):
//   batch = ATT_R = 4 consecutive CSR slots: acc_g = (((acc_g + p_0g) + p_1g) + p_2g) + p_3g, plain adds
//           (slots past the row's end take no part: their p is zeros, and acc + 0 is acc)
//   row   = of at most ATT_CHUNK = 64 in-edges: its batches in slot order onto 0.  Longer (a hub): pieces of 64 slots taken
//           round-robin by the workgroup's lane groups in a second walk behind the short rows (gnnb_attn.h's scheme), each
//           piece's batches in slot order onto 0, parked in LDS; the owner adds the pieces in piece order onto 0 -- a plain sum
//   out   = the formulae above; an absent b_ih or skip adds nothing, not + 0
// A repeat launch, another grid or other neighbours in the batch give a row the same bits.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int GG_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int GG_B = 3;         // gate blocks of a gathered row: r | z | n

__device__ __forceinline__ float gg_sigmoid(float s) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * -ATT_LOG2E)); }
__device__ __forceinline__ float gg_tanh(float s)
{
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * (2.0f * ATT_LOG2E))), 1.0f);
}

// the three blocks of row `row` of x = [r | z | n] (row stride ld, a block w columns): the lane's columns of each
template <int VEC, int T>
__device__ __forceinline__ void gg_load_blocks(const float *__restrict__ x, size_t row, int ld, int gl, int glog2, int w, float (&v)[GG_B][T * VEC])
{
#pragma unroll
    for (int g = 0; g < GG_B; g++)
        att_load_row<VEC, T>(x, row, ld, g * w, gl, glog2, w, v[g]);
}

// the first n of ATT_R neighbours' p rows (the lane's columns of the three blocks), all 3 ATT_R loads issued side by side; the
// others zeros
template <int VEC, int T>
__device__ __forceinline__ void gg_load_rows(const float *__restrict__ px, int ldp, const int (&j)[ATT_R], int n, int gl, int glog2, int w,
                                             float (&pj)[ATT_R][GG_B][T * VEC])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        if (r < n) {
            gg_load_blocks<VEC, T>(px, (size_t)j[r], ldp, gl, glog2, w, pj[r]);
        } else {
#pragma unroll
            for (int g = 0; g < GG_B; g++)
#pragma unroll
                for (int c = 0; c < T * VEC; c++)
                    pj[r][g][c] = 0.0f;
        }
    }
}

// one batch: the loaded neighbours added to the accumulators -- the batch rule of the header (a slot past the row's end adds 0)
template <int NC>
__device__ __forceinline__ void gg_take_batch(const float (&pj)[ATT_R][GG_B][NC], float (&acc)[GG_B][NC])
{
#pragma unroll
    for (int g = 0; g < GG_B; g++)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            float t = acc[g][c];
#pragma unroll
            for (int r = 0; r < ATT_R; r++)
                t += pj[r][g][c];
            acc[g][c] = t;
        }
}

// the CSR slots [k0, k1) added to the accumulators in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void gg_piece(const float *__restrict__ px, int ldp, const int32_t *__restrict__ col, int k0, int k1, int N, int gl,
                                         int glog2, int w, float (&acc)[GG_B][T * VEC])
{
    for (int s = k0; s < k1; s += ATT_R) {
        int j[ATT_R];
        float pj[ATT_R][GG_B][T * VEC];
        row_load_slots(col, s, k1, N, j);
        gg_load_rows<VEC, T>(px, ldp, j, k1 - s, gl, glog2, w, pj);
        gg_take_batch<T * VEC>(pj, acc);
    }
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_ggnn_aggregate(const float *__restrict__ px, int ldp, const float *__restrict__ ghx, int ldgh,
                                                        const float *__restrict__ hx, int ldh, int hw, const float *__restrict__ b_ih,
                                                        const float *__restrict__ skip, float *__restrict__ out,
                                                        const int4 *__restrict__ node_rec, const int32_t *__restrict__ col, int N, int E, int w,
                                                        int glog2, int iters)
{
    constexpr int NC = T * VEC;
    __shared__ float s_part[WG * GG_B * NC]; // one round of a long row's pieces: [lane group][lane of the group][acc[GG_B][NC]]
    __shared__ int s_long[WG];               // per lane group: the long row of its step, or -1
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
    // the GRU cell of row `node` on its summed input side, the row's own gh and h (the lane's columns), and the store
    auto finish = [&](int node, const float (&acc)[GG_B][NC], const float (&gh)[GG_B][NC], const float (&h)[NC]) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < w) {
                float gi[GG_B][VEC], o[VEC], sk[VEC];
#pragma unroll
                for (int g = 0; g < GG_B; g++) {
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        gi[g][u] = acc[g][t * VEC + u];
                    if (b_ih != nullptr) { // (an absent term adds nothing, not + 0)
                        float b[VEC];
                        row_load_vec<VEC>(b_ih + g * w + c, b);
#pragma unroll
                        for (int u = 0; u < VEC; u++)
                            gi[g][u] += b[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < VEC; u++) {
                    const float r = gg_sigmoid(gi[0][u] + gh[0][t * VEC + u]);
                    const float z = gg_sigmoid(gi[1][u] + gh[1][t * VEC + u]);
                    const float n = gg_tanh(fmaf(r, gh[2][t * VEC + u], gi[2][u]));
                    o[u] = fmaf(z, h[t * VEC + u] - n, n);
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
            float pj[ATT_R][GG_B][NC], acc[GG_B][NC], gh[GG_B][NC], h[NC];
            gg_load_rows<VEC, T>(px, ldp, j0, dg_0, gl, glog2, w, pj);
            gg_load_blocks<VEC, T>(ghx, (size_t)n0, ldgh, gl, glog2, w, gh);
            att_load_row<VEC, T>(hx, (size_t)n0, ldh, 0, gl, glog2, hw, h);
#pragma unroll
            for (int g = 0; g < GG_B; g++)
#pragma unroll
                for (int c = 0; c < NC; c++)
                    acc[g][c] = 0.0f;
            if (dg_0 > 0)
                gg_take_batch<NC>(pj, acc);
            if (dg_0 > ATT_R)
                gg_piece<VEC, T>(px, ldp, col, rp_0 + ATT_R, rp_0 + dg_0, N, gl, glog2, w, acc);
            finish(n0, acc, gh, h);
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
            float acc[GG_B][NC]; // (the owner's, the pieces in their order onto 0; the others' copy is not used)
#pragma unroll
            for (int b = 0; b < GG_B; b++)
#pragma unroll
                for (int c = 0; c < NC; c++)
                    acc[b][c] = 0.0f;
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                float part[GG_B][NC];
#pragma unroll
                for (int b = 0; b < GG_B; b++)
#pragma unroll
                    for (int u = 0; u < NC; u++)
                        part[b][u] = 0.0f;
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    gg_piece<VEC, T>(px, ldp, col, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, gl, glog2, w, part);
#pragma unroll
                for (int b = 0; b < GG_B; b++)
#pragma unroll
                    for (int u = 0; u < NC; u++)
                        s_part[(size_t)threadIdx.x * (GG_B * NC) + b * NC + u] = part[b][u];
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked as zeros and are not read)
                    for (int qq = 0; qq < nq; qq++) {
                        const float *pp = s_part + (size_t)((qq << glog2) + gl) * (GG_B * NC);
#pragma unroll
                        for (int b = 0; b < GG_B; b++)
#pragma unroll
                            for (int u = 0; u < NC; u++)
                                acc[b][u] += pp[b * NC + u];
                    }
                }
                __syncthreads();
            }
            if (grp == g) {
                float gh[GG_B][NC], h[NC];
                gg_load_blocks<VEC, T>(ghx, (size_t)ln, ldgh, gl, glog2, w, gh);
                att_load_row<VEC, T>(hx, (size_t)ln, ldh, 0, gl, glog2, hw, h);
                finish(ln, acc, gh, h);
            }
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
    }
}

hipError_t launch_ggnn_aggregate(const BatchTables &t, const float *p, int ldp, const float *gh, int ldgh, const float *h, int ldh, int h_width,
                                 const float *b_ih, const float *skip, int act, float *out, int width, hipStream_t s)
{
    if (width < 1 || width > GG_MAX_WIDTH || h_width < 1 || h_width > width || ldp < 3 * width || ldgh < 3 * width || ldh < h_width ||
        (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    // (h_width rides with the strides: the 16-byte form needs it a multiple of 4 as it needs them)
    const AttForm fm = att_form(width, {p, gh, h, b_ih, skip, out}, {ldp, ldgh, ldh, h_width});
    const int steps = att_item_steps(t.num_nodes, 1, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, width, [&](auto vec, auto strides) {
            auto kern = k_ggnn_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, GG_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, p, ldp, gh, ldgh, h, ldh, h_width, b_ih, skip, out, t.node_rec, t.col,
                               t.num_nodes, t.num_edges, width, fm.glog2, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
