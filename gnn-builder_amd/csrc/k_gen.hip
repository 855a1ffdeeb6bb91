// k_gen.hip -- GENConv (DeeperGCN): the per-column softmax aggregate of the messages themselves (gnnb_gen.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_gen_aggregate (no reference in gnnbuilder; models.py, class _GENConv):
//   m_ij[c] = relu(s_j[c] + p_ij[c]) + eps_m,   p_ij = W_e e_ij + b_e (edge_dim 0: p = 0),   e_ij = edge_attr[eid[slot]]  (COO row order)
//   out_i[c] = sum_j a_ij[c] m_ij[c] + r_i[c],  a_ij[c] = exp(t m_ij[c]) / sum_k exp(t m_ik[c])    -- softmax over i's in-edges, PER COLUMN
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid).  A row without in-edges is r_i (0 with r = NULL).  No
// other aggregate can express it: the fixed statistics of k_aggregate / k_gine add or compare, and the attention kernels of
// gnnb_attn.h keep one (max, sum) per HEAD for a score that is not the message.  Unfused the layer is an [E, width] edge term, an
// [E, width] message, a segmented max, an [E, width] exp and two segmented sums; here none of them reaches HBM.
//
// Work split: k_gine_aggregate's, because the traffic is the same -- one gathered row and one attribute row per edge.  A lane group
// of G = 2^glog2 lanes owns a destination row, a lane owns VEC consecutive columns (16-byte form when width, lds, ldr, ldo are
// multiples of 4 and s, r, out are 16-byte aligned; scalar form otherwise: a first layer with in == out = 9 is no corner case); rows
// wider than 64 vectors are walked in column passes; lane groups walk their rows with a grid stride over what is resident; GEN_R = 4
// neighbour rows and attribute rows are in flight and the walk is three deep (record of step it + 2, slots of step it + 1, rows of
// step `it`); the attribute row is read at a group-uniform address.
//
// What is this kernel's:
//   state   = per COLUMN (M, S, W): the running max of z = t m, the sum of the weights exp(z - M) and the weighted sum of the
//             messages, 3 VEC registers per lane -- every column is a softmax of its own, so there is no cross-lane exchange and no
//             LDS on the short-row path.  The empty state is (-inf, 0, 0).
//   update  = ONE transcendental per (edge, column): d = z - M, f = exp(-|d|);
//               d > 0:  S = fma(S, f, 1), W = fma(W, f, m), M = z        (a new max: the old sums shrink)
//               else:   S = S + f,        W = fma(f, m, W)
//             The first message meets M = -inf: d = +inf, f = exp2(-inf) = 0, so S = 1, W = m with no special case.  exp(x) is the
//             hardware's exp2 of x * log2(e) (att_exp).  t = 0 gives f = 1 throughout: the mean; a negative t leans to the min.
//   weights = W_e [width, edge_dim] and b_e are staged in LDS once per workgroup as [edge_dim + 1][width] (b_e the last row) -- a
//             lane's columns of one d are one 16-byte piece, consecutive lanes consecutive pieces -- behind ONE barrier, and read
//             once per (batch of GEN_R slots, d): one LDS read feeds GEN_R VEC FMAs.  k_gine keeps them in registers (VEC edge_dim +
//             VEC per lane); with 3 VEC state registers on top that costs a wave per SIMD at edge_dim 16, and k_resgated_edge measured
//             the staged form 7 .. 9 % faster for the same access pattern.  edge_dim 0 compiles no edge code, no LDS.
//
// Summation order (fixed: it depends on the batch and on the form -- 16-byte or scalar --, never on the grid or on occupancy; the two
// forms give the same bits, a column's chain does not involve its neighbours):
//   p_c   = fma(W_e[c][edge_dim - 1], e[edge_dim - 1], ... fma(W_e[c][0], e[0], b_e[c]))        -- d increasing
//   m_c   = fmaxf(s_jc + p_c, 0) + eps_m;   z = t * m_c                                          -- the message before z
//   row   = of at most GEN_CHUNK = 64 in-edges: the update above, one slot after the other in CSR slot order, from the empty state
//   hub   = a longer row in pieces of 64 slots, each from the empty state; the pieces merged in piece order onto the empty state:
//           M' = max(M, M_p); fa = exp(M - M'), fb = exp(M_p - M'); S = fma(S_p, fb, S * fa); W = fma(W_p, fb, W * fa)
//   out   = (S > 0 ? W / S : 0) + r_ic  (IEEE division; r read once per row; r = NULL: no add)
// PyG's + 1e-16 in the denominator is dropped: S >= 1 whenever the row has an edge (the max's own weight is 1).
// Degree skew: k_gine's.  The workgroup's lane groups take a hub's pieces round-robin, park (M, S, W) per column in LDS (3 VEC floats
// per lane: 12 KiB at VEC 4) and the owner merges them.  Long rows go in a second walk: a workgroup without one pays ONE barrier per
// column pass.  No MFMA: the kernel is a gather, the layer's matrix work is its GEMMs.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int GEN_CHUNK = 64;     // CSR slots per piece of a long row
constexpr int GEN_R = 4;          // neighbour rows in flight per lane group
constexpr int GEN_WG_PER_CU = 8;  // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int GEN_LDS_AHEAD = 4;  // values of d whose staged weights are in flight at once
constexpr int GEN_MAX_EDGE_DIM = 16;

extern __shared__ __attribute__((aligned(16))) float gen_s_w[]; // [ED + 1][w]: W_e transposed, b_e last (the launch's dynamic LDS)

template <int VEC>
__device__ __forceinline__ void gen_store_vec(float *p, const float (&v)[VEC])
{
    if constexpr (VEC == 4)
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *p = v[0];
}

template <int VEC>
__device__ __forceinline__ void gen_empty(float (&M)[VEC], float (&S)[VEC], float (&W)[VEC])
{
#pragma unroll
    for (int v = 0; v < VEC; v++)
        M[v] = -INFINITY, S[v] = 0.0f, W[v] = 0.0f;
}

// one message into one column's state: the update of the header
__device__ __forceinline__ void gen_take(float m, float t, float &M, float &S, float &W)
{
    const float z = t * m, d = z - M;
    const float f = att_exp(-fabsf(d));
    const bool up = d > 0.0f;
    S = up ? fmaf(S, f, 1.0f) : S + f;
    W = up ? fmaf(W, f, m) : fmaf(f, m, W);
    M = up ? z : M;
}

// the state (M2, S2, W2) of a later piece merged onto (M, S, W)
__device__ __forceinline__ void gen_merge(float M2, float S2, float W2, float &M, float &S, float &W)
{
    const float Mn = fmaxf(M, M2);
    const float fa = att_exp(M - Mn), fb = att_exp(M2 - Mn);
    S = fmaf(S2, fb, S * fa);
    W = fmaf(W2, fb, W * fa);
    M = Mn;
}

// the CSR slots [k, k + GEN_R) below k1 (and their COO rows, where the kernel has edge features)
template <int ED>
__device__ __forceinline__ void gen_load_slots(const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int k, int k1, int N, int E,
                                               int (&j)[GEN_R], int (&ei)[GEN_R])
{
    if constexpr (ED > 0) {
        row_load_slots(col, eid, k, k1, N, E, j, ei);
    } else {
        row_load_slots(col, k, k1, N, j);
#pragma unroll
        for (int r = 0; r < GEN_R; r++)
            ei[r] = 0;
    }
}

// the first n of those neighbours' s_j (the lane's VEC columns from column fo) and attribute rows; the others zeros
template <int VEC, int ED>
__device__ __forceinline__ void gen_load_messages(const float *__restrict__ s, int lds, const float *__restrict__ ea, const int (&j)[GEN_R],
                                                  const int (&ei)[GEN_R], int n, int fo, bool avec, float (&sj)[GEN_R][VEC],
                                                  float (&e)[GEN_R][ED > 0 ? ED : 1])
{
#pragma unroll
    for (int r = 0; r < GEN_R; r++) {
#pragma unroll
        for (int v = 0; v < VEC; v++)
            sj[r][v] = 0.0f;
#pragma unroll
        for (int d = 0; d < (ED > 0 ? ED : 1); d++)
            e[r][d] = 0.0f;
        if (r < n) {
            row_load_vec<VEC>(s + (size_t)j[r] * lds + fo, sj[r]);
            if constexpr (ED > 0)
                row_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e[r]);
        }
    }
}

// the first n of GEN_R loaded neighbours taken into the lane's states in their order.  p forms in sj (the d loop is outermost so
// that a staged weight is fetched once per batch: every (edge, column) chain keeps its own order)
template <int VEC, int ED>
__device__ __forceinline__ void gen_take_batch(float (&sj)[GEN_R][VEC], const float (&e)[GEN_R][ED > 0 ? ED : 1], int n, int w, int fo, float t,
                                               float eps_m, float (&M)[VEC], float (&S)[VEC], float (&W)[VEC])
{
    if constexpr (ED > 0) {
        float p[GEN_R][VEC], b[VEC];
        row_load_vec<VEC>(gen_s_w + ED * w + fo, b);
#pragma unroll
        for (int r = 0; r < GEN_R; r++)
#pragma unroll
            for (int v = 0; v < VEC; v++)
                p[r][v] = b[v];
#pragma unroll
        for (int d = 0; d < ED; d++) {
            // (the staged weights do not change during the walk: left to itself the compiler reads them once in front of the edge
            // loop -- registers by another road.  A compiler-only fence and a scheduling fence, neither an instruction, keep the
            // reads where they are written: k_resgated_edge's finding)
            if (d % GEN_LDS_AHEAD == 0) {
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                __builtin_amdgcn_sched_barrier(0);
            }
            float wd[VEC];
            row_load_vec<VEC>(gen_s_w + d * w + fo, wd);
#pragma unroll
            for (int r = 0; r < GEN_R; r++)
#pragma unroll
                for (int v = 0; v < VEC; v++)
                    p[r][v] = fmaf(wd[v], e[r][d], p[r][v]);
        }
#pragma unroll
        for (int r = 0; r < GEN_R; r++)
#pragma unroll
            for (int v = 0; v < VEC; v++)
                sj[r][v] = sj[r][v] + p[r][v];
    }
#pragma unroll
    for (int r = 0; r < GEN_R; r++)
        if (r < n) {
#pragma unroll
            for (int v = 0; v < VEC; v++)
                gen_take(fmaxf(sj[r][v], 0.0f) + eps_m, t, M[v], S[v], W[v]);
        }
}

// the messages of the CSR slots [k0, k1) taken into the states, in slot order
template <int VEC, int ED>
__device__ __forceinline__ void gen_piece(const float *__restrict__ s, int lds, const float *__restrict__ ea, const int32_t *__restrict__ col,
                                          const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int w, int fo, bool avec, float t,
                                          float eps_m, float (&M)[VEC], float (&S)[VEC], float (&W)[VEC])
{
    for (int k = k0; k < k1; k += GEN_R) {
        int j[GEN_R], ei[GEN_R];
        float sj[GEN_R][VEC], e[GEN_R][ED > 0 ? ED : 1];
        gen_load_slots<ED>(col, eid, k, k1, N, E, j, ei);
        gen_load_messages<VEC, ED>(s, lds, ea, j, ei, k1 - k, fo, avec, sj, e);
        gen_take_batch<VEC, ED>(sj, e, k1 - k, w, fo, t, eps_m, M, S, W);
    }
}

template <int VEC, int ED>
__global__ __launch_bounds__(WG) void k_gen_aggregate(const float *__restrict__ s, int lds, const float *__restrict__ rt, int ldr,
                                                      const float *__restrict__ ea, const float *__restrict__ we, int ldwe,
                                                      const float *__restrict__ be, float *__restrict__ out, int ldo,
                                                      const int4 *__restrict__ node_rec, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ eid, int N, int E, int w, int glog2, float t, float eps_m,
                                                      int avec, int iters)
{
    __shared__ float s_part[WG * 3 * VEC]; // the states of one round of a long row's pieces: [lane][M | S | W][VEC]
    __shared__ int s_long[WG];             // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const int nvec = w / VEC;
    if constexpr (ED > 0) {
        for (int i = threadIdx.x; i < w * ED; i += WG) {
            const int c = i / ED, d = i - c * ED;
            gen_s_w[d * w + c] = we[(size_t)c * ldwe + d];
        }
        for (int c = threadIdx.x; c < w; c += WG)
            gen_s_w[ED * w + c] = be[c];
        __syncthreads(); // (the one barrier of the short-row path with edge features: every batch below reads the staged weights)
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
    for (int fb = 0; fb < nvec; fb += G) { // column passes (one, up to 64 vectors per row)
        const bool active = fb + gl < nvec;
        const int fo = active ? (fb + gl) * VEC : 0; // (a lane past the width computes on column 0's operands and stores nothing)
        auto finish = [&](int node, const float (&S)[VEC], const float (&W)[VEC]) { // the epilogue of the header
            float o[VEC], ri[VEC];
            if (rt != nullptr)
                row_load_vec<VEC>(rt + (size_t)node * ldr + fo, ri);
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                o[v] = S[v] > 0.0f ? W[v] / S[v] : 0.0f;
                if (rt != nullptr)
                    o[v] += ri[v];
            }
            gen_store_vec<VEC>(out + (size_t)node * ldo + fo, o);
        };
        // ---- rows of at most GEN_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
        // memory latency, not the chain record -> slots -> rows
        int n0, rp_0, dg_0, n1, rp_1, dg_1;
        int j0[GEN_R], e0[GEN_R];
        row_of(0, n0, rp_0, dg_0);
        gen_load_slots<ED>(col, eid, rp_0, rp_0 + (dg_0 <= GEN_CHUNK ? dg_0 : 0), N, E, j0, e0);
        row_of(1, n1, rp_1, dg_1);
        bool any_long = false;
        for (int it = 0; it < iters; it++) {
            int n2, rp_2, dg_2, j1[GEN_R], e1[GEN_R];
            row_of(it + 2, n2, rp_2, dg_2);
            gen_load_slots<ED>(col, eid, rp_1, rp_1 + (dg_1 <= GEN_CHUNK ? dg_1 : 0), N, E, j1, e1);
            any_long |= dg_0 > GEN_CHUNK;
            if (n0 < N && dg_0 <= GEN_CHUNK && active) {
                float sj[GEN_R][VEC], e[GEN_R][ED > 0 ? ED : 1], M[VEC], S[VEC], W[VEC];
                gen_load_messages<VEC, ED>(s, lds, ea, j0, e0, dg_0, fo, avec != 0, sj, e);
                gen_empty<VEC>(M, S, W);
                gen_take_batch<VEC, ED>(sj, e, dg_0, w, fo, t, eps_m, M, S, W);
                if (dg_0 > GEN_R)
                    gen_piece<VEC, ED>(s, lds, ea, col, eid, rp_0 + GEN_R, rp_0 + dg_0, N, E, w, fo, avec != 0, t, eps_m, M, S, W);
                finish(n0, S, W);
            }
            n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
            n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
            for (int r = 0; r < GEN_R; r++)
                j0[r] = j1[r], e0[r] = e1[r];
        }
        // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met
        // none is done with this column pass after ONE barrier
        if (!__syncthreads_or(any_long))
            continue;
        for (int it = 0; it < iters; it++) {
            int node, rp0, deg;
            row_of(it, node, rp0, deg);
            const bool is_long = deg > GEN_CHUNK;
            if (!__syncthreads_or(is_long))
                continue;
            // the long rows of this step, one after the other: pieces round-robin over the lane groups, states through LDS
            if (gl == 0)
                s_long[grp] = is_long ? node : -1;
            __syncthreads();
            for (int g = 0; g < groups; g++) {
                const int ln = s_long[g];
                if (ln < 0)
                    continue;
                int lrp, ldeg;
                row_record(node_rec, ln, E, lrp, ldeg);
                const int npieces = (ldeg + GEN_CHUNK - 1) / GEN_CHUNK;
                float M[VEC], S[VEC], W[VEC];
                gen_empty<VEC>(M, S, W);
                for (int c0 = 0; c0 < npieces; c0 += groups) {
                    const int c = c0 + grp;
                    float pM[VEC], pS[VEC], pW[VEC];
                    gen_empty<VEC>(pM, pS, pW);
                    if (c < npieces && active) // (a piece below npieces holds at least one slot)
                        gen_piece<VEC, ED>(s, lds, ea, col, eid, lrp + c * GEN_CHUNK, lrp + min((c + 1) * GEN_CHUNK, ldeg), N, E, w, fo,
                                           avec != 0, t, eps_m, pM, pS, pW);
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        s_part[(threadIdx.x * 3 + 0) * VEC + v] = pM[v];
                        s_part[(threadIdx.x * 3 + 1) * VEC + v] = pS[v];
                        s_part[(threadIdx.x * 3 + 2) * VEC + v] = pW[v];
                    }
                    __syncthreads();
                    if (grp == g && active) {
                        const int nq = min(groups, npieces - c0);
                        for (int q = 0; q < nq; q++) {
                            const int ql = (q << glog2) + gl;
#pragma unroll
                            for (int v = 0; v < VEC; v++)
                                gen_merge(s_part[(ql * 3 + 0) * VEC + v], s_part[(ql * 3 + 1) * VEC + v], s_part[(ql * 3 + 2) * VEC + v], M[v],
                                          S[v], W[v]);
                        }
                    }
                    __syncthreads();
                }
                if (grp == g && active)
                    finish(ln, S, W);
            }
            __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
        }
    }
}

hipError_t launch_gen_aggregate(const BatchTables &tb, const float *s, int lds, const float *r, int ldr, int width, const float *edge_attr,
                                int edge_dim, const float *we, int ldwe, const float *be, float t, float eps_m, float *out, int ldo,
                                hipStream_t st)
{
    if (edge_dim < 0 || edge_dim > GEN_MAX_EDGE_DIM || width < 1 || ldwe < edge_dim || lds < width || ldo < width || (r && ldr < width))
        return hipErrorInvalidValue;
    if (tb.num_nodes <= 0)
        return hipSuccess;
    const bool v4 = (width % 4 == 0) && (lds % 4 == 0) && (ldo % 4 == 0) && (!r || ldr % 4 == 0) && (((uintptr_t)s & 15) == 0) &&
                    (((uintptr_t)r & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int avec = edge_dim > 0 && (edge_dim % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
    const int nvec = v4 ? width / 4 : width;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int steps = (tb.num_nodes + groups - 1) / groups; // a step = `groups` rows, one per lane group of a workgroup
    const size_t lds_bytes = edge_dim > 0 ? (size_t)(edge_dim + 1) * width * sizeof(float) : 0; // (at most 17 KiB: width 256, edge_dim 16)
    auto launch = [&](auto vec, auto ed) {
        auto kern = k_gen_aggregate<decltype(vec)::value, decltype(ed)::value>;
        // the grid is what is resident at once (the kernel's own occupancy with the launch's dynamic LDS counted, at most
        // GEN_WG_PER_CU per CU): every workgroup walks `iters` steps, the steps of one sweep side by side in memory
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, lds_bytes, GEN_WG_PER_CU);
        const int max_grid = std::max(occ.blocks * occ.cus, 1);
        const int iters = (steps + max_grid - 1) / max_grid;
        const int grid = (steps + iters - 1) / iters;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), lds_bytes, st, s, lds, r, r ? ldr : width, edge_attr, we, ldwe, be, out, ldo, tb.node_rec,
                           tb.col, tb.eid, tb.num_nodes, tb.num_edges, width, glog2, t, eps_m, avec, iters);
    };
    auto by_vec = [&](auto ed) {
        if (v4)
            launch(IntTag<4>{}, ed);
        else
            launch(IntTag<1>{}, ed);
    };
    switch (edge_dim) {
#define GNNB_GEN_ED(n) case n: by_vec(IntTag<n>{}); break;
    GNNB_GEN_ED(0) GNNB_GEN_ED(1) GNNB_GEN_ED(2) GNNB_GEN_ED(3) GNNB_GEN_ED(4) GNNB_GEN_ED(5) GNNB_GEN_ED(6) GNNB_GEN_ED(7) GNNB_GEN_ED(8)
    GNNB_GEN_ED(9) GNNB_GEN_ED(10) GNNB_GEN_ED(11) GNNB_GEN_ED(12) GNNB_GEN_ED(13) GNNB_GEN_ED(14) GNNB_GEN_ED(15) GNNB_GEN_ED(16)
#undef GNNB_GEN_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
