// k_pna_edge.hip -- PNA with edge features: the edge projection inside the four-statistics aggregate (gnnb_pna_edge.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_pna_edge_aggregate (models.py _PNAEConv: PyG's PNAConv(edge_dim=...) message + its four aggregators; pna_conv_agg,
// gnn_builder_lib.h:1750-1834, is the same without the edge term):
//   out_i = max | min | mean | std  over the in-edges j -> i of   h_ij = q_i + p_j + (W_e e_ij + b_e),   e_ij = edge_attr[eid[slot]]
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid).  PNA's pre-NN is linear, so
// pre_nn([x_i | x_j | enc(e_ij)]) splits into the per-node products q = x Wa^T + b and p = x Wb^T (two GEMMs, as for PNA without
// edges) and an edge term whose weights W_e = W_c W_enc, b_e = W_c b_enc are formed at upload (gnnb_weights.h:
// pna_edge_projection).  The [E, width] edge term is formed per lane from the edge's edge_dim <= 16 attributes and never reaches
// HBM.  Output layout and finalisation are AggAcc<GNNB_AGG_PNA>'s (k_aggregate.hip): [N, 4 width], mean = sum / d, std = pyg_std
// of (sum of squares / d, mean), four zeros for a row without in-edges; q == nullptr: no destination term.
//
// Work split -- k_gine_aggregate's (k_gine.hip), which this kernel is modelled on.  A lane group of G = 2^glog2 lanes owns a
// destination row, a lane owns VEC consecutive columns (16-byte accesses when width % 4 == 0 and p / q / out are aligned, scalar
// accesses otherwise: a first layer runs at width 9 or 11).  Rows wider than 64 vectors are walked in column passes.  The grid is a
// few workgroups per CU, every lane group walks its rows with a grid stride; W_e[c][0 .. edge_dim) and b_e[c] of the lane's columns
// are loop invariants in REGISTERS.  The edge's attribute row is read at an address that is the same in every lane of the group:
// one fetch serves the group.  PNAE_R neighbour rows (p_j and e_ij) are loaded before the first is consumed, and the walk is
// software-pipelined over three steps (record of row it + 2, slots of row it + 1, rows of row `it`).
//
// Summation order (fixed: it depends on the batch, never on the launch shape):
//   t_c   = fma(W_e[c][edge_dim - 1], e[edge_dim - 1], ... fma(W_e[c][0], e[0], b_e[c]))           -- d increasing
//   h_c   = (t_c + p_j[c]) + q_i[c]
//   piece = a row's CSR slots in pieces of PNAE_CHUNK = 64; of a piece's messages, in slot order: max, min, the sum s1 (starting
//           from 0) and the sum of squares s2 = fma(h, h, s2) (starting from 0)
//   row   = the pieces' four partials combined in piece order: max of max, min of min, s1 and s2 each added starting from 0
//           (a row of at most 64 in-edges IS its one piece: plain slot order)
// Degree skew: a row of more than PNAE_CHUNK in-edges (a hub) is not walked by its own lane group.  The workgroup's lane groups take
// its pieces round-robin, park the four partials per piece in LDS and the owner combines them in piece order -- the rule above.
// Long rows are taken in a second walk behind the short ones: a workgroup without one pays ONE barrier per column pass.
#include "gnnb_device.h"

namespace gnnb {

constexpr int PNAE_CHUNK = 64;      // CSR slots per piece of a row's statistics
constexpr int PNAE_R = 4;           // neighbour rows in flight per lane group
constexpr int PNAE_WG_PER_CU = 8;   // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int PNAE_MAX_EDGE_DIM = 16;

// a lane's four running statistics of its VEC columns
template <int VEC>
struct PnaeStats {
    float mx[VEC], mn[VEC], s1[VEC], s2[VEC];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int v = 0; v < VEC; v++)
            mx[v] = -INFINITY, mn[v] = INFINITY, s1[v] = 0.0f, s2[v] = 0.0f;
    }
};

// h = (W_e e + b_e + p_j) + q_i of the first n of PNAE_R loaded neighbours, taken into the statistics in their order
template <int VEC, int ED>
__device__ __forceinline__ void pnae_take_messages(const float (&pj)[PNAE_R][VEC], const float (&e)[PNAE_R][ED], int n,
                                                   const float (&wgt)[VEC][ED], const float (&bias)[VEC], const float (&qi)[VEC],
                                                   PnaeStats<VEC> &a)
{
#pragma unroll
    for (int r = 0; r < PNAE_R; r++)
        if (r < n) {
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                float t = bias[v];
#pragma unroll
                for (int d = 0; d < ED; d++)
                    t = fmaf(wgt[v][d], e[r][d], t);
                const float h = (t + pj[r][v]) + qi[v];
                a.mx[v] = fmaxf(a.mx[v], h);
                a.mn[v] = fminf(a.mn[v], h);
                a.s1[v] += h;
                a.s2[v] = fmaf(h, h, a.s2[v]);
            }
        }
}

// ... and the first n of those neighbours' p_j (the lane's VEC columns from column fo) and attribute rows
template <int VEC, int ED>
__device__ __forceinline__ void pnae_load_messages(const float *__restrict__ p, const float *__restrict__ ea, const int (&j)[PNAE_R],
                                                   const int (&ei)[PNAE_R], int n, int w, int fo, bool avec, float (&pj)[PNAE_R][VEC],
                                                   float (&e)[PNAE_R][ED])
{
#pragma unroll
    for (int r = 0; r < PNAE_R; r++) {
#pragma unroll
        for (int v = 0; v < VEC; v++)
            pj[r][v] = 0.0f;
#pragma unroll
        for (int d = 0; d < ED; d++)
            e[r][d] = 0.0f;
        if (r < n) {
            row_load_vec<VEC>(p + (size_t)j[r] * w + fo, pj[r]);
            row_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e[r]);
        }
    }
}

// the messages of the CSR slots [k0, k1) taken into the statistics, in slot order
template <int VEC, int ED>
__device__ __forceinline__ void pnae_piece(const float *__restrict__ p, const float *__restrict__ ea, const int32_t *__restrict__ col,
                                           const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int w, int fo, bool avec,
                                           const float (&wgt)[VEC][ED], const float (&bias)[VEC], const float (&qi)[VEC], PnaeStats<VEC> &a)
{
    for (int k = k0; k < k1; k += PNAE_R) {
        int j[PNAE_R], ei[PNAE_R];
        float pj[PNAE_R][VEC], e[PNAE_R][ED];
        row_load_slots(col, eid, k, k1, N, E, j, ei);
        pnae_load_messages<VEC, ED>(p, ea, j, ei, k1 - k, w, fo, avec, pj, e);
        pnae_take_messages<VEC, ED>(pj, e, k1 - k, wgt, bias, qi, a);
    }
}

// (<4, 4> -- 16-byte form, edge_dim 4: bond features -- is asked to fit four waves per SIMD: 127 registers, no scratch, where the
// compiler's own choice was 130 and three waves; the kernel is latency-bound: 78.0 -> 72.5 us at the shape of DESIGN 3.2b.  The
// same request spills from edge_dim 5 up, so it is made for this one instantiation)
template <int VEC, int ED>
__global__ __launch_bounds__(WG, (VEC == 4 && ED == 4) ? 4 : 1) void k_pna_edge_aggregate(const float *__restrict__ p, const float *__restrict__ q, const float *__restrict__ ea,
                                                           const float *__restrict__ we, int ldwe, const float *__restrict__ be,
                                                           float *__restrict__ out, const int4 *__restrict__ node_rec,
                                                           const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int N, int E, int w,
                                                           int glog2, int avec, int iters)
{
    __shared__ float s_part[WG * 4 * VEC]; // the partials of one round of a long row: [lane group][lane of the group][max, min, s1, s2][VEC]
    __shared__ int s_long[WG];             // per lane group: the long row of its step, or -1
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const int nvec = w / VEC;
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
        const int fo = active ? (fb + gl) * VEC : 0;
        float wgt[VEC][ED], bias[VEC];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            bias[v] = active ? be[fo + v] : 0.0f;
#pragma unroll
            for (int d = 0; d < ED; d++)
                wgt[v][d] = active ? we[(size_t)(fo + v) * ldwe + d] : 0.0f;
        }
        auto load_q = [&](int node, float (&qi)[VEC]) { // the destination term (none: zeros)
#pragma unroll
            for (int v = 0; v < VEC; v++)
                qi[v] = 0.0f;
            if (q != nullptr)
                row_load_vec<VEC>(q + (size_t)node * w + fo, qi);
        };
        auto finish = [&](int node, int deg, const PnaeStats<VEC> &a) { // AggAcc<GNNB_AGG_PNA>::done
            float mx[VEC], mn[VEC], mean[VEC], sd[VEC];
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                mx[v] = mn[v] = mean[v] = sd[v] = 0.0f;
                if (deg > 0) {
                    const float dn = (float)deg;
                    mx[v] = a.mx[v], mn[v] = a.mn[v];
                    mean[v] = a.s1[v] / dn;
                    sd[v] = pyg_std1(a.s2[v] / dn, mean[v]);
                }
            }
            float *o = out + (size_t)node * 4 * w + fo;
            row_store_nt<VEC>(o, mx);
            row_store_nt<VEC>(o + w, mn);
            row_store_nt<VEC>(o + 2 * (size_t)w, mean);
            row_store_nt<VEC>(o + 3 * (size_t)w, sd);
        };
        // ---- rows of at most PNAE_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
        // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first PNAE_R slots of step it + 1
        // are requested in front of the rows of step `it`, whose own record and slots arrived a step ago
        int n0, rp_0, dg_0, n1, rp_1, dg_1;
        int j0[PNAE_R], e0[PNAE_R];
        row_of(0, n0, rp_0, dg_0);
        row_load_slots(col, eid, rp_0, rp_0 + (dg_0 <= PNAE_CHUNK ? dg_0 : 0), N, E, j0, e0);
        row_of(1, n1, rp_1, dg_1);
        bool any_long = false;
        for (int it = 0; it < iters; it++) {
            int n2, rp_2, dg_2, j1[PNAE_R], e1[PNAE_R];
            row_of(it + 2, n2, rp_2, dg_2);
            row_load_slots(col, eid, rp_1, rp_1 + (dg_1 <= PNAE_CHUNK ? dg_1 : 0), N, E, j1, e1);
            any_long |= dg_0 > PNAE_CHUNK;
            if (n0 < N && dg_0 <= PNAE_CHUNK && active) {
                float qi[VEC], pj[PNAE_R][VEC], e[PNAE_R][ED];
                PnaeStats<VEC> a;
                load_q(n0, qi);
                pnae_load_messages<VEC, ED>(p, ea, j0, e0, dg_0, w, fo, avec != 0, pj, e);
                a.init();
                pnae_take_messages<VEC, ED>(pj, e, dg_0, wgt, bias, qi, a);
                if (dg_0 > PNAE_R)
                    pnae_piece<VEC, ED>(p, ea, col, eid, rp_0 + PNAE_R, rp_0 + dg_0, N, E, w, fo, avec != 0, wgt, bias, qi, a);
                finish(n0, dg_0, a);
            }
            n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
            n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
            for (int r = 0; r < PNAE_R; r++)
                j0[r] = j1[r], e0[r] = e1[r];
        }
        // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met
        // none is done with this column pass after ONE barrier
        if (!__syncthreads_or(any_long))
            continue;
        for (int it = 0; it < iters; it++) {
            int node, rp0, deg;
            row_of(it, node, rp0, deg);
            const bool is_long = deg > PNAE_CHUNK;
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
                const int npieces = (ldeg + PNAE_CHUNK - 1) / PNAE_CHUNK;
                float qi[VEC];
                load_q(ln, qi); // (every piece's messages carry the row's destination term)
                PnaeStats<VEC> a;
                a.init();
                for (int c0 = 0; c0 < npieces; c0 += groups) {
                    const int c = c0 + grp;
                    PnaeStats<VEC> part;
                    part.init();
                    if (c < npieces && active)
                        pnae_piece<VEC, ED>(p, ea, col, eid, lrp + c * PNAE_CHUNK, lrp + min((c + 1) * PNAE_CHUNK, ldeg), N, E, w, fo,
                                            avec != 0, wgt, bias, qi, part);
#pragma unroll
                    for (int v = 0; v < VEC; v++) {
                        float *sp = s_part + (size_t)threadIdx.x * 4 * VEC + v;
                        sp[0] = part.mx[v], sp[VEC] = part.mn[v], sp[2 * VEC] = part.s1[v], sp[3 * VEC] = part.s2[v];
                    }
                    __syncthreads();
                    if (grp == g) {
                        const int nq = min(groups, npieces - c0);
                        for (int qq = 0; qq < nq; qq++)
#pragma unroll
                            for (int v = 0; v < VEC; v++) {
                                const float *sp = s_part + (size_t)((qq << glog2) + gl) * 4 * VEC + v;
                                a.mx[v] = fmaxf(a.mx[v], sp[0]);
                                a.mn[v] = fminf(a.mn[v], sp[VEC]);
                                a.s1[v] += sp[2 * VEC];
                                a.s2[v] += sp[3 * VEC];
                            }
                    }
                    __syncthreads();
                }
                if (grp == g && active)
                    finish(ln, ldeg, a);
            }
            __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
        }
    }
}

hipError_t launch_pna_edge_aggregate(const BatchTables &t, const float *p, const float *q, const float *edge_attr, int edge_dim, const float *we,
                                     int ldwe, const float *be, float *out, int width, hipStream_t s)
{
    if (edge_dim < 1 || edge_dim > PNAE_MAX_EDGE_DIM || width < 1 || ldwe < edge_dim)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const bool v4 = (width % 4 == 0) && (((uintptr_t)p & 15) == 0) && (((uintptr_t)q & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int avec = (edge_dim % 4 == 0) && (((uintptr_t)edge_attr & 15) == 0);
    const int nvec = v4 ? width / 4 : width;
    const int glog2 = lane_group_log2(nvec);
    const int groups = WG >> glog2;
    const int steps = (t.num_nodes + groups - 1) / groups; // a step = `groups` rows, one per lane group of a workgroup
    auto launch = [&](auto vec, auto ed) {
        auto kern = k_pna_edge_aggregate<decltype(vec)::value, decltype(ed)::value>;
        // the grid is what is resident at once (the kernel's own occupancy, at most PNAE_WG_PER_CU per CU): every workgroup walks
        // `iters` steps, the steps of one sweep side by side in memory
        const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, 0, PNAE_WG_PER_CU);
        const int max_grid = std::max(occ.blocks * occ.cus, 1);
        const int iters = (steps + max_grid - 1) / max_grid;
        const int grid = (steps + iters - 1) / iters;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, p, q, edge_attr, we, ldwe, be, out, t.node_rec, t.col, t.eid, t.num_nodes,
                           t.num_edges, width, glog2, avec, iters);
    };
    auto by_vec = [&](auto ed) {
        if (v4)
            launch(IntTag<4>{}, ed);
        else
            launch(IntTag<1>{}, ed);
    };
    switch (edge_dim) {
#define GNNB_PNAE_ED(n) case n: by_vec(IntTag<n>{}); break;
    GNNB_PNAE_ED(1) GNNB_PNAE_ED(2) GNNB_PNAE_ED(3) GNNB_PNAE_ED(4) GNNB_PNAE_ED(5) GNNB_PNAE_ED(6) GNNB_PNAE_ED(7) GNNB_PNAE_ED(8)
    GNNB_PNAE_ED(9) GNNB_PNAE_ED(10) GNNB_PNAE_ED(11) GNNB_PNAE_ED(12) GNNB_PNAE_ED(13) GNNB_PNAE_ED(14) GNNB_PNAE_ED(15) GNNB_PNAE_ED(16)
#undef GNNB_PNAE_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
