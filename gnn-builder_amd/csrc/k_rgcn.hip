// k_rgcn.hip -- RGCNConv with integer edge types: the per-slot records (relation, mean weight) and the per-relation mean of the
// neighbours' transformed rows in ONE gather per edge (gnnb_rgcn.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels
// of the GNNBuilder hot path); wavefront = 64 lanes.
//
// The layer (models.py _RGCNConv: PyG's RGCNConv(in, out, num_relations = R, aggr = 'mean'), behind its GEMM x -> [p_0 | .. | p_{R-1} | root]):
//   out_ic = act((sum_{r < R} (1 / |N_r(i)|) sum_{j in N_r(i)} p_r[j, c] + root_ic) + skip_ic)
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid) of a workspace whose tables keep explicit (v, v) edges
// (any but a GCN description's): no self term is added and none is removed, duplicate edges count as often as they occur, a relation
// without an edge into i contributes nothing.  The message is linear, so the per-relation transform is the GEMM's and the kernel
// gathers ONE row-width per edge -- the traffic of a plain sum --: which column block, and with which weight, is the slot's record.
//
// k_rgcn_slots (once per forward, shared by all layers): rec[s] = {rel, w} for every CSR slot s of row i, rel = edge_type[eid[s]],
// w = 1.0f / (float)|N_rel(i)|.  The counts are integers -- exact, whatever the order --, the division is the correctly rounded one
// (__fdiv_rn: numpy's float32 division gives the same bits).  The R <= 8 counters are registers: unrolled compares, no indexed
// array, no scratch.  A row of at most RGCN_SLOT_CHUNK = 64 slots is one thread's (two passes over its slots); a longer row (a hub)
// is taken by the whole wave of the thread that met it: a lane per slot, stride 64, the counters summed across the lanes.  A type
// outside [0, R) sets GNNB_FLAG_EDGE_TYPE (once per wave that saw one) and gives the record {0, 0.0f}: the slot adds 0 * p_0[j] to
// its row, and no address is ever formed from an unchecked type.
//
// k_rgcn_aggregate: k_ggnn_aggregate's row walk (gnnb_attn.h) with one gathered block per neighbour.  A destination row is owned
// by a lane group of G = 2^glog2 lanes, G >= width / VEC, at most a wave; a lane owns VEC consecutive columns in each of T strides
// of G * VEC columns (T > 1: the scalar form at width > 64) and keeps its accumulators in registers for the whole row.  16-byte
// form (VEC = 4) when width % 4 == 0 and every operand and stride is 16-byte aligned, scalar form otherwise (att_form with one head
// of `width` columns).  The grid is cut from the kernel's own occupancy (att_grid), at most RGCN_WG_PER_CU workgroups per CU; every
// lane group walks its steps with a grid stride, three deep (record of step it + 2, slots of step it + 1, rows of step `it`).
// ATT_R = 4 neighbours are in flight per batch: their row loads are all issued before the first is consumed; the row's own root
// and skip terms are requested with the first batch.  Stores are non-temporal.  The relation of a record is clamped into [0, R)
// before it is used (the stage entry takes the caller's records).
//
// Summation order (fixed: it depends on the batch and on the form, never on the grid or on which workgroup took a row):
//   batch = ATT_R = 4 consecutive CSR slots: acc = fma(w_3, p_3, fma(w_2, p_2, fma(w_1, p_1, fma(w_0, p_0, acc))))
//           (slots past the row's end take no part: w = 0 and p = 0, and fma(0, 0, acc) is acc)
//   row   = of at most ATT_CHUNK = 64 in-edges: its batches in slot order onto 0.  Longer (a hub): pieces of 64 slots taken
//           round-robin by the workgroup's lane groups in a second walk behind the short rows (gnnb_attn.h's scheme), each
//           piece's batches in slot order onto 0, parked in LDS; the owner adds the pieces in piece order onto 0 -- a plain sum
//   out   = act((acc + root_ic) + skip_ic); an absent root or skip adds nothing, not + 0
// A repeat launch, another grid or other neighbours in the batch give a row the same bits.
#include "gnnb_attn.h"

namespace gnnb {

constexpr int RGCN_WG_PER_CU = 8;   // workgroups per CU the grid is cut for at most (what is resident; more rows than that: grid stride)
constexpr int RGCN_SLOT_CHUNK = 64; // k_rgcn_slots: rows up to this many slots are one thread's, longer ones a wave's

// ---- k_rgcn_slots -----------------------------------------------------------------------------------------------------------------
// the R counters of a row as eight registers: every access is an unrolled compare against a constant
struct RgcnCounts {
    int c[RGCN_MAX_RELATIONS];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int r = 0; r < RGCN_MAX_RELATIONS; r++)
            c[r] = 0;
    }
    __device__ __forceinline__ void count(int rel)
    {
#pragma unroll
        for (int r = 0; r < RGCN_MAX_RELATIONS; r++)
            c[r] += rel == r ? 1 : 0;
    }
    __device__ __forceinline__ int of(int rel) const
    {
        int n = 0;
#pragma unroll
        for (int r = 0; r < RGCN_MAX_RELATIONS; r++)
            n = rel == r ? c[r] : n;
        return n;
    }
};

// the type of CSR slot s: its COO row clamped into [0, E) as every walk of the tables clamps it
__device__ __forceinline__ int rgcn_slot_type(const int32_t *__restrict__ edge_type, const int32_t *__restrict__ eid, int s, int E)
{
    return edge_type[min(max(eid[s], 0), E - 1)];
}

// the record of a slot of type `rel` in a row with these counts; bad: the type is outside [0, R)
__device__ __forceinline__ RgcnSlot rgcn_record(int rel, const RgcnCounts &cnt, int R, bool &bad)
{
    const bool ok = (unsigned)rel < (unsigned)R;
    bad |= !ok;
    RgcnSlot o;
    o.rel = ok ? rel : 0;
    o.w = ok ? __fdiv_rn(1.0f, (float)cnt.of(rel)) : 0.0f; // (ok: the slot itself was counted, the count is >= 1)
    return o;
}

__global__ __launch_bounds__(WG) void k_rgcn_slots(const int32_t *__restrict__ edge_type, const int4 *__restrict__ node_rec,
                                                   const int32_t *__restrict__ eid, RgcnSlot *__restrict__ rec, int N, int E, int R,
                                                   int32_t *__restrict__ err, int32_t *__restrict__ err_host)
{
    const int node = blockIdx.x * WG + threadIdx.x, lane = threadIdx.x & 63;
    int rp0 = 0, deg = 0;
    if (node < N)
        row_record(node_rec, node, E, rp0, deg);
    bool bad = false;
    RgcnCounts cnt;
    if (deg <= RGCN_SLOT_CHUNK) { // (deg = 0: past the batch, or a row without in-edges)
        cnt.clear();
        for (int s = rp0; s < rp0 + deg; s++)
            cnt.count(rgcn_slot_type(edge_type, eid, s, E));
        for (int s = rp0; s < rp0 + deg; s++)
            rec[s] = rgcn_record(rgcn_slot_type(edge_type, eid, s, E), cnt, R, bad);
    }
    // the wave's long rows, one after the other, by all its lanes (wave-uniform trip counts: the ballot and the shuffles below
    // have every lane of the wave active)
    unsigned long long todo = __ballot(deg > RGCN_SLOT_CHUNK);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int lrp = __shfl(rp0, owner, 64), ldeg = __shfl(deg, owner, 64);
        cnt.clear();
        for (int s = lrp + lane; s < lrp + ldeg; s += 64)
            cnt.count(rgcn_slot_type(edge_type, eid, s, E));
#pragma unroll
        for (int r = 0; r < RGCN_MAX_RELATIONS; r++)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1)
                cnt.c[r] += __shfl_xor(cnt.c[r], d, 64);
        for (int s = lrp + lane; s < lrp + ldeg; s += 64)
            rec[s] = rgcn_record(rgcn_slot_type(edge_type, eid, s, E), cnt, R, bad);
    }
    if (__ballot(bad) != 0ull && lane == 0)
        report_flag(err, err_host, GNNB_FLAG_EDGE_TYPE);
}

hipError_t launch_rgcn_slots(const BatchTables &t, const int32_t *edge_type, int relations, RgcnSlot *rec, hipStream_t s)
{
    if (relations < 1 || relations > RGCN_MAX_RELATIONS || (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull ||
        (t.num_edges > 0 && (!edge_type || !rec)))
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0 || t.num_edges <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_rgcn_slots, dim3((unsigned)((t.num_nodes + WG - 1) / WG)), dim3(WG), 0, s, edge_type, t.node_rec, t.eid, rec, t.num_nodes,
                       t.num_edges, relations, t.err, t.err_host_dev);
    return hipGetLastError();
}

// ---- k_rgcn_aggregate -------------------------------------------------------------------------------------------------------------
// the CSR slots [k, k + ATT_R) below k1: source rows clamped into [0, N), relations into [0, R); a slot at or past k1 reads
// nothing and gets weight 0
__device__ __forceinline__ void rgcn_load_slots(const int32_t *__restrict__ col, const RgcnSlot *__restrict__ rec, int k, int k1, int N, int R,
                                                int (&j)[ATT_R], int (&rel)[ATT_R], float (&w)[ATT_R])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        j[r] = 0, rel[r] = 0, w[r] = 0.0f;
        if (k + r < k1) {
            const int2 q = *reinterpret_cast<const int2 *>(rec + (k + r));
            j[r] = min(max(col[k + r], 0), N - 1);
            rel[r] = min(max(q.x, 0), R - 1);
            w[r] = __int_as_float(q.y);
        }
    }
}

// the first n of ATT_R neighbours' rows (the lane's columns of the slot's relation block), all loads issued side by side; the
// others zeros
template <int VEC, int T>
__device__ __forceinline__ void rgcn_load_rows(const float *__restrict__ px, int ldp, const int (&j)[ATT_R], const int (&rel)[ATT_R], int n, int gl,
                                               int glog2, int wd, float (&pj)[ATT_R][T * VEC])
{
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        if (r < n) {
            att_load_row<VEC, T>(px, (size_t)j[r], ldp, rel[r] * wd, gl, glog2, wd, pj[r]);
        } else {
#pragma unroll
            for (int c = 0; c < T * VEC; c++)
                pj[r][c] = 0.0f;
        }
    }
}

// one batch: the batch rule of the header
template <int NC>
__device__ __forceinline__ void rgcn_take_batch(const float (&pj)[ATT_R][NC], const float (&w)[ATT_R], float (&acc)[NC])
{
#pragma unroll
    for (int c = 0; c < NC; c++) {
        float t = acc[c];
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            t = fmaf(w[r], pj[r][c], t);
        acc[c] = t;
    }
}

// the CSR slots [k0, k1) taken into the accumulators in batches of ATT_R, in slot order
template <int VEC, int T>
__device__ __forceinline__ void rgcn_piece(const float *__restrict__ px, int ldp, const int32_t *__restrict__ col, const RgcnSlot *__restrict__ rec,
                                           int k0, int k1, int N, int R, int gl, int glog2, int wd, float (&acc)[T * VEC])
{
    for (int s = k0; s < k1; s += ATT_R) {
        int j[ATT_R], rel[ATT_R];
        float w[ATT_R], pj[ATT_R][T * VEC];
        rgcn_load_slots(col, rec, s, k1, N, R, j, rel, w);
        rgcn_load_rows<VEC, T>(px, ldp, j, rel, k1 - s, gl, glog2, wd, pj);
        rgcn_take_batch<T * VEC>(pj, w, acc);
    }
}

template <int VEC, int T, int ACT>
__global__ __launch_bounds__(WG) void k_rgcn_aggregate(const float *__restrict__ px, int ldp, int R, const RgcnSlot *__restrict__ rec,
                                                        const float *__restrict__ root, int ldr, const float *__restrict__ skip,
                                                        float *__restrict__ out, const int4 *__restrict__ node_rec,
                                                        const int32_t *__restrict__ col, int N, int E, int wd, int glog2, int iters)
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
    // the row's own terms (the lane's columns; zeros where absent -- finish does not add those)
    auto load_own = [&](int node, float (&rt)[NC], float (&sk)[NC]) {
#pragma unroll
        for (int c = 0; c < NC; c++)
            rt[c] = 0.0f, sk[c] = 0.0f;
        if (root != nullptr)
            att_load_row<VEC, T>(root, (size_t)node, ldr, 0, gl, glog2, wd, rt);
        if (skip != nullptr)
            att_load_row<VEC, T>(skip, (size_t)node, wd, 0, gl, glog2, wd, sk);
    };
    // the epilogue of row `node` and the store
    auto finish = [&](int node, const float (&acc)[NC], const float (&rt)[NC], const float (&sk)[NC]) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < wd) {
                float o[VEC];
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = acc[t * VEC + u];
                if (root != nullptr) { // (an absent term adds nothing, not + 0)
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += rt[t * VEC + u];
                }
                if (skip != nullptr) {
#pragma unroll
                    for (int u = 0; u < VEC; u++)
                        o[u] += sk[t * VEC + u];
                }
#pragma unroll
                for (int u = 0; u < VEC; u++)
                    o[u] = act_t<ACT>(o[u]);
                row_store_nt<VEC>(out + (size_t)node * wd + c, o);
            }
        }
    };
    // ---- rows of at most ATT_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1 are
    // requested in front of the rows of step `it`, whose own record and slots arrived a step ago
    int n0, rp_0, dg_0, n1, rp_1, dg_1;
    int j0[ATT_R], rl0[ATT_R];
    float w0[ATT_R];
    row_of(0, n0, rp_0, dg_0);
    rgcn_load_slots(col, rec, rp_0, rp_0 + (dg_0 <= ATT_CHUNK ? dg_0 : 0), N, R, j0, rl0, w0);
    row_of(1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int n2, rp_2, dg_2, j1[ATT_R], rl1[ATT_R];
        float w1[ATT_R];
        row_of(it + 2, n2, rp_2, dg_2);
        rgcn_load_slots(col, rec, rp_1, rp_1 + (dg_1 <= ATT_CHUNK ? dg_1 : 0), N, R, j1, rl1, w1);
        any_long |= dg_0 > ATT_CHUNK;
        if (n0 < N && dg_0 <= ATT_CHUNK) {
            float pj[ATT_R][NC], acc[NC], rt[NC], sk[NC];
            rgcn_load_rows<VEC, T>(px, ldp, j0, rl0, dg_0, gl, glog2, wd, pj);
            load_own(n0, rt, sk);
#pragma unroll
            for (int c = 0; c < NC; c++)
                acc[c] = 0.0f;
            if (dg_0 > 0)
                rgcn_take_batch<NC>(pj, w0, acc);
            if (dg_0 > ATT_R)
                rgcn_piece<VEC, T>(px, ldp, col, rec, rp_0 + ATT_R, rp_0 + dg_0, N, R, gl, glog2, wd, acc);
            finish(n0, acc, rt, sk);
        }
        n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            j0[r] = j1[r], rl0[r] = rl1[r], w0[r] = w1[r];
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
            float acc[NC]; // (the owner's, the pieces in their order onto 0; the others' copy is not used)
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
                    rgcn_piece<VEC, T>(px, ldp, col, rec, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, R, gl, glog2, wd, part);
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
            if (grp == g) {
                float rt[NC], sk[NC];
                load_own(ln, rt, sk);
                finish(ln, acc, rt, sk);
            }
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long row)
    }
}

hipError_t launch_rgcn_aggregate(const BatchTables &t, const RgcnSlot *rec, const float *p, int ldp, int relations, const float *root, int ldr,
                                 const float *skip, int act, float *out, int width, hipStream_t s)
{
    if (width < 1 || width > RGCN_MAX_WIDTH || relations < 1 || relations > RGCN_MAX_RELATIONS || ldp < relations * width ||
        (root && ldr < width) || ((uintptr_t)rec & 7) != 0 || (uint64_t)std::max(t.num_nodes, 0) > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    if (!p || !out || (t.num_edges > 0 && !rec))
        return hipErrorInvalidValue;
    const AttForm fm = att_form(width, {p, root, skip, out}, {ldp, root ? ldr : 0});
    const int steps = att_item_steps(t.num_nodes, 1, fm);
    auto by_act = [&](auto a) {
        att_by_form(fm, width, [&](auto vec, auto strides) {
            auto kern = k_rgcn_aggregate<decltype(vec)::value, decltype(strides)::value, decltype(a)::value>;
            const AttGrid g = att_grid(kern, steps, RGCN_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, p, ldp, relations, rec, root, ldr, skip, out, t.node_rec, t.col, t.num_nodes,
                               t.num_edges, width, fm.glog2, g.iters);
        });
    };
    GNNB_DISPATCH_ACT(act, by_act);
    return hipGetLastError();
}

} // namespace gnnb
