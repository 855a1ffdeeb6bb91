// k_transformer_edge.hip -- TransformerConv with edge features: the scaled dot-product scores with their edge term, the
// per-destination softmax and the weighted sum of the value rows and of the edge attributes in ONE pass over the edges
// (gnnb_transformer_edge.h).  Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path);
// wavefront = 64 lanes.
//
// k_transformer_edge_aggregate (models.py _TransformerEConv: PyG's TransformerConv(concat=True, beta=False, edge_dim=d,
// root_weight=True)).  With p_ij = W_e e_ij the layer is s_ij[h] = q_i[h] . (k_j[h] + p_ij[h]) / sqrt(C) and
// out_i[h] = sum_j a_ij[h] (v_j[h] + p_ij[h]) + root_i.  Both are linear in p_ij, so the kernel never forms it:
//   s_ij[h]  = (sum_c q_i[h, c] * k_j[h, c]  +  sum_d qe_i[h, d] * e_ij[d]) * scale        qe_i[h] = W_e[h]^T q_i[h], an OPERAND
//   aacc[d]  = sum_j softmax_j(s_ij[h]) * e_ij[d]                                           beside acc_c = sum_j softmax_j * v_j[h, c]
//   out_i[h, c] = act( ((acc_c + sum_d we[hC + c][d] * aacc[d]) / (l + 1e-16) + root_ic) + skip_ic )
// on the CSR-by-destination tables of the prepared batch (node_rec, col, eid) of a workspace whose tables keep explicit (v, v)
// edges: such an edge is an ordinary edge and so is its attribute row.  Per (edge, head) the edge term costs edge_dim FMAs in the
// score and edge_dim in the state; W_e is applied once per item, in the epilogue.  qe and we are separate operands: the kernel
// computes what it is given (the layer passes qe as columns of its one GEMM, gnnb_weights.h transformer_edge_fold).
//
// Work split, summation order, exp and the long rows' second walk: the contract at the top of gnnb_attn.h, on its dealing of
// items (item = row * heads + head), as k_transformer_aggregate.  What is this kernel's:
//   gathers = THREE per edge: k_j, v_j and the attribute row at edge_attr + eid[slot] * edge_dim, the same address in every lane
//             of the group (16-byte pieces when edge_dim % 4 == 0 and edge_attr is aligned): a batch's slot records carry eid; all
//             loads of a batch are issued before the first is consumed
//   kept    = q_i of the lane's columns and qe_i[h], all edge_dim values, the same in every lane of the group; the state.  W_e is
//             NOT held across the edge loop and no per-edge p_ij is formed
//   score   = per lane sum_c fma(q_c, k_jc, .); the group's sum; then fma(qe[d-1], e[d-1], ... fma(qe[0], e[0], group sum)), d
//             increasing; then ONE multiply by `scale` ("dot, then edge dot, then scale")
//   state   = AttState<NC + ED>: the attribute row is appended to the lane's columns of the value row, so aacc[d] is acc's columns
//             NC .. NC + ED and takes exactly the batch rule and the merge rule acc_c takes (att_softmax_batch, att_park, att_merge
//             as they are); starts at (-inf, 0, 0): there is no self term.  aacc is the same in every lane of the group
//   out     = t = acc_c; for d increasing t = fma(we[hC + c][d], aacc[d], t); act((t / (l + 1e-16) + root_c) + skip_c).  W_e's
//             rows of the lane's columns are read HERE, once per item, from LDS: a workgroup stages W_e (16 KB at most) once, in
//             front of its walk, behind ONE barrier -- the only one of the short-row path.  Measured against reading the rows
//             from global memory in the epilogue: 5 % (edge_dim 4) and 18 % (edge_dim 16) faster at the C3t batch, same bits
//             (DESIGN 3.2g).  A row without in-edges takes nothing: act(root_c + skip_c) with root's own bits (0 where root is
//             absent)
// With all-zero edge_attr every score and every sum has k_transformer_aggregate's value: fma(qe, 0, s) = s, fma(w, 0, acc) = acc.
// 16-byte form when q / k / v / root / skip / out and the four strides allow it.  Instantiated over edge_dim, `act` at run time
// (k_gatv2_edge's way).
#include "gnnb_attn.h"

namespace gnnb {

constexpr int TFE_WG_PER_CU = 8; // workgroups per CU the grid is cut for at most (what is resident; more items than that: grid stride)

__device__ __forceinline__ float tfe_act(int act, float v)
{
    switch (act) {
    case GNNB_ACT_RELU: return act_t<GNNB_ACT_RELU>(v);
    case GNNB_ACT_GELU: return act_t<GNNB_ACT_GELU>(v);
    case GNNB_ACT_SIGMOID: return act_t<GNNB_ACT_SIGMOID>(v);
    case GNNB_ACT_TANH: return act_t<GNNB_ACT_TANH>(v);
    default: return v;
    }
}

// the first n of ATT_R neighbours' k rows and [v row | attribute row] (the lane's columns; the attributes whole), all 3 ATT_R
// loads issued side by side; the others zeros
template <int VEC, int T, int ED>
__device__ __forceinline__ void tfe_load_rows(const float *__restrict__ kx, int ldk, const float *__restrict__ vx, int ldv,
                                              const float *__restrict__ ea, const int (&j)[ATT_R], const int (&ei)[ATT_R], int n, int hc, int gl,
                                              int glog2, int C, bool avec, float (&kj)[ATT_R][T * VEC], float (&ve)[ATT_R][T * VEC + ED])
{
    constexpr int NC = T * VEC;
#pragma unroll
    for (int r = 0; r < ATT_R; r++) {
        float vj[NC], e[ED];
#pragma unroll
        for (int c = 0; c < NC; c++)
            kj[r][c] = 0.0f, vj[c] = 0.0f;
#pragma unroll
        for (int d = 0; d < ED; d++)
            e[d] = 0.0f;
        if (r < n) {
            att_load_row<VEC, T>(kx, (size_t)j[r], ldk, hc, gl, glog2, C, kj[r]);
            att_load_row<VEC, T>(vx, (size_t)j[r], ldv, hc, gl, glog2, C, vj);
            row_load_attr<ED>(ea + (size_t)ei[r] * ED, avec, e);
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
            ve[r][c] = vj[c];
#pragma unroll
        for (int d = 0; d < ED; d++)
            ve[r][NC + d] = e[d];
    }
}

// one batch: the first n (1 .. ATT_R) of the loaded neighbours taken into the state: their scores -- dot, then edge dot, then
// scale --, then att_softmax_batch over [v | e]
template <int NC, int ED>
__device__ __forceinline__ void tfe_take_batch(const float (&kj)[ATT_R][NC], const float (&ve)[ATT_R][NC + ED], int n, const float (&q)[NC],
                                               const float (&qe)[ED], float scale, int glog2, AttState<NC + ED> &a)
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
    for (int r = 0; r < ATT_R; r++) {
        float t = att_group_sum(s[r], glog2);
#pragma unroll
        for (int d = 0; d < ED; d++)
            t = fmaf(qe[d], ve[r][NC + d], t);
        s[r] = t * scale;
    }
    att_softmax_batch<NC + ED>(s, n, ve, a);
}

// the CSR slots [k0, k1) taken into the state in batches of ATT_R, in slot order
template <int VEC, int T, int ED>
__device__ __forceinline__ void tfe_piece(const float *__restrict__ kx, int ldk, const float *__restrict__ vx, int ldv, const float *__restrict__ ea,
                                          const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int k0, int k1, int N, int E, int hc,
                                          int gl, int glog2, int C, bool avec, const float (&q)[T * VEC], const float (&qe)[ED], float scale,
                                          AttState<T * VEC + ED> &a)
{
    for (int k = k0; k < k1; k += ATT_R) {
        int j[ATT_R], ei[ATT_R];
        float kj[ATT_R][T * VEC], ve[ATT_R][T * VEC + ED];
        row_load_slots(col, eid, k, k1, N, E, j, ei);
        tfe_load_rows<VEC, T, ED>(kx, ldk, vx, ldv, ea, j, ei, k1 - k, hc, gl, glog2, C, avec, kj, ve);
        tfe_take_batch<T * VEC, ED>(kj, ve, min(k1 - k, ATT_R), q, qe, scale, glog2, a);
    }
}

// vec: bit 0 -- edge_attr rows, bit 1 -- qe rows are 16-byte pieces at 16-byte aligned addresses
template <int VEC, int T, int ED>
__global__ __launch_bounds__(WG) void k_transformer_edge_aggregate(const float *__restrict__ qx, int ldq, const float *__restrict__ kx, int ldk,
                                                                    const float *__restrict__ vx, int ldv, const float *__restrict__ qex, int ldqe,
                                                                    const float *__restrict__ root, int ldr, const float *__restrict__ skip,
                                                                    float *__restrict__ out, const float *__restrict__ ea,
                                                                    const float *__restrict__ we, int ldwe, const int4 *__restrict__ node_rec,
                                                                    const int32_t *__restrict__ col, const int32_t *__restrict__ eid, int N, int E,
                                                                    int w, int heads, int C, float scale, int act, int glog2, int vec, int iters)
{
    constexpr int NC = T * VEC, NS = NC + ED;
    __shared__ float s_part[WG * (NS + 2)]; // one round of a long row's pieces: [lane group][lane of the group][m, l, acc[NC], aacc[ED]]
    __shared__ int s_long[WG];              // per lane group: the long item of its step, or -1
    __shared__ float s_we[TF_MAX_WIDTH * ED]; // W_e [w, ED] at row stride ED, staged once per workgroup for the epilogues
    const int G = 1 << glog2, groups = WG >> glog2;
    const int grp = threadIdx.x >> glog2, gl = threadIdx.x & (G - 1);
    const bool avec = (vec & 1) != 0, qvec = (vec & 2) != 0;
    const int items = N * heads;
    for (int i = threadIdx.x; i < w * ED; i += WG)
        s_we[i] = we[(size_t)(i / ED) * ldwe + (i % ED)];
    __syncthreads(); // (the one barrier of the short-row path: every epilogue below reads s_we)
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
    auto finish = [&](int node, int hc, const AttState<NS> &a) {
        const float den = a.l + 1e-16f;
        const bool took = a.l > 0.0f; // (in-degree 0: nothing was taken, the row is root's own bits -- not 0 + root, which loses a -0)
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (gl + (t << glog2)) * VEC;
            if (c < C) {
                float o[VEC], rt[VEC], sk[VEC];
#pragma unroll
                for (int u = 0; u < VEC; u++) {
                    float s = a.acc[t * VEC + u];
#pragma unroll
                    for (int d = 0; d < ED; d++)
                        s = fmaf(s_we[(hc + c + u) * ED + d], a.acc[NC + d], s);
                    o[u] = s / den;
                }
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
                    o[u] = tfe_act(act, o[u]);
                row_store_nt<VEC>(out + (size_t)node * w + hc + c, o);
            }
        }
    };
    // ---- rows of at most ATT_CHUNK in-edges, no barrier.  Three steps are in flight per lane group, so that a step exposes ONE
    // memory latency, not the chain record -> slots -> rows: the record of step it + 2 and the first ATT_R slots of step it + 1 are
    // requested in front of the rows of step `it`, whose own record and slots arrived a step ago.  Every condition below is the
    // same in all lanes of a lane group (the cross-lane sums need the whole group)
    int i0, n0, rp_0, dg_0, i1, n1, rp_1, dg_1;
    int j0[ATT_R], e0[ATT_R];
    item_of(0, i0, n0, rp_0, dg_0);
    row_load_slots(col, eid, rp_0, rp_0 + (dg_0 <= ATT_CHUNK ? dg_0 : 0), N, E, j0, e0);
    item_of(1, i1, n1, rp_1, dg_1);
    bool any_long = false;
    for (int it = 0; it < iters; it++) {
        int i2, n2, rp_2, dg_2, j1[ATT_R], e1[ATT_R];
        item_of(it + 2, i2, n2, rp_2, dg_2);
        row_load_slots(col, eid, rp_1, rp_1 + (dg_1 <= ATT_CHUNK ? dg_1 : 0), N, E, j1, e1);
        any_long |= dg_0 > ATT_CHUNK;
        if (i0 < items && dg_0 <= ATT_CHUNK) {
            const int h = i0 - n0 * heads, hc = h * C;
            float q[NC], qe[ED], kj[ATT_R][NC], ve[ATT_R][NS];
            AttState<NS> a;
            tfe_load_rows<VEC, T, ED>(kx, ldk, vx, ldv, ea, j0, e0, dg_0, hc, gl, glog2, C, avec, kj, ve);
            att_load_row<VEC, T>(qx, (size_t)n0, ldq, hc, gl, glog2, C, q);
            row_load_attr<ED>(qex + (size_t)n0 * ldqe + h * ED, qvec, qe);
            a.clear();
            if (dg_0 > 0)
                tfe_take_batch<NC, ED>(kj, ve, min(dg_0, ATT_R), q, qe, scale, glog2, a);
            if (dg_0 > ATT_R)
                tfe_piece<VEC, T, ED>(kx, ldk, vx, ldv, ea, col, eid, rp_0 + ATT_R, rp_0 + dg_0, N, E, hc, gl, glog2, C, avec, q, qe, scale, a);
            finish(n0, hc, a);
        }
        i0 = i1, n0 = n1, rp_0 = rp_1, dg_0 = dg_1;
        i1 = i2, n1 = n2, rp_1 = rp_2, dg_1 = dg_2;
#pragma unroll
        for (int r = 0; r < ATT_R; r++)
            j0[r] = j1[r], e0[r] = e1[r];
    }
    // ---- long rows (every trip count and every barrier below is the same for the whole workgroup): a workgroup that met none is
    // done after ONE more barrier
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
            const int ln = li / heads, h = li - ln * heads, hc = h * C;
            int lrp, ldeg;
            row_record(node_rec, ln, E, lrp, ldeg);
            const int npieces = (ldeg + ATT_CHUNK - 1) / ATT_CHUNK;
            float q[NC], qe[ED];
            AttState<NS> a; // (the owner's: the pieces in their order onto the empty state; the others' copy is not used)
            att_load_row<VEC, T>(qx, (size_t)ln, ldq, hc, gl, glog2, C, q);
            row_load_attr<ED>(qex + (size_t)ln * ldqe + h * ED, qvec, qe);
            a.clear();
            for (int c0 = 0; c0 < npieces; c0 += groups) {
                const int c = c0 + grp;
                AttState<NS> part;
                part.clear();
                if (c < npieces) // (a piece below npieces holds at least one slot)
                    tfe_piece<VEC, T, ED>(kx, ldk, vx, ldv, ea, col, eid, lrp + c * ATT_CHUNK, lrp + min((c + 1) * ATT_CHUNK, ldeg), N, E, hc, gl,
                                          glog2, C, avec, q, qe, scale, part);
                att_park<NS>(s_part, part);
                __syncthreads();
                if (grp == g) {
                    const int nq = min(groups, npieces - c0); // (pieces past the row's last were parked empty and are not read)
                    for (int qq = 0; qq < nq; qq++)
                        att_merge<NS>(s_part, qq, gl, glog2, a);
                }
                __syncthreads();
            }
            if (grp == g)
                finish(ln, hc, a);
        }
        __syncthreads(); // (s_long is rewritten by the next step that meets a long item)
    }
}

hipError_t launch_transformer_edge_aggregate(const BatchTables &t, const float *q, int ldq, const float *k, int ldk, const float *v, int ldv,
                                             const float *qe, int ldqe, const float *root, int ldr, const float *skip, int act, int heads,
                                             float scale, const float *edge_attr, int edge_dim, const float *we, int ldwe, float *out, int width,
                                             hipStream_t s)
{
    if (heads < 1 || heads > TF_MAX_HEADS || width < 1 || width > TF_MAX_WIDTH || width % heads != 0 || ldq < width || ldk < width ||
        ldv < width || (root != nullptr && ldr < width) || edge_dim < 1 || edge_dim > TFE_MAX_EDGE_DIM || qe == nullptr || we == nullptr ||
        ldqe < heads * edge_dim || ldwe < edge_dim || (t.num_edges > 0 && edge_attr == nullptr) ||
        (uint64_t)std::max(t.num_nodes, 0) * (uint64_t)heads > 0x7fff0000ull)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0)
        return hipSuccess;
    const int C = width / heads;
    const AttForm fm = att_form(C, {q, k, v, root, skip, out}, {ldq, ldk, ldv, root != nullptr ? ldr : 0});
    const bool ed4 = edge_dim % 4 == 0;
    const int vec = (ed4 && ((uintptr_t)edge_attr & 15) == 0 ? 1 : 0) | (ed4 && ((uintptr_t)qe & 15) == 0 && ldqe % 4 == 0 ? 2 : 0);
    const int steps = att_item_steps(t.num_nodes, heads, fm);
    auto by_ed = [&](auto ed) {
        att_by_form(fm, C, [&](auto vc, auto strides) {
            auto kern = k_transformer_edge_aggregate<decltype(vc)::value, decltype(strides)::value, decltype(ed)::value>;
            const AttGrid g = att_grid(kern, steps, TFE_WG_PER_CU);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(WG), 0, s, q, ldq, k, ldk, v, ldv, qe, ldqe, root, root != nullptr ? ldr : width, skip,
                               out, edge_attr, we, ldwe, t.node_rec, t.col, t.eid, t.num_nodes, t.num_edges, width, heads, C, scale, act,
                               fm.glog2, vec, g.iters);
        });
    };
    switch (edge_dim) {
#define GNNB_TFE_ED(n) case n: by_ed(IntTag<n>{}); break;
    GNNB_TFE_ED(1) GNNB_TFE_ED(2) GNNB_TFE_ED(3) GNNB_TFE_ED(4) GNNB_TFE_ED(5) GNNB_TFE_ED(6) GNNB_TFE_ED(7) GNNB_TFE_ED(8)
    GNNB_TFE_ED(9) GNNB_TFE_ED(10) GNNB_TFE_ED(11) GNNB_TFE_ED(12) GNNB_TFE_ED(13) GNNB_TFE_ED(14) GNNB_TFE_ED(15) GNNB_TFE_ED(16)
#undef GNNB_TFE_ED
    }
    return hipGetLastError();
}

} // namespace gnnb
