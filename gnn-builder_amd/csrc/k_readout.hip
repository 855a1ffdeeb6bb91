// k_readout.hip -- per-graph add / mean / max pooling + MLP head: k_global_pool, k_pool_mlp, k_head_small
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include <algorithm>
#include <cstring>

#include "gnnb_device.h"
#include "gnnb_head.h"
#include "gnnb_prep.h"

namespace gnnb {

// =====================================================================================
// global pooling
// =====================================================================================
// Reference: global_add_pool / global_mean_pool / global_max_pool
// (gnn_builder_lib.h:2709-2739, :2741-2771, :2773-2803) concatenated in `aggrs` order
// (templates/model.cpp.jinja:440-448; gnnbuilder/models.py:348-352).  One lane group
// (d/4 lanes, float4 each) owns one graph and walks its node rows in order, so the sum
// order equals the reference's; all requested reductions come from a single read of x.
template <int VEC>
__global__ __launch_bounds__(WG) void k_global_pool(const float *__restrict__ x,
                                                    const int32_t *__restrict__ node_ptr, int B,
                                                    int d, int glog2, int p0, int p1, int p2,
                                                    int np, float *__restrict__ out)
{
    typedef Vf<VEC> V;
    const int G = 1 << glog2;
    const int grp = threadIdx.x >> glog2;
    const int gl = threadIdx.x & (G - 1);
    const int g = blockIdx.x * (WG >> glog2) + grp;
    if (g >= B)
        return;
    const int n0 = node_ptr[g], n1 = node_ptr[g + 1];
    const int nvec = d / VEC;
    const int pools[3] = {p0, p1, p2};
    for (int f = gl; f < nvec; f += G) {
        const int fo = f * VEC;
        V sum = V::splat(0.0f), mx = V::splat(0.0f);
        int i = n0;
        if (i < n1) {
            const V v = V::load(x + (size_t)i * d + fo);
            sum = v;
            mx = v;
            i++;
        }
        for (; i + 3 < n1; i += 4) {
            const V a = V::load(x + (size_t)i * d + fo);
            const V b = V::load(x + (size_t)(i + 1) * d + fo);
            const V c = V::load(x + (size_t)(i + 2) * d + fo);
            const V e = V::load(x + (size_t)(i + 3) * d + fo);
            sum = vadd(vadd(vadd(vadd(sum, a), b), c), e);
            mx = vmax(vmax(mx, a), vmax(b, vmax(c, e)));
        }
        for (; i < n1; i++) {
            const V v = V::load(x + (size_t)i * d + fo);
            sum = vadd(sum, v);
            mx = vmax(mx, v);
        }
        const int n = n1 - n0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (k >= np)
                break;
            V r = sum;
            if (pools[k] == GNNB_POOL_MEAN)
                r = n > 0 ? vdiv(sum, V::splat((float)n)) : V::splat(0.0f);
            else if (pools[k] == GNNB_POOL_MAX)
                r = mx;
            r.store(out + (size_t)g * np * d + (size_t)k * d + fo);
        }
    }
}

hipError_t launch_global_pool(const float *x, const int32_t *node_ptr, int num_graphs, int d,
                              const int32_t *pools, int num_pools, float *out, hipStream_t s)
{
    if (num_graphs <= 0)
        return hipSuccess;
    const bool v4 = (d % 4 == 0) && (((uintptr_t)x & 15) == 0) && (((uintptr_t)out & 15) == 0);
    const int nvec = v4 ? d / 4 : d;
    const int glog2 = lane_group_log2(nvec, 2);
    const int per_wg = WG >> glog2;
    const int grid = (num_graphs + per_wg - 1) / per_wg;
    const PoolSel sel = pool_sel(pools, num_pools);
    hipLaunchKernelGGL((v4 ? k_global_pool<4> : k_global_pool<1>), dim3(grid), dim3(WG), 0, s, x, node_ptr, num_graphs, d, glog2,
                       sel.kind[0], sel.kind[1], sel.kind[2], sel.np, out);
    return hipGetLastError();
}


// =====================================================================================
// fused readout: global pooling + MLP head
// =====================================================================================
// Reference: compute_global_graph_pooling + compute_mlp_head (templates/model.cpp.jinja:413-530;
// global_*_pool gnn_builder_lib.h:2709-2803; MLP gnnbuilder/models.py:398-430).  As separate
// launches the head is three GEMMs with M = B rows (32 workgroups on a 256-CU chip) behind a
// pooling pass that writes and re-reads [B, k*d].  Here one workgroup owns 16 graphs:
//   0. fires the LDS-DMA of ALL head weights (they fit LDS: 119 KB at the BASELINE configs),
//   1. pools its graphs' node rows (the only HBM-sized read) into a [16, k*d] LDS tile while the
//      weights land -- one lane group per graph, rows in order, so the sum order is the reference's,
//   2. runs every linear as 16 x n MFMA tiles (v_mfma_f32_16x16x4_f32, A and W fragments both
//      from LDS, XOR-swizzled rows), activations staying in LDS,
//   3. writes [16, OUT].
// The pooled tile and the hidden activations never touch HBM.
// (tile and thread counts, the swizzle and the LDS carve: gnnb_head.h)
template <int ACT>
__global__ __launch_bounds__(HEAD_THREADS) void k_pool_mlp(const float *__restrict__ x,
                                                 const int32_t *__restrict__ node_ptr, int B, int d,
                                                 int glog2, PoolSel sel, HeadArgs head, float *__restrict__ out,
                                                 const float *__restrict__ prepooled, PoolMlpCarve carve)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // buffer 0 holds the pooled tile and every even layer's output, buffer 1 the odd ones
    // (LDS pointers derived arithmetically from smem: a runtime-indexed pointer array turns the
    // accesses into FLAT loads that wait on vmcnt)
    float *const act_lo = reinterpret_cast<float *>(smem);
    float *wbase = reinterpret_cast<float *>(smem) + (size_t)carve.act0 + carve.act1;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int g0 = blockIdx.x * HEAD_GRAPHS;

    GNNB_STAMP(0);
    // ---- 0. all weights (+ biases) -> LDS: row-wise linear DMA, swizzle applied on the source side
#pragma unroll 1
    for (int l = 0; l < head.nlin; l++) {
        const int k = head.dims[l], n = head.dims[l + 1];
        const float *W = head.w[l];
        float *dstf = wbase + carve.woff[l];
        if ((k & 3) == 0) {
            const int C = k >> 2, P = head_swz_p(k), nch = n * C;
            for (int c0 = wave * 64; c0 < nch; c0 += (HEAD_THREADS / 64) * 64) {
                const int L = c0 + lane;
                if (L < nch) {
                    const int r = L / C, sl = L - r * C;
                    dma16_to_lds(W + (size_t)r * k + ((sl ^ (r & (P - 1))) << 2),
                                 reinterpret_cast<char *>(dstf) + (size_t)c0 * 16);
                }
            }
        } else {
            const int nd = n * k;
            for (int c0 = wave * 64; c0 < nd; c0 += (HEAD_THREADS / 64) * 64)
                if (c0 + lane < nd)
                    dma4_to_lds(W + c0 + lane, reinterpret_cast<char *>(dstf) + (size_t)c0 * 4);
        }
        // bias right behind its matrix (zeros when the layer has none)
        float *dstb = dstf + PoolMlpCarve::bias_off(n, k);
        if (head.b[l] != nullptr) {
            for (int c0 = wave * 64; c0 < n; c0 += (HEAD_THREADS / 64) * 64)
                if (c0 + lane < n)
                    dma4_to_lds(head.b[l] + c0 + lane, reinterpret_cast<char *>(dstb) + (size_t)c0 * 4);
        } else {
            for (int i = tid; i < n; i += HEAD_THREADS)
                dstb[i] = 0.0f;
        }
    }
    GNNB_STAMP(1);
    if (prepooled != nullptr) {
        // ---- 1'. the pooled tile already exists ([B, k*d], written by the fused conv stack): DMA this
        // workgroup's 16 rows into the swizzled LDS tile
        const int k0 = head.dims[0], C0 = k0 >> 2, P0 = head_swz_p(k0);
        const int rows = min(HEAD_GRAPHS, B - g0), nch = rows * C0;
        for (int c0 = wave * 64; c0 < nch; c0 += (HEAD_THREADS / 64) * 64) {
            const int L = c0 + lane;
            if (L < nch) {
                const int r = L / C0, sl = L - r * C0;
                dma16_to_lds(prepooled + (size_t)(g0 + r) * k0 + ((sl ^ (r & (P0 - 1))) << 2),
                             reinterpret_cast<char *>(act_lo) + (size_t)c0 * 16);
            }
        }
    } else
    // ---- 1. pooling: one lane group per graph, rows in order
    {
        const int G = 1 << glog2, groups = HEAD_THREADS >> glog2;
        const int grp = tid >> glog2, gl = tid & (G - 1);
        const int k0 = head.dims[0], P0 = head_swz_p(k0);
        const int nvec = d >> 2;
        for (int gi = grp; gi < HEAD_GRAPHS; gi += groups) {
            const int g = g0 + gi;
            const int n0 = g < B ? node_ptr[g] : 0, n1 = g < B ? node_ptr[g + 1] : 0;
            for (int f = gl; f < nvec; f += G) {
                const int fo = f * 4;
                typedef Vf<4> V;
                V sum = V::splat(0.0f), mx = V::splat(0.0f);
                int i = n0;
                if (i < n1) {
                    sum = V::load(x + (size_t)i * d + fo);
                    mx = sum;
                    i++;
                }
                for (; i + 7 < n1; i += 8) { // eight independent 16-B loads in flight per lane
                    V r8[8];
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        r8[u] = V::load(x + (size_t)(i + u) * d + fo);
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        sum = vadd(sum, r8[u]); // row order kept: the reference's sum order
                        mx = vmax(mx, r8[u]);
                    }
                }
                for (; i + 3 < n1; i += 4) {
                    const V a = V::load(x + (size_t)i * d + fo);
                    const V b = V::load(x + (size_t)(i + 1) * d + fo);
                    const V c = V::load(x + (size_t)(i + 2) * d + fo);
                    const V e = V::load(x + (size_t)(i + 3) * d + fo);
                    sum = vadd(vadd(vadd(vadd(sum, a), b), c), e);
                    mx = vmax(vmax(mx, a), vmax(b, vmax(c, e)));
                }
                for (; i < n1; i++) {
                    const V v = V::load(x + (size_t)i * d + fo);
                    sum = vadd(sum, v);
                    mx = vmax(mx, v);
                }
                const int n = n1 - n0;
#pragma unroll
                for (int kk = 0; kk < 3; kk++) {
                    if (kk >= sel.np)
                        break;
                    V r = sum;
                    if (sel.kind[kk] == GNNB_POOL_MEAN)
                        r = n > 0 ? vdiv(sum, V::splat((float)n)) : V::splat(0.0f);
                    else if (sel.kind[kk] == GNNB_POOL_MAX)
                        r = mx;
                    r.store(act_lo + head_off(gi, kk * d + fo, k0, P0));
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F); // (lgkmcnt(0): pooled tile written)
    GNNB_STAMP(2);
    __syncthreads(); // drains vmcnt: weights have landed; pooled tile complete
    GNNB_STAMP(3);

    // ---- 2. the linears
    int cur = 0;
#pragma unroll 1
    for (int l = 0; l < head.nlin; l++) {
        const int k = head.dims[l], n = head.dims[l + 1];
        const bool last = (l == head.nlin - 1);
        const int Pk = head_swz_p(k), Pn = head_swz_p(n);
        const float *sA = reinterpret_cast<const float *>(smem) + (cur ? carve.act0 : 0);
        float *sY = reinterpret_cast<float *>(smem) + (cur ? 0 : carve.act0);
        const float *sW = wbase + carve.woff[l];
        const float *sbias = sW + PoolMlpCarve::bias_off(n, k); // staged next to the matrix
        const bool vec = (k & 3) == 0;
        for (int sl = wave; sl * 16 < n; sl += HEAD_THREADS / 64) {
            const int nn = sl * 16 + li; // this lane's output column (B-fragment row of W)
            // four independent accumulator chains over interleaved 16-wide k blocks: the LDS reads of
            // four blocks are issued together and the MFMAs never wait on each other
            f32x4 accs[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                accs[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
            auto frag = [&](int kb, float4 &a, float4 &w) {
                const int kk = kb + 4 * lg;
                a = make_float4(0.f, 0.f, 0.f, 0.f);
                w = a;
                if (vec) {
                    if (kk < k) {
                        a = *reinterpret_cast<const float4 *>(sA + head_off(li, kk, k, Pk));
                        if (nn < n)
                            w = *reinterpret_cast<const float4 *>(sW + head_off(nn, kk, k, Pk));
                    }
                } else {
                    const float *pa = sA + li * k + kk;
                    const float *pw = sW + (size_t)nn * k + kk;
                    a.x = kk + 0 < k ? pa[0] : 0.f;
                    a.y = kk + 1 < k ? pa[1] : 0.f;
                    a.z = kk + 2 < k ? pa[2] : 0.f;
                    a.w = kk + 3 < k ? pa[3] : 0.f;
                    if (nn < n) {
                        w.x = kk + 0 < k ? pw[0] : 0.f;
                        w.y = kk + 1 < k ? pw[1] : 0.f;
                        w.z = kk + 2 < k ? pw[2] : 0.f;
                        w.w = kk + 3 < k ? pw[3] : 0.f;
                    }
                }
            };
            // fast path (wave-uniform): every 64-wide k block is whole -> unguarded loads that are all
            // in flight together (a lane-dependent guard makes the compiler wait at each join); an
            // out-of-range output column re-reads the last valid W row and is dropped at the store
            const bool kfast = vec && (k % 64 == 0);
            const int nnc = nn < n ? nn : n - 1;
            for (int kb = 0; kb < k; kb += 64) {
                float4 a[4], w[4];
                if (kfast) {
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int kk = kb + 16 * u + 4 * lg;
                        a[u] = *reinterpret_cast<const float4 *>(sA + head_off(li, kk, k, Pk));
                        w[u] = *reinterpret_cast<const float4 *>(sW + head_off(nnc, kk, k, Pk));
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        frag(kb + 16 * u, a[u], w[u]); // blocks past k come back as zeros
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, w[u].x, accs[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, w[u].y, accs[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, w[u].z, accs[u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, w[u].w, accs[u], 0, 0, 0);
            }
            f32x4 acc;
#pragma unroll
            for (int r = 0; r < 4; r++)
                acc[r] = (accs[0][r] + accs[1][r]) + (accs[2][r] + accs[3][r]);
            // C/D: col = lane&15 (output column nn), row = (lane>>4)*4 + r (graph inside the tile)
            if (nn < n) {
                const float bvv = sbias[nn];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int gi = lg * 4 + r;
                    const float v = acc[r] + bvv;
                    if (last) {
                        if (g0 + gi < B)
                            out[(size_t)(g0 + gi) * n + nn] = v;
                    } else {
                        sY[(n & 3) == 0 ? head_off(gi, nn, n, Pn) : gi * n + nn] = act_t<ACT>(v);
                    }
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
#ifdef GNNB_PROBE
    if (threadIdx.x == 0 && blockIdx.x < 8192) {
        g_probe[blockIdx.x * 8 + 1] = wall_clock64(); // overwrite slot-0 cycle word: end time
    }
#endif
}

// -------------------------------------------------------------------------------------
// Readout on a pooled matrix, small-footprint form.  k_pool_mlp keeps every weight in LDS (119 KB at the
// BASELINE configs): fast on an idle chip, but when batches are in flight on several streams it cannot
// start on a CU until BOTH resident workgroups of the next batch's conv-stack kernel have left, and while
// it runs nothing else fits -- measured cost 12.5 us per step at C2 for 10.5 us of kernel.  This form
// needs ~9 KB of LDS and < 96 registers, so its 4-wave workgroups slot in BESIDE the conv-stack kernel
// (31 KB of LDS and one wave slot of 96 registers per SIMD are left over there): weights and the pooled
// rows are MFMA operands fetched straight from L2 (the pooled matrix was just written, the head's weights
// are shared by all workgroups), only the 16 x width activations between layers live in LDS.
// One workgroup = 16 graphs; wave w takes the 16-column output slices w, w + 4, ...
static constexpr int HS_THREADS = 256;

// GUEST (gnnb_forward_prepared_prep_next): the graph prep of the stream's NEXT batch -- COO -> CSR, node records,
// normalisers, tile tables of ANOTHER workspace (gnnb_prep.h: one wavefront per graph, <= 64 nodes each by that workspace's
// promise) -- as EXTRA WORKGROUPS of this launch: blocks [0, prep_blocks) prepare four graphs each, the rest run the head.  The
// prep is a chain of dependent fetches (its graph's table entries, its edges, then a few hundred instructions and the
// stores: ~6 us from launch to the last store) that occupies almost nothing; as a launch of its own beside the stack kernels
// of the other streams' batches it cost the three-stream pipeline ~4.5 us of a 42-us step.  Here it starts with the first
// blocks of a kernel that runs ~11 us anyway.  (Tried first inside k_gcn2_zf, on the waves that idle through the last stage's
// aggregation phase: that window is 2 us, the chain -- even with its fetches hoisted into the kernel's prologue -- outlasts
// it by 4 us, and the stack kernel is the pipeline's critical resource: no gain)
// The parameter block is the kernel's FIRST argument and is never named: the prep blocks read it from the kernarg segment
// (offset 0), the head blocks never fetch it.
// The three forms and their register budgets (the launcher's table picks one):
//   plain, PAIRS     72 (a launch bound of seven waves per SIMD; 67 used).  Beside k_gcn2_zf's four 96-register waves a SIMD has
//                    128 registers left: this kernel's wave and a graph-prep wave (56) of the stream's next batch then run side by
//                    side instead of one after the other -- BASELINE config 2, three batches in flight: 40.4-41.6 -> 37.6-37.7 us
//                    per step.
//   plain, !PAIRS    (option head_pairs = 0) four operand slices in flight, 82 registers, five waves per SIMD -- the faster form
//                    when NOTHING shares the chip (one stream of forwards: 49.8 vs 51.9 us per forward at BASELINE config 2),
//                    the slower one in the pipeline.
//   GUEST (PAIRS)    carries the prep's code: five waves per SIMD.
static constexpr int HS_WAVES = 7; // waves per SIMD of the plain, paired-operand form
template <int ACT, bool GUEST, bool PAIRS = true>
__global__ __launch_bounds__(HS_THREADS, (GUEST || !PAIRS) ? 5 : HS_WAVES) void k_head_small(PrepParams guest_kernarg, int prep_blocks, const float *__restrict__ pooled, int B,
                                                             HeadArgs head, float *__restrict__ out, int ldact)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __builtin_amdgcn_s_setprio(GNNB_GUEST_PRIO); // (co-runs with the next batch's conv-stack kernel: see k_graph_prep)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if constexpr (GUEST) {
        if ((int)blockIdx.x < prep_blocks) {
            const PrepParams gp = *kernarg_prep_params();
            prep_graph_group<64, 4>(gp, (blockIdx.x * (HS_THREADS / 64) + wave) * 4, lane, reinterpret_cast<int32_t *>(smem) + wave * prep_wave_lds_ints(64));
            return;
        }
    }
    float *sact = reinterpret_cast<float *>(smem); // [2][16][ldact]: ldact = widest hidden layer + 4 (padded rows)
    // one workgroup = one group of four waves = one tile of 16 graphs (gnnb_head.h)
    head_small_run<ACT, PAIRS ? 2 : 4>(pooled, 0, B, head, out, ldact, sact, lane, wave, (int)blockIdx.x - (GUEST ? prep_blocks : 0), 0, 1,
                                       [] { __syncthreads(); });
}

// the readout's three options, each read here only
struct ReadoutOpts {
    bool fuse_head, head_small, head_pairs;
};
static ReadoutOpts readout_opts() { return ReadoutOpts{options().fuse_head != 0, options().head_small != 0, options().head_pairs != 0}; }
bool readout_small_enabled() { return readout_opts().fuse_head && readout_opts().head_small; }

// hipErrorNotSupported when the head's shape does not suit the small form (plan_head_small; the ladder goes on to k_pool_mlp)
static hipError_t launch_head_small(const float *pooled, int num_graphs, const HeadArgs &head, int act, float *out, hipStream_t s)
{
    const int ldact = plan_head_small(head, pooled);
    if (ldact <= 0)
        return hipErrorNotSupported;
    const int grid = (num_graphs + HEAD_GRAPHS - 1) / HEAD_GRAPHS;
    // a guest graph prep on offer (gnnb_forward_prepared_prep_next)?
    GuestPrep *const gslot = guest_prep_slot();
    const bool guest = gslot && gslot->params && !gslot->taken && gslot->params->max_graph_nodes_hint > 0 && gslot->params->max_graph_nodes_hint <= 64;
    PrepParams gp;
    memset(&gp, 0, sizeof(gp));
    int prep_blocks = 0;
    if (guest) {
        gp = *gslot->params;
        prep_blocks = prep_grid_blocks(gp.B + 1, 4, HS_THREADS);
    }
    const size_t lds = std::max(head_small_lds_bytes(ldact), guest ? (HS_THREADS / 64) * prep_wave_lds_ints(64) * sizeof(int32_t) : (size_t)0);
    const bool pairs = readout_opts().head_pairs;
    auto go = [&](auto tag) {
        constexpr int ACT = decltype(tag)::value;
        // (guest, pairs) -> form: the guest form is paired whatever the option says
        auto kern = guest ? k_head_small<ACT, true, true> : pairs ? k_head_small<ACT, false, true> : k_head_small<ACT, false, false>;
        hipLaunchKernelGGL(kern, dim3(grid + prep_blocks), dim3(HS_THREADS), lds, s, gp, prep_blocks, pooled, num_graphs, head, out, ldact);
    };
    GNNB_DISPATCH_ACT(act, go)
    const hipError_t rc = hipGetLastError();
    if (guest && rc == hipSuccess)
        gslot->taken = true;
    return rc;
}

// k_pool_mlp from the node matrix (pooled == nullptr) or from the pooled matrix (x, node_ptr == nullptr)
static hipError_t launch_pool_mlp(const float *x, const int32_t *node_ptr, const float *pooled, int num_graphs, int d, PoolSel sel,
                                  const HeadArgs &head, int act, float *out, hipStream_t s)
{
    const PoolMlpPlan p = plan_pool_mlp(readout_opts().fuse_head, head, d, pooled ? pooled : x, pooled != nullptr);
    if (!p.ok)
        return hipErrorNotSupported; // (a head too large for LDS among the reasons: the caller uses pool + GEMMs)
    const size_t lds = p.carve.total();
    const int glog2 = lane_group_log2(d >> 2, 2);
    const int grid = (num_graphs + HEAD_GRAPHS - 1) / HEAD_GRAPHS;
    auto go = [&](auto tag) {
        constexpr int ACT = decltype(tag)::value;
        auto kern = k_pool_mlp<ACT>;
        (void)ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(HEAD_THREADS), lds, s, x, node_ptr, num_graphs, d, glog2, sel, head, out, pooled, p.carve);
    };
    GNNB_DISPATCH_ACT(act, go)
    return hipGetLastError();
}

hipError_t launch_readout_fused(const float *x, const int32_t *node_ptr, int num_graphs, int d, const int32_t *pools, int num_pools,
                                const HeadArgs &head, int act, float *out, hipStream_t s)
{
    if (num_graphs <= 0)
        return hipSuccess;
    return launch_pool_mlp(x, node_ptr, nullptr, num_graphs, d, pool_sel(pools, num_pools), head, act, out, s);
}

hipError_t launch_readout_pooled(const float *pooled, int num_graphs, int d, const HeadArgs &head, int act, float *out, hipStream_t s)
{
    if (num_graphs <= 0)
        return hipSuccess;
    if (readout_small_enabled()) {
        const hipError_t e = launch_head_small(pooled, num_graphs, head, act, out, s);
        if (e != hipErrorNotSupported)
            return e;
    }
    return launch_pool_mlp(nullptr, nullptr, pooled, num_graphs, d, PoolSel{}, head, act, out, s);
}

} // namespace gnnb
