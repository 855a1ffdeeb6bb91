// gnnb_head.h -- the readout's one header: the pooling selection, k_pool_mlp's swizzle and LDS carve, the launch plans of k_pool_mlp
// and k_head_small, and the MLP head on pooled rows as a device function: k_head_small (k_readout.hip) runs it as a kernel of its
// own, k_gcn2_zf (k_stack_zf.h) runs it at the end of every workgroup's life on the graphs that workgroup pooled (round 5: conv
// stack + pooling + head in ONE launch -- reference compute_gnn_head -> compute_global_graph_pooling -> compute_mlp_head inside
// one top, templates/model.cpp.jinja:737-765).
#pragma once
#include "gnnb_device.h"
#include "gnnb_stack_plan.h"

namespace gnnb {

// ---- pooling: the requested reductions in `aggrs` order, k_pool_mlp's kernel argument by value
struct PoolSel {
    int kind[3];
    int np;
};
static inline PoolSel pool_sel(const int32_t *pools, int num_pools)
{
    return PoolSel{{pools[0], num_pools > 1 ? pools[1] : 0, num_pools > 2 ? pools[2] : 0}, num_pools};
}

// (The ordered row walk -- seed from the first row, blocks of four, tail -- stays spelled in both pool kernels: as one
// pool_rows<VEC, DEEP8> / pool_pick, by reference or by value, with or without __restrict__, k_global_pool schedules its address
// arithmetic differently, and as a by-value argument PoolSel changes how it fetches its kernarg: it keeps p0, p1, p2, np.)

// ---- k_pool_mlp's LDS plan
static constexpr int HEAD_GRAPHS = 16;   // graphs per workgroup (one MFMA tile of rows), every readout form
static constexpr int HEAD_THREADS = 512; // k_pool_mlp: 8 waves, 16 graphs pooled in parallel (32 lanes each at d=128)
static constexpr size_t POOL_MLP_LDS_MAX = 158 * 1024; // (2 KB short of the CU's LDS)
static_assert(POOL_MLP_LDS_MAX <= (size_t)STACK_LDS_MAX, "k_pool_mlp's dynamic LDS is one CU's");

// largest power of two <= 16 dividing the number of 16-B chunks per row (1 = no swizzle)
__device__ inline int head_swz_p(int k)
{
    if (k & 3)
        return 1;
    const int c = k >> 2;
    int p = 1;
    while (p < 16 && (c % (2 * p)) == 0)
        p *= 2;
    return p;
}
// float offset of element (row, k) in a [rows][kdim] LDS image with 16-B chunks XOR-swizzled
__device__ inline int head_off(int row, int k, int kdim, int P)
{
    return row * kdim + ((((k >> 2) ^ (row & (P - 1))) << 2) | (k & 3));
}

// Carve (floats): two activation buffers [16][widest layer they hold] -- layer l reads buffer l & 1 and writes buffer (l + 1) & 1,
// buffer 0 holds the pooled tile -- then every layer's matrix with its bias right behind it.  Filled by pool_mlp_carve on the
// host, read by the kernel as one by-value argument.
struct PoolMlpCarve {
    int act0, act1; // floats of the two activation buffers
    int woff[8];    // layer l's matrix, in floats behind the activation buffers
    size_t bytes;   // everything
    __host__ __device__ static size_t bias_off(int n, int k) { return ((size_t)n * k + 3) & ~(size_t)3; } // behind the [n][k] matrix
    size_t total() const { return bytes; }
    bool fits() const { return bytes <= POOL_MLP_LDS_MAX; }
};
static inline PoolMlpCarve pool_mlp_carve(const HeadArgs &head)
{
    PoolMlpCarve c = {};
    int maxw[2] = {4, 4};
    for (int l = 0; l <= head.nlin; l++)
        maxw[l & 1] = std::max(maxw[l & 1], (int)head.dims[l]);
    c.act0 = (HEAD_GRAPHS * maxw[0] + 3) & ~3;
    c.act1 = (HEAD_GRAPHS * maxw[1] + 3) & ~3;
    size_t wfl = 0;
    for (int l = 0; l < head.nlin; l++) {
        c.woff[l] = (int)wfl;
        wfl += PoolMlpCarve::bias_off(head.dims[l + 1], head.dims[l]) + (((size_t)head.dims[l + 1] + 3) & ~(size_t)3);
    }
    c.bytes = ((size_t)c.act0 + c.act1 + wfl) * 4;
    return c;
}

// launch_pool_mlp (k_pool_mlp, from the node matrix x or from a pooled matrix).  The first row that applies:
//   | condition                                                                  | result            |
//   |----------------------------------------------------------------------------|-------------------|
//   | option fuse_head off; nlin outside 1..8; d % 4 != 0                        | not supported     |
//   | the source (x / pooled) or a weight matrix not 16-B aligned                | not supported     |
//   | from a pooled matrix and dims[0] % 4 != 0                                  | not supported     |
//   | the carve does not fit POOL_MLP_LDS_MAX                                    | not supported     |
//   | otherwise                                                                  | carve, lds = carve.total() |
struct PoolMlpPlan {
    bool ok = false;
    PoolMlpCarve carve = {};
};
static inline PoolMlpPlan plan_pool_mlp(bool fuse_head, const HeadArgs &head, int d, const float *src, bool from_pooled)
{
    PoolMlpPlan p;
    if (!fuse_head || head.nlin < 1 || head.nlin > 8 || (d & 3) || (((uintptr_t)src & 15) != 0))
        return p;
    if (from_pooled && (head.dims[0] & 3))
        return p;
    for (int l = 0; l < head.nlin; l++)
        if (((uintptr_t)head.w[l] & 15) != 0)
            return p;
    p.carve = pool_mlp_carve(head);
    p.ok = p.carve.fits();
    return p;
}

// ---- the small-footprint head (operands from L2): shape test and LDS
static constexpr int HS_MAXW = 128; // widest hidden layer this form takes

// Host side: does the head take this form?  (float4 operand fetches: widths % 4, 16-B aligned weights; hidden activations
// live in a 16 x ldact LDS tile.)  Returns ldact (floats per activation row) or 0.
static inline int head_small_ldact(const HeadArgs &head)
{
    if (head.nlin < 1 || head.nlin > 8)
        return 0;
    for (int l = 0; l < head.nlin; l++) {
        if ((head.dims[l] & 3) || (((uintptr_t)head.w[l]) & 15))
            return 0;
        if (l > 0 && head.dims[l] > HS_MAXW)
            return 0;
    }
    int maxw = 4;
    for (int l = 1; l < head.nlin; l++)
        maxw = std::max(maxw, (int)head.dims[l]);
    return ((maxw + 3) & ~3) + 4;
}
static inline size_t head_small_lds_bytes(int ldact) { return (size_t)2 * 16 * ldact * 4; } // per group of four waves
// launch_head_small (k_head_small on a pooled matrix).  The first row that applies:
//   | condition                                                                  | result            |
//   |----------------------------------------------------------------------------|-------------------|
//   | no pooled matrix, or not 16-B aligned                                      | not supported     |
//   | nlin outside 1..8; a width dims[0 .. nlin - 1] % 4 != 0; a weight matrix not 16-B aligned; a hidden width > HS_MAXW | not supported |
//   | otherwise                                                                  | ldact = widest hidden layer + 4 |
static inline int plan_head_small(const HeadArgs &head, const float *pooled)
{
    return (!pooled || (((uintptr_t)pooled) & 15)) ? 0 : head_small_ldact(head);
}

// ---- the head on pooled rows, operands from L2
// (head_small_run keeps its own k loop and both run functions their own epilogue: as one head_tile_mma<UW> / one epilogue function --
// tried with the row pointer or the operand fetch chosen by the caller, the offset as a functor, base and offset passed apart, the
// chains by value -- k_head_small and k_gcn2_zf<HEAD> come out with other schedules or register assignments; they are budgeted)
// One 16 x 16 output tile of one linear over the k range [k_lo, k_hi) (multiples of 16, or k): acc += A[16 graphs][k] . W[nn][k]^T,
// v_mfma_f32_16x16x4_f32, four accumulator chains over interleaved 16-wide k blocks, every operand fetch of a 64-wide k step in
// flight at once.  arow = this lane's A row (+ 4 lg), wrow = its W row (+ 4 lg); k = the row length (a float4 past it is zero).
__device__ __forceinline__ void head_tile_mma(const float *arow, const float *wrow, int k, int k_lo, int k_hi, f32x4 (&accs)[4])
{
    const int lg = (threadIdx.x & 63) >> 4;
    for (int kb = k_lo; kb < k_hi; kb += 64) {
        float4 a[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int kk = kb + 16 * u; // (+ 4 lg inside the row pointers)
            const bool ok = kk < k_hi && kk + 4 * lg < k; // k % 4 == 0: a float4 is whole or absent
            const int kc = ok ? kk : 0;
            w[u] = *reinterpret_cast<const float4 *>(wrow + kc);
            a[u] = *reinterpret_cast<const float4 *>(arow + kc);
            if (!ok)
                a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
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
}

// The head at the END of a conv-stack workgroup's life (k_gcn2_zf), written for LATENCY: nothing else runs on the CU then, so
// every global round trip is paid in full.  The stand-alone form walks layer 0's K = np d (384 at BASELINE config 2) in six
// dependent steps of 64; here the workgroup's NGRP groups of four waves split that K between them -- each wave fetches its
// whole share at once: ONE round trip --, park their partial tiles in LDS and add them up in group order (deterministic).
// Later layers (K <= 128: one or two steps) run on group 0 as in the stand-alone form.  Tiles of 16 graphs one after the other
// (a workgroup pools 16 graphs at BASELINE config 2).  spart: LDS [NGRP][16][ldact], sact: LDS [2][16][ldact].
template <int ACT, int NGRP, typename Barrier>
__device__ __forceinline__ void head_tail_run(const float *__restrict__ pooled, int g_begin, int g_end, const HeadArgs &head,
                                              float *__restrict__ out, int ldact, float *spart, float *sact, int tid, Barrier bar)
{
    const int lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wave >> 2, gw = wave & 3;
    const int ntile = (g_end - g_begin + 15) >> 4;
#pragma unroll 1
    for (int it = 0; it < ntile; it++) {
        const int g0 = g_begin + it * 16;
        const int grow = max(min(g0 + li, g_end - 1), 0); // (rows past the range re-read its last graph and are dropped at the store)
        // ---- layer 0, K split over the groups
        {
            const int k = head.dims[0], n = head.dims[1];
            const int kshare = (((k + 15) >> 4) + NGRP - 1) / NGRP * 16; // whole 16-wide blocks per group
            const int k_lo = min(grp * kshare, k), k_hi = min(k_lo + kshare, k);
            const float *__restrict__ W = head.w[0];
            for (int sl = gw; sl * 16 < n; sl += 4) {
                const int nn = sl * 16 + li;
                const int nnc = nn < n ? nn : n - 1;
                f32x4 accs[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                head_tile_mma(pooled + (size_t)grow * k + 4 * lg, W + (size_t)nnc * k + 4 * lg, k, k_lo, k_hi, accs);
                if (nn < n) {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        spart[(grp * 16 + lg * 4 + r) * ldact + nn] = (accs[0][r] + accs[1][r]) + (accs[2][r] + accs[3][r]);
                }
            }
            bar();
            const float *__restrict__ bias = head.b[0];
            const bool last = head.nlin == 1;
            for (int e = tid; e < 16 * n; e += NGRP * 256) {
                const int gi = e / n, nn = e - gi * n;
                float v = spart[gi * ldact + nn];
#pragma unroll
                for (int g = 1; g < NGRP; g++)
                    v += spart[(g * 16 + gi) * ldact + nn];
                v += bias ? bias[nn] : 0.0f;
                if (last) {
                    if (g0 + gi < g_end)
                        out[(size_t)(g0 + gi) * n + nn] = v;
                } else {
                    sact[gi * ldact + nn] = act_t<ACT>(v);
                }
            }
            bar();
        }
        // ---- later layers on group 0 (activations in LDS)
        int cur = 0;
#pragma unroll 1
        for (int l = 1; l < head.nlin; l++) {
            const int k = head.dims[l], n = head.dims[l + 1];
            const bool last = (l == head.nlin - 1);
            const float *__restrict__ W = head.w[l];
            const float *__restrict__ bias = head.b[l];
            for (int sl = wave; sl * 16 < n; sl += NGRP * 4) { // (one 16-column slice per wave: n <= 128 fits sixteen or eight waves)
                const int nn = sl * 16 + li;
                const int nnc = nn < n ? nn : n - 1;
                f32x4 accs[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                head_tile_mma(sact + (cur * 16 + li) * ldact + 4 * lg, W + (size_t)nnc * k + 4 * lg, k, 0, k, accs);
                if (nn < n) {
                    const float bvv = bias ? bias[nn] : 0.0f;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int gi = lg * 4 + r;
                        const float v = (accs[0][r] + accs[1][r]) + (accs[2][r] + accs[3][r]) + bvv;
                        if (last) {
                            if (g0 + gi < g_end)
                                out[(size_t)(g0 + gi) * n + nn] = v;
                        } else {
                            sact[((cur ^ 1) * 16 + gi) * ldact + nn] = act_t<ACT>(v);
                        }
                    }
                }
            }
            bar();
            cur ^= 1;
        }
    }
}

// One GROUP of four waves takes tiles of 16 graphs: tile index tile0 + it * tile_stride for it = 0 .. iters - 1, graphs
// g_begin + 16 tile ... (< g_end).  Every linear as 16 x 16 MFMA tiles (v_mfma_f32_16x16x4_f32): wave gw of the group takes the
// 16-column output slices gw, gw + 4, ...; A = the pooled rows straight from L2 (layer 0) or the activations in LDS, B = the
// weights straight from L2 (shared by every workgroup); four accumulator chains over interleaved 16-wide k blocks.
// `bar()` is the barrier that every wave of the WORKGROUP reaches once per layer and iteration -- groups without a tile
// still call it (iters is workgroup-uniform).  sact: this group's LDS tile [2][16][ldact].
// UW: k slices of a 64-wide block fetched and multiplied together -- 2 (default: the 72-register form, below) or 4 (82 registers, more
// loads in flight: ~2 us faster when the kernel has the chip to itself; option head_pairs = 0).  Same accumulators, same sums.
template <int ACT, int UW = 2, typename Barrier>
__device__ __forceinline__ void head_small_run(const float *__restrict__ pooled, int g_begin, int g_end, const HeadArgs &head,
                                               float *__restrict__ out, int ldact, float *sact, int lane, int gw, int tile0,
                                               int tile_stride, int iters, Barrier bar)
{
    const int li = lane & 15, lg = lane >> 4;
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
        const int g0 = g_begin + (tile0 + it * tile_stride) * 16;
        const bool on = g0 < g_end;                          // (wave-uniform)
        const int grow = max(min(g0 + li, g_end - 1), 0);    // (rows past the range re-read its last graph and are dropped at the store)
        int cur = 0;
#pragma unroll 1
        for (int l = 0; l < head.nlin; l++) {
            const int k = head.dims[l], n = head.dims[l + 1];
            const bool last = (l == head.nlin - 1);
            const float *__restrict__ W = head.w[l];
            const float *__restrict__ bias = head.b[l];
            for (int sl = gw; on && sl * 16 < n; sl += 4) {
                const int nn = sl * 16 + li;
                const int nnc = nn < n ? nn : n - 1;
                const float *wrow = W + (size_t)nnc * k + 4 * lg;
                const float *arow_g = pooled + (size_t)grow * k + 4 * lg;          // layer 0: A straight from the pooled matrix
                const float *arow_l = sact + (cur * 16 + li) * ldact + 4 * lg;     // later layers: from LDS
                f32x4 accs[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    accs[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                // The four k slices of a 64-wide block are fetched and multiplied as TWO PAIRS (round 6): half the operand registers of
                // the four-at-once form, the same four accumulators and the same sums in the same order (bit-identical results).
                // What it buys is the stand-alone kernel's register count, 82 -> 67: beside four 96-register waves of k_gcn2_zf a SIMD
                // has 128 registers left, and a 72-register readout wave + a 56-register graph-prep wave now fit TOGETHER.
                // (no operand double-buffering either: the register budget is what lets the stand-alone kernel share a SIMD with the
                // conv-stack kernel of another batch, and inside k_gcn2_zf it must stay below that kernel's own budget)
                static_assert(UW == 2 || UW == 4, "operand group width");
                for (int kb = 0; kb < k; kb += 64) {
#pragma unroll
                    for (int hp = 0; hp < 4 / UW; hp++) {
                        float4 a[UW], w[UW];
#pragma unroll
                        for (int u2 = 0; u2 < UW; u2++) {
                            const int kk = kb + 16 * (UW * hp + u2); // (+ 4 lg inside the row pointers)
                            const bool ok = kk + 4 * lg < k;         // k % 4 == 0: a float4 is whole or absent
                            const int kc = ok ? kk : 0;
                            w[u2] = *reinterpret_cast<const float4 *>(wrow + kc);
                            a[u2] = l == 0 ? *reinterpret_cast<const float4 *>(arow_g + kc)  // layer 0: A straight from the pooled matrix
                                           : *reinterpret_cast<const float4 *>(arow_l + kc); // later layers: from LDS
                            if (!ok)
                                a[u2] = make_float4(0.f, 0.f, 0.f, 0.f);
                        }
#pragma unroll
                        for (int u2 = 0; u2 < UW; u2++)
                            accs[UW * hp + u2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u2].x, w[u2].x, accs[UW * hp + u2], 0, 0, 0);
#pragma unroll
                        for (int u2 = 0; u2 < UW; u2++)
                            accs[UW * hp + u2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u2].y, w[u2].y, accs[UW * hp + u2], 0, 0, 0);
#pragma unroll
                        for (int u2 = 0; u2 < UW; u2++)
                            accs[UW * hp + u2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u2].z, w[u2].z, accs[UW * hp + u2], 0, 0, 0);
#pragma unroll
                        for (int u2 = 0; u2 < UW; u2++)
                            accs[UW * hp + u2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u2].w, w[u2].w, accs[UW * hp + u2], 0, 0, 0);
                    }
                }
                // C/D: col = lane&15 (output column nn), row = (lane>>4)*4 + r (graph inside the tile)
                if (nn < n) {
                    const float bvv = bias ? bias[nn] : 0.0f;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int gi = lg * 4 + r;
                        const float v = (accs[0][r] + accs[1][r]) + (accs[2][r] + accs[3][r]) + bvv;
                        if (last) {
                            if (g0 + gi < g_end)
                                out[(size_t)(g0 + gi) * n + nn] = v;
                        } else {
                            sact[((cur ^ 1) * 16 + gi) * ldact + nn] = act_t<ACT>(v);
                        }
                    }
                }
            }
            bar();
            cur ^= 1;
        }
    }
}

} // namespace gnnb
