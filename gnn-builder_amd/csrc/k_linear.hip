// k_linear.hip -- dense update on the fp32 matrix cores, generic form: k_linear (register-staged LDS tiles, any shape)
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include "gnnb_gemm.h"

namespace gnnb {

// =====================================================================================
// dense update: multi-segment  Y = act( sum_s (rs_s . A_s) W_s^T + bias + skip )
// =====================================================================================
// Reference: `linear` applied to one node vector at a time (gnn_builder_lib.h:808-905) inside
// every conv (gcn :1379, gin :1538-1544, sage, pna :2146-2147) and the MLP head
// (templates/model.cpp.jinja:454-530).  Here all M rows of the batch go through one GEMM on
// the fp32 matrix cores: v_mfma_f32_32x32x2_f32 (exact fp32 products and accumulation; gfx950
// has no xf32).  Both operands are K-contiguous ("NT" GEMM: activations [M,K] row-major,
// weights [N,K] row-major = torch Linear layout), so A and W tiles are staged identically:
// 16-B global loads -> registers -> LDS rows padded to 36 floats (conflict-free
// ds_read_b128).  One ds_read_b128 per operand feeds four MFMA k-steps: lane (i, h) holds
// k = kb+4h..kb+4h+3, and MFMA step s contracts k in {kb+s, kb+4+s} -- a permutation of the
// k order shared by A and W, which the sum does not care about.
// Segments let SAGE ([mean | x] . [Wl | Wr]^T) and PNA ([x | A | amp.A | att.A] . Wpost^T, 13F
// wide) run as ONE GEMM without materialising the concatenation in HBM: the per-row scaler is
// applied while the A tile is staged.

// RC (round 4): the row-class mode of k_linear_dma (see there) for the shapes that kernel does not take -- PNA's FIRST layer
// under a degree promise: [x | A] with F = 11, K = 55 --: rows of A and Y through rc.perm, the weight matrix and bias of the
// 128-row tile's class.  M = the length of the class-sorted space.
template <int NT, bool RC = false> // workgroup tile = 128 x (64*NT); wave tile = 64 x (32*NT)
__global__ __launch_bounds__(WG) void k_linear(GemmArgs g, const float *__restrict__ W, int ldw,
                                               const float *__restrict__ bias,
                                               const float *__restrict__ skip,
                                               float *__restrict__ Y, int M, int N, int act, RowClasses rc = RowClasses{})
{
    static_assert(BM == 128, "a row-class tile is one workgroup tile");
    if (RC) {
        const int cls = __builtin_amdgcn_readfirstlane(rc.tile_cls[blockIdx.x]);
        W += (size_t)cls * rc.w_stride;
        if (bias)
            bias += (size_t)cls * rc.bias_stride;
    }
    constexpr int BN = 64 * NT;
    constexpr int BROWS = BN / 32; // W-tile staging passes per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *As = reinterpret_cast<float *>(smem);         // [2][BM*LDS_LD]
    float *Bs = As + 2 * BM * LDS_LD;                    // [2][BN*LDS_LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    const int c4 = tid & 7;  // which float4 of the 32-wide k chunk
    const int r0 = tid >> 3; // 0..31

    f32x16 acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int ni = 0; ni < NT; ni++)
#pragma unroll
            for (int i = 0; i < 16; i++)
                acc[mi][ni][i] = 0.0f;

    float4 ra[4], rb[BROWS];
    const int total = g.cpre[g.nseg];
    int arow[4]; // (RC) the rows this thread stages: the same four in every chunk
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int pos = m0 + r0 + 32 * p;
        arow[p] = RC ? (pos < M ? rc.perm[pos] : -1) : (pos < M ? pos : -1);
    }

    auto load_chunk = [&](int c) {
        // segment lookup with static indexing only (keeps the kernarg struct out of scratch)
        const float *ap = g.a[0];
        const float *rs = g.rs[0];
        int lda = g.lda[0], ks = g.k[0], koff = g.koff[0], cbase = 0, av = g.avec[0], wv = g.wvec[0];
#pragma unroll
        for (int s = 1; s < 4; s++) {
            if (s < g.nseg && c >= g.cpre[s]) {
                ap = g.a[s];
                rs = g.rs[s];
                lda = g.lda[s];
                ks = g.k[s];
                koff = g.koff[s];
                cbase = g.cpre[s];
                av = g.avec[s];
                wv = g.wvec[s];
            }
        }
        const int kk = (c - cbase) * BK + c4 * 4;
        const int rem = ks - kk;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = arow[p];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row >= 0) {
                v = load4_guard(ap + (size_t)row * lda + kk, rem, av != 0);
                if (rs != nullptr) {
                    const float sc = rs[row];
                    v.x *= sc;
                    v.y *= sc;
                    v.z *= sc;
                    v.w *= sc;
                }
            }
            ra[p] = v;
        }
#pragma unroll
        for (int p = 0; p < BROWS; p++) {
            const int n = n0 + r0 + 32 * p;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < N)
                v = load4_guard(W + (size_t)n * ldw + koff + kk, rem, wv != 0);
            rb[p] = v;
        }
    };
    auto store_chunk = [&](int buf) {
        float *a = As + buf * BM * LDS_LD;
        float *b = Bs + buf * BN * LDS_LD;
#pragma unroll
        for (int p = 0; p < 4; p++)
            *reinterpret_cast<float4 *>(a + (r0 + 32 * p) * LDS_LD + c4 * 4) = ra[p];
#pragma unroll
        for (int p = 0; p < BROWS; p++)
            *reinterpret_cast<float4 *>(b + (r0 + 32 * p) * LDS_LD + c4 * 4) = rb[p];
    };

    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    const int li = lane & 31, lh = lane >> 5;
    for (int c = 0; c < total; c++) {
        const int buf = c & 1;
        if (c + 1 < total)
            load_chunk(c + 1); // global loads stay in flight under the MFMAs below
        const float *a = As + buf * BM * LDS_LD + (wm * 64 + li) * LDS_LD + 4 * lh;
        const float *b = Bs + buf * BN * LDS_LD + (wn * 32 * NT + li) * LDS_LD + 4 * lh;
#pragma unroll
        for (int kb = 0; kb < BK; kb += 8) {
            float4 fa[2], fb[NT];
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
                fa[mi] = *reinterpret_cast<const float4 *>(a + mi * 32 * LDS_LD + kb);
#pragma unroll
            for (int ni = 0; ni < NT; ni++)
                fb[ni] = *reinterpret_cast<const float4 *>(b + ni * 32 * LDS_LD + kb);
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
#pragma unroll
                for (int ni = 0; ni < NT; ni++) {
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].x, fb[ni].x, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].y, fb[ni].y, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].z, fb[ni].z, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi].w, fb[ni].w, acc[mi][ni], 0, 0, 0);
                }
        }
        if (c + 1 < total)
            store_chunk(buf ^ 1);
        __syncthreads();
    }

    // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    auto epilogue = [&](auto tag) {
        constexpr int ACT = decltype(tag)::value;
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int ni = 0; ni < NT; ni++) {
                const int colg = n0 + wn * 32 * NT + ni * 32 + li;
                if (colg >= N)
                    continue;
                const float bv = bias ? bias[colg] : 0.0f;
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    const int pos = m0 + wm * 64 + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
                    const int rowg = RC ? (pos < M ? rc.perm[pos] : -1) : (pos < M ? pos : -1);
                    if (rowg >= 0) {
                        float v = acc[mi][ni][reg] + bv;
                        if (skip)
                            v += skip[(size_t)rowg * N + colg];
                        Y[(size_t)rowg * N + colg] = act_t<ACT>(v);
                    }
                }
            }
    };
    GNNB_DISPATCH_ACT(act, epilogue)
}

// N <= 64 takes 64-column workgroup tiles, everything wider (and every row-class launch: M is whole class tiles) 128-column ones
hipError_t launch_linear_tiles(const GemmArgs &g, const float *w, int ldw, const float *bias, const float *skip, float *y, int M,
                               int N, int act, hipStream_t s, const RowClasses *rcp)
{
    hipError_t e = hipSuccess;
    auto go = [&](auto nttag, auto rctag) {
        constexpr int NT = decltype(nttag)::value;
        constexpr bool RC = decltype(rctag)::value != 0;
        constexpr int BN = 64 * NT;
        const size_t lds = (size_t)(2 * BM * LDS_LD + 2 * BN * LDS_LD) * 4;
        e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_linear<NT, RC>), lds);
        if (e != hipSuccess)
            return;
        hipLaunchKernelGGL((k_linear<NT, RC>), dim3((M + BM - 1) / BM, (N + BN - 1) / BN), dim3(WG), lds, s, g, w, ldw, bias, skip,
                           y, M, N, act, rcp ? *rcp : RowClasses{});
        e = hipGetLastError();
    };
    if (rcp)
        go(IntTag<2>{}, IntTag<1>{});
    else if (N > 64)
        go(IntTag<2>{}, IntTag<0>{});
    else
        go(IntTag<1>{}, IntTag<0>{});
    return e;
}

} // namespace gnnb
