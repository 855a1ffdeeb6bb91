// k_linear_reg.hip -- dense update on the fp32 matrix cores for K <= 128, weights in registers: k_linear_reg, plain and with the
// fused gather of a narrow first conv layer (launch_conv_gather instantiates the same kernel)
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include "gnnb_gemm.h"

namespace gnnb {

// -------------------------------------------------------------------------------------
// Register-resident-weight variant for K <= 128 (every full-width layer of the d<=128 models, the
// first layer, the MLP head's 64-wide linears).  The weight matrix is tiny next to the activation
// stream, so each wave keeps ITS 32 output columns x K of W in VGPRs for the whole kernel (K/2
// registers) and the workgroup is persistent: it walks a contiguous range of 16-row units, the A
// rows arriving through a double-buffered LDS stage filled by LDS-DMA (global_load_lds) while the
// previous stage is on the matrix cores.  v_mfma_f32_16x16x4_f32 (exact fp32) gives a 16-row
// scheduling quantum, which keeps the persistent ranges balanced.  LDS rows are XOR-swizzled by
// pre-swizzling the DMA *source* address (the DMA destination is lane-linear), which makes the
// ds_read_b128 fragment reads conflict-free:  slot = chunk ^ (row & (P-1)).
// Lane (i = l&15, g = l>>4) reads chunk 4q+g of row i: k = 16q+4g .. +3; MFMA step (q,s) contracts
// k in {16q + 4g + s : g = 0..3}, the same k-permutation on A and W.
static constexpr int LR_SR = 2; // 16-row units per stage


// Optional fused gather: when `rec` is set the A stage is not copied from memory but PRODUCED -- the
// workgroup aggregates its destination rows (GCN / sum / mean semantics of k_aggregate_*) from the
// raw feature matrix straight into the LDS stage.  Used for narrow first layers (F_in = 9, 11):
// the gather touches 44-byte rows that live in L2, so the separate aggregate launch and its
// [N, F_in] round trip through memory disappear (reference gcn_conv / gin_conv do the same per
// node: aggregate, then `linear`, gnn_builder_lib.h:1346-1379, :1497-1544).
struct GatherDesc {
    const int4 *rec;     // node records {rp0, deg, j0, j1}{j2, j3, -, -}; nullptr = plain A copy
    const int32_t *col;  // CSR sources (degree > 4)
    const float *dinv;   // GCN normaliser
    int32_t mode;        // gnnb_agg (GCN, SUM, MEAN)
    float eps;
    int32_t cat;         // > 0: the stage row is [aggregate(x)(cat wide) | x_i (cat wide)]  (GraphSAGE: [mean | x], K = 2 cat)
};

// MATH 1 (opt-in, K % 32 == 0, N % 32 == 0, plain A copy): the products go through the bf16 matrix cores as six
// partial products of an exact 3-way split (see split3); A fragments are split in the wave after the LDS read.
template <int KQ, bool VEC_A, int MATH = 0> // KQ = ceil(K/16) in {1,2,4,8}; VEC_A: K % 4 == 0 and 16-B aligned rows
__global__ __launch_bounds__(WG, MATH ? 2 : 3) void k_linear_reg(
    const float *__restrict__ A, int lda, int K, const float *__restrict__ W, int ldw,
    const float *__restrict__ bias, const float *__restrict__ skip, float *__restrict__ Y, int M, int N,
    int act, int rg_log2, int P, int vec_out, GatherDesc gd)
{
    constexpr int SR = LR_SR;
    constexpr int EPI_LD = 36; // padded row of the epilogue transpose scratch
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int RG = 1 << rg_log2;     // row groups: waves that take different rows
    const int cw = wave >> rg_log2;  // which 32-column slice this wave owns
    const int rgi = wave & (RG - 1); // which row group
    const int n0 = blockIdx.y * (128 >> rg_log2) + cw * 32;
    const int unit_rows = 16 * RG;
    const int stage_rows = SR * unit_rows;
    const size_t buf_bytes = (((size_t)stage_rows * K * 4) + 15) & ~(size_t)15;
    float *sC = reinterpret_cast<float *>(smem + 2 * buf_bytes) + (size_t)wave * 16 * SR * EPI_LD;

    // ---- persistent range, balanced in UNITS of 16*RG rows (half a stage), so the remainder a
    // workgroup may carry is half a stage.  Local stage j covers units [u0+2j, min(u0+2j+2, u1)).
    const int num_units = (M + unit_rows - 1) / unit_rows;
    int u0, u1;
    run_cuts(blockIdx.x, gridDim.x, (unsigned)num_units, u0, u1); // (32-bit: gnnb_device.h)
    if (u1 <= u0)
        return;
    const int nstages = (u1 - u0 + SR - 1) / SR;
    const int C = K >> 2; // 16-B chunks per row (VEC_A)
    auto row_begin = [&](int j) { return (u0 + SR * j) * unit_rows; };
    auto rows_of = [&](int j) { return min(min(u0 + SR * j + SR, u1) * unit_rows, M) - (u0 + SR * j) * unit_rows; };

    // ---- this wave's weight slice -> registers
    float breg[2][KQ * 4];
    constexpr int KB = KQ / 2 > 0 ? KQ / 2 : 1; // 32-wide k blocks (MATH 1)
    u32x4 wh[2][KB], wm[2][KB], wl_[2][KB];
    // fast path (wave-uniform): the 32 x K slice is in range and 16-B aligned.  Its rows are read
    // whole (coalesced LDS-DMA) into this wave's share of the not-yet-used stage buffers and picked
    // apart into fragments from LDS; fragment-shaped global loads (16 rows x 64 B per instruction)
    // took ~2 us per workgroup and serialised co-resident workgroups' start.
    const bool wfast = VEC_A && (ldw % 4 == 0) && (K == 16 * KQ) && (n0 + 32 <= N) && (((uintptr_t)W & 15) == 0);
    if (wfast) {
        float *wl = reinterpret_cast<float *>(smem) + (size_t)wave * 16 * K; // 4 x 16*K floats <= 2 buffers
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int nrow0 = n0 + 16 * u;
            const int nch = 16 * C;
            for (int c0 = 0; c0 < nch; c0 += 64) {
                const int L = c0 + lane;
                if (L < nch) {
                    const int rr = L / C, cc = L - rr * C;
                    dma16_to_lds(W + (size_t)(nrow0 + rr) * ldw + cc * 4, reinterpret_cast<char *>(wl) + (size_t)c0 * 16);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // own DMA, wave-private region: no barrier
            if (MATH) { // lane (li, lg) of a 16x16x32 MFMA holds k = 32 kb + 8 lg .. + 7 of column li
#pragma unroll
                for (int kb = 0; kb < KB; kb++) {
                    const float4 f0 = *reinterpret_cast<const float4 *>(wl + (size_t)li * K + 32 * kb + 8 * lg);
                    const float4 f1 = *reinterpret_cast<const float4 *>(wl + (size_t)li * K + 32 * kb + 8 * lg + 4);
                    split3x8(f0, f1, wh[u][kb], wm[u][kb], wl_[u][kb]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < KQ; q++) {
                    const float4 v = *reinterpret_cast<const float4 *>(wl + (size_t)li * K + 16 * q + 4 * lg);
                    breg[u][q * 4 + 0] = v.x;
                    breg[u][q * 4 + 1] = v.y;
                    breg[u][q * 4 + 2] = v.z;
                    breg[u][q * 4 + 3] = v.w;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // fragments read before the region is reused
        }
    } else {
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int n = n0 + 16 * u + li;
#pragma unroll
            for (int q = 0; q < KQ; q++) {
                const int k = 16 * q + 4 * lg;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < N)
                    v = load4_guard(W + (size_t)n * ldw + k, K - k, VEC_A && (ldw % 4 == 0));
                breg[u][q * 4 + 0] = v.x;
                breg[u][q * 4 + 1] = v.y;
                breg[u][q * 4 + 2] = v.z;
                breg[u][q * 4 + 3] = v.w;
            }
        }
    }
    float bv[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int n = n0 + 16 * u + li;
        bv[u] = (bias != nullptr && n < N) ? bias[n] : 0.0f;
    }
    // loop-invariant epilogue operands, loaded ONCE: a global load inside the stage loop would make
    // its s_waitcnt also wait for the next stage's DMA (VM operations retire in order)
    const int c4 = (lane & 7) * 4;
    const int nq = n0 + c4;
    float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec_out && bias != nullptr && nq < N)
        bq = *reinterpret_cast<const float4 *>(bias + nq);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(bq.x), "+v"(bq.y), "+v"(bq.z), "+v"(bq.w), "+v"(bv[0]), "+v"(bv[1])::"memory");
    __syncthreads(); // every wave is out of the stage buffers (weight prologue) before A lands there

    auto issue = [&](int j, int bb) {
        char *dst = smem + (size_t)bb * buf_bytes;
        const int m0i = row_begin(j);
        const int rows = rows_of(j);
        if (VEC_A) {
            const int nchunks = rows * C;
            for (int c0 = wave * 64; c0 < nchunks; c0 += 4 * 64) {
                const int L = c0 + lane;
                if (L < nchunks) {
                    const int i = L / C, sl = L - i * C;
                    const int c = sl ^ (i & (P - 1));
                    dma16_to_lds_u(A + (size_t)(m0i + i) * lda + c * 4, dst + (size_t)c0 * 16);
                }
            }
        } else {
            const int nd = rows * K;
            for (int c0 = wave * 64; c0 < nd; c0 += 4 * 64) {
                const int L = c0 + lane;
                if (L < nd) {
                    const int i = L / K, kk = L - i * K;
                    dma4_to_lds_u(A + (size_t)(m0i + i) * lda + kk, dst + (size_t)c0 * 4);
                }
            }
        }
    };

#ifdef GNNB_PROBE
    unsigned long long pt_wait = 0, pt_mma = 0, pt_epi = 0, pt0 = clock64(), pw0 = wall_clock64();
    unsigned long long pt_last = pt0;
#endif
    // Stores count in vmcnt on CDNA4 and VM operations retire in order.  A full stage's vector
    // epilogue issues EXACTLY four 16-B stores per wave after the next stage's DMA, so waiting for
    // vmcnt <= 4 proves that DMA has landed while the stores stay in flight; anything irregular
    // (ragged stage, scalar epilogue, a wave without columns) falls back to a full drain.
    const bool wave_has_cols = nq < N || (n0 < N); // some lane of this wave stores
    const bool gather = !VEC_A && gd.rec != nullptr; // workgroup-uniform
    // gather producer: element (row i, feature f) of stage j, neighbours in CSR order, self term last
    auto produce = [&](int j, int bb) {
        float *dst = reinterpret_cast<float *>(smem + (size_t)bb * buf_bytes);
        const int m0i = row_begin(j);
        const int rows = rows_of(j);
        for (int e = tid; e < rows * K; e += WG) {
            const int i = e / K, fk = e - i * K;
            const int node = m0i + i;
            // (GraphSAGE form: columns [0, cat) hold the aggregate, columns [cat, 2 cat) the node's own row)
            const bool own = gd.cat > 0 && fk >= gd.cat;
            const int f = own ? fk - gd.cat : fk;
            const int4 r0 = gd.rec[2 * (size_t)node], r1 = gd.rec[2 * (size_t)node + 1];
            const int deg = r0.y;
            const int jn[4] = {r0.z, r0.w, r1.x, r1.y};
            const float xs = A[(size_t)node * lda + f];
            float xv[4], sv[4];
            const float di = gd.mode == GNNB_AGG_GCN ? gd.dinv[node] : 1.0f;
#pragma unroll
            for (int q = 0; q < 4; q++) { // unused slots alias the node itself (cache hit, discarded)
                xv[q] = A[(size_t)jn[q] * lda + f];
                sv[q] = gd.mode == GNNB_AGG_GCN ? gd.dinv[jn[q]] : 1.0f;
            }
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (deg > q)
                    acc += xv[q] * (di * sv[q]);
            for (int k = r0.x + 4; k < r0.x + deg; k++) {
                const int jj = gd.col[k];
                acc += A[(size_t)jj * lda + f] * (di * (gd.mode == GNNB_AGG_GCN ? gd.dinv[jj] : 1.0f));
            }
            if (gd.mode == GNNB_AGG_GCN)
                acc += xs * (di * di);
            else if (gd.mode == GNNB_AGG_SUM)
                acc += xs * (1.0f + gd.eps);
            else if (deg > 0)
                acc = acc / (float)deg;
            if (own)
                acc = xs;
            dst[e] = acc;
        }
    };
    bool prev_counted = false;
    if (gather)
        produce(0, 0);
    else
        issue(0, 0);
    int b = 0;
    for (int j = 0; j < nstages; j++, b ^= 1) {
        if (prev_counted) {
            static_assert(2 * SR == 4, "a full stage's vector epilogue issues 2 * SR 16-B stores per wave: the counted wait names that number");
            asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (j + 1 < nstages) {
            if (gather)
                produce(j + 1, b ^ 1); // plain loads + ds_write; the next barrier publishes it
            else
                issue(j + 1, b ^ 1);
        }
        GNNB_PT(pt_wait, pt_last);
        const float *sA = reinterpret_cast<const float *>(smem + (size_t)b * buf_bytes);
        const int m0 = row_begin(j);
        const int m_end = m0 + rows_of(j); // rows past it belong to another workgroup (or nobody)

        f32x4 acc[SR][2];
#pragma unroll
        for (int rt = 0; rt < SR; rt++)
#pragma unroll
            for (int u = 0; u < 2; u++)
                acc[rt][u] = (f32x4){0.f, 0.f, 0.f, 0.f};

        if (MATH) {
#pragma unroll
            for (int kb = 0; kb < KB; kb++) {
                u32x4 ah[SR], am[SR], al[SR];
#pragma unroll
                for (int rt = 0; rt < SR; rt++) {
                    const int row = (rt * RG + rgi) * 16 + li;
                    const int c0 = 8 * kb + 2 * lg; // float4 chunks 8 kb + 2 lg, + 1 of the row
                    const float4 f0 = *reinterpret_cast<const float4 *>(sA + (size_t)row * K + ((c0 ^ (row & (P - 1))) << 2));
                    const float4 f1 = *reinterpret_cast<const float4 *>(sA + (size_t)row * K + (((c0 + 1) ^ (row & (P - 1))) << 2));
                    split3x8(f0, f1, ah[rt], am[rt], al[rt]);
                }
                // six partial products, smallest first; the four accumulators interleaved
#define GNNB_BF6(APIECE, BPIECE)                                                                                  \
    _Pragma("unroll") for (int rt = 0; rt < SR; rt++) _Pragma("unroll") for (int u = 0; u < 2; u++)                \
        acc[rt][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(APIECE[rt]), as_bf16x8(BPIECE[u][kb]), acc[rt][u], 0, 0, 0);
                GNNB_BF6(am, wm)
                GNNB_BF6(al, wh)
                GNNB_BF6(ah, wl_)
                GNNB_BF6(am, wh)
                GNNB_BF6(ah, wm)
                GNNB_BF6(ah, wh)
#undef GNNB_BF6
            }
        } else {
#pragma unroll
            for (int q = 0; q < KQ; q++) {
                float4 a[SR];
    #pragma unroll
                for (int rt = 0; rt < SR; rt++) {
                    const int row = (rt * RG + rgi) * 16 + li; // row inside the stage: unit rt, row group rgi
                    if (VEC_A) {
                        const int c = 4 * q + lg;
                        a[rt] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (c < C)
                            a[rt] = *reinterpret_cast<const float4 *>(sA + (size_t)row * K + ((c ^ (row & (P - 1))) << 2));
                    } else {
                        const int k = 16 * q + 4 * lg;
                        const float *pr = sA + (size_t)row * K + k;
                        a[rt].x = (k + 0 < K) ? pr[0] : 0.f;
                        a[rt].y = (k + 1 < K) ? pr[1] : 0.f;
                        a[rt].z = (k + 2 < K) ? pr[2] : 0.f;
                        a[rt].w = (k + 3 < K) ? pr[3] : 0.f;
                    }
                }
                // k-step outermost: consecutive MFMAs hit the four different accumulators, so the 40-cycle
                // dependent latency of v_mfma_f32_16x16x4_f32 hides behind its 32-cycle issue interval
                float as[SR][4];
    #pragma unroll
                for (int rt = 0; rt < SR; rt++) {
                    as[rt][0] = a[rt].x;
                    as[rt][1] = a[rt].y;
                    as[rt][2] = a[rt].z;
                    as[rt][3] = a[rt].w;
                }
    #pragma unroll
                for (int sk = 0; sk < 4; sk++)
    #pragma unroll
                    for (int rt = 0; rt < SR; rt++)
    #pragma unroll
                        for (int u = 0; u < 2; u++)
                            acc[rt][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(as[rt][sk], breg[u][q * 4 + sk], acc[rt][u], 0, 0, 0);
            }
        }
#ifdef GNNB_PROBE
        asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[SR - 1][1][3]));
#endif
        GNNB_PT(pt_mma, pt_last);
        // epilogue: C/D of the 16x16 MFMA: col = lane&15, row = (lane>>4)*4 + reg
        const bool full = (m_end - m0) == stage_rows;
        prev_counted = vec_out && full && wave_has_cols && (skip == nullptr) && !gather;
        auto epilogue = [&](auto tag) {
            constexpr int ACT = decltype(tag)::value;
            if (vec_out) {
                // transpose the wave's 32x32 block through its LDS scratch, then 4 x (ds_read_b128 +
                // 16-B global store) instead of 16 dword stores: 8 lanes cover one 128-B row segment
#pragma unroll
                for (int rt = 0; rt < SR; rt++)
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            sC[(rt * 16 + lg * 4 + r) * EPI_LD + u * 16 + li] = acc[rt][u][r];
                // (same wave wrote and reads: the compiler's lgkmcnt wait orders it; no barrier)
#pragma unroll
                for (int ps = 0; ps < 2 * SR; ps++) {
                    const int rl = ps * 8 + (lane >> 3); // row inside the wave's 16*SR (unit rl>>4)
                    const int m = m0 + ((rl >> 4) * RG + rgi) * 16 + (rl & 15);
                    float4 v = *reinterpret_cast<const float4 *>(sC + rl * EPI_LD + c4);
                    if (m < m_end && nq < N) {
                        v.x += bq.x;
                        v.y += bq.y;
                        v.z += bq.z;
                        v.w += bq.w;
                        if (skip) {
                            const float4 sk = *reinterpret_cast<const float4 *>(skip + (size_t)m * N + nq);
                            v.x += sk.x;
                            v.y += sk.y;
                            v.z += sk.z;
                            v.w += sk.w;
                        }
                        v.x = act_t<ACT>(v.x);
                        v.y = act_t<ACT>(v.y);
                        v.z = act_t<ACT>(v.z);
                        v.w = act_t<ACT>(v.w);
                        *reinterpret_cast<float4 *>(Y + (size_t)m * N + nq) = v;
                    }
                }
            } else {
#pragma unroll
                for (int rt = 0; rt < SR; rt++)
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int n = n0 + 16 * u + li;
                        if (n >= N)
                            continue;
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int m = m0 + (rt * RG + rgi) * 16 + lg * 4 + r;
                            if (m < m_end) {
                                float v = acc[rt][u][r] + bv[u];
                                if (skip)
                                    v += skip[(size_t)m * N + n];
                                Y[(size_t)m * N + n] = act_t<ACT>(v);
                            }
                        }
                    }
            }
        };
        GNNB_DISPATCH_ACT(act, epilogue)
        GNNB_PT(pt_epi, pt_last);
    }
#ifdef GNNB_PROBE
    if (tid == 0 && blockIdx.x < 8192 && blockIdx.y == 0) {
        unsigned long long *o = g_probe + blockIdx.x * 8;
        o[0] = pw0;
        o[1] = wall_clock64();
        o[2] = pt_wait;
        o[3] = pt_mma;
        o[4] = pt_epi;
        o[5] = clock64() - pt0;
        o[6] = (unsigned long long)nstages;
    }
#endif
}

template <int KQ, bool VEC_A, int MATH = 0>
static hipError_t launch_linear_reg_t(const float *A, int lda, int K, const float *W, int ldw,
                                      const float *bias, const float *skip, float *Y, int M, int N,
                                      int act, hipStream_t s, const GatherDesc &gd = GatherDesc{})
{
    if (MATH == 0 && VEC_A && KQ >= 2 && launch_math() != 0 && K == 16 * KQ && N % 32 == 0 && ldw % 4 == 0 &&
        (((uintptr_t)W & 15) == 0) && gd.rec == nullptr)
        return launch_linear_reg_t<KQ, VEC_A, 1>(A, lda, K, W, ldw, bias, skip, Y, M, N, act, s, gd);
    // waves: N <= 32 -> 4 row groups x 1 column slice; N <= 64 -> 2 x 2; else 1 x 4 (128 cols / WG)
    const int rg_log2 = N <= 32 ? 2 : (N <= 64 ? 1 : 0);
    const int cols_per_wg = 128 >> rg_log2;
    const int stage_rows = (16 * LR_SR) << rg_log2;
    const int gy = (N + cols_per_wg - 1) / cols_per_wg;
    const size_t buf = (((size_t)stage_rows * K * 4) + 15) & ~(size_t)15;
    const size_t lds = 2 * buf + 4 * 16 * LR_SR * 36 * 4; // two stage buffers + per-wave epilogue scratch
    const int vec_out = (N % 4 == 0) && (((uintptr_t)Y & 15) == 0) && (bias == nullptr || ((uintptr_t)bias & 15) == 0) &&
                        (skip == nullptr || ((uintptr_t)skip & 15) == 0);
    int P = 1;
    if (VEC_A) {
        const int C = K / 4;
        while (P < 16 && C % (2 * P) == 0)
            P *= 2;
    }
    const int num_stages = (M + stage_rows - 1) / stage_rows;
    auto kern = k_linear_reg<KQ, VEC_A, MATH>;
    {
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess)
            return e;
    }
    // persistent grid = what is resident at once (registers + LDS), asked of the runtime once per
    // LDS size and capped (MI355X_MICROARCH: keep <= 4 blocks of 256 threads per CU)
    static size_t occ_lds = (size_t)-1;
    static int occ_blocks = 1, num_cus = 256;
    if (occ_lds != lds) {
        int nb = 0, devid = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, WG, lds) != hipSuccess || nb < 1)
            nb = 1;
        if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess)
            num_cus = prop.multiProcessorCount;
        occ_blocks = nb;
        occ_lds = lds;
    }
    // K = 128 keeps 64 weight registers per lane and is MFMA-bound: 2 workgroups per CU measured
    // best.  Narrow K is store- / gather-latency-bound: the more resident workgroups the better.
    const int cap = KQ >= 8 ? (int)options().gemm_max_wg_per_cu : (KQ >= 4 ? 3 : 6);
    int gx = num_cus * (occ_blocks > cap ? cap : occ_blocks) / gy;
    if (gx < 1)
        gx = 1;
    if (gx > num_stages)
        gx = num_stages; // at least one full stage per workgroup
    hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(WG), lds, s, A, lda, K, W, ldw, bias, skip, Y, M, N, act,
                       rg_log2, P, vec_out, gd);
    return hipGetLastError();
}

bool linear_reg_eligible(const GemmArgs &g)
{
    return options().gemm_variant == 0 && g.nseg == 1 && g.rs[0] == nullptr && g.k[0] <= 128;
}

hipError_t launch_linear_reg(const GemmArgs &g, const float *w, int ldw, const float *bias,
                             const float *skip, float *y, int M, int N, int act, hipStream_t s)
{
    const int K = g.k[0];
    const bool vec = g.avec[0] != 0;
    const int kq = K <= 16 ? 1 : (K <= 32 ? 2 : (K <= 64 ? 4 : 8));
#define GNNB_LR_CASE(Q)                                                                              \
    case Q:                                                                                          \
        return vec ? launch_linear_reg_t<Q, true>(g.a[0], g.lda[0], K, w, ldw, bias, skip, y, M, N, act, s) \
                   : launch_linear_reg_t<Q, false>(g.a[0], g.lda[0], K, w, ldw, bias, skip, y, M, N, act, s);
    switch (kq) {
        GNNB_LR_CASE(1)
        GNNB_LR_CASE(2)
        GNNB_LR_CASE(4)
        GNNB_LR_CASE(8)
    }
#undef GNNB_LR_CASE
    return hipErrorInvalidValue;
}

// Fused narrow-input conv: Y = act(aggregate(x) . W^T + b (+ skip)) in one launch (K <= 32).
hipError_t launch_conv_gather(const BatchTables &t, int agg_kind, float eps, const float *x, int lda,
                              int K, const float *w, int ldw, const float *bias, const float *skip,
                              float *y, int N, int act, hipStream_t s, int cat)
{
    // K = width of the stage row the GEMM contracts over: F_in, or 2 F_in in the [aggregate | own row] form
    if (K > 32 || agg_kind == GNNB_AGG_PNA || t.num_nodes <= 0 || (cat > 0 && K != 2 * cat))
        return hipErrorNotSupported;
    // the ring form (k_first.hip): whole graphs staged once for all output columns
    if (options().first_ring && skip == nullptr && lda == (cat > 0 ? cat : K)) {
        hipError_t he = launch_conv_first(t, agg_kind, eps, x, lda, K, w, ldw, bias, y, N, act, s, cat);
        if (he != hipErrorNotSupported)
            return he;
    }
    GatherDesc gd;
    gd.rec = t.node_rec;
    gd.col = t.col;
    gd.dinv = t.dinv;
    gd.mode = agg_kind;
    gd.eps = eps;
    gd.cat = cat;
    if (K <= 16)
        return launch_linear_reg_t<1, false>(x, lda, K, w, ldw, bias, skip, y, t.num_nodes, N, act, s, gd);
    return launch_linear_reg_t<2, false>(x, lda, K, w, ldw, bias, skip, y, t.num_nodes, N, act, s, gd);
}

} // namespace gnnb
