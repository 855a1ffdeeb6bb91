// k_schnet.hip -- SchNet's continuous-filter convolution (CFConv): the filter MLP on the matrix cores inside the aggregate (gnnb_schnet.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_schnet_cfconv (no reference in gnnbuilder; models.py, class _SchNetConv; PyG's CFConv):
//   rbf_k = exp(coeff (d - mu_k)^2),  d = edge_dist[eid[slot]],  mu_k = k cutoff / (G - 1),  coeff = -0.5 / mu_1^2      [G]
//   h     = ssp(W1 rbf + b1)                                                                                            [F]
//   w     = (W2 h + b2) C(d),   C(d) = 0.5 (cos(pi d / cutoff) + 1)                                                     [F]
//   out_i = sum_{j -> i} x1_j * w_ij                                                (a row without in-edges: 0)         [N, F]
// on the CSR-by-destination tables of the prepared batch.  2 (Gp F + F^2) flops per edge against one gathered row: the first
// aggregate here whose work is matrix work.  Unfused it is [E, G], [E, F] and [E, F] in HBM and two GEMMs over E rows; here none of
// them leaves the chip.
//
// Work split: TILES OF EDGES, not rows.  A persistent workgroup (4 waves) takes a contiguous range of tiles of TE consecutive CSR slots
// (TE = 64 where the carve below fits, else 32); CSR order keeps a destination's edges contiguous in a tile.  Which row a slot belongs
// to is read from a slot -> row map (k_schnet_slot_rows, once per batch; -1: a gap slot behind a graph's dropped edges).  Per tile:
//   1  basis   slot -> (row, source, distance, C(d), kind) by the first TE lanes; rbf [TE][Gp] -> LDS, Gp = roundup4(G), pad columns 0;
//              accurate cosf / expf, mu_k rounded once from double
//   2  layer 1 H = ssp(rbf W1^T + b1) by v_mfma_f32_16x16x4_f32 (exact fp32 products in every math mode), W1 [F][Gp] staged in LDS
//              once per workgroup.  Operands swapped as k_first_mean does -- A = 16 weight rows, B = 16 slots --, so a lane's
//              accumulator holds four consecutive columns of ONE slot.  A wave owns 16 slots (TE 64) or 16 slots and every second
//              16-column slice (TE 32) and keeps ALL its slices' accumulators in registers: one B read feeds up to 16 MFMAs, 1.06 ..
//              1.25 operand registers from LDS per MFMA.  k step t multiplies column 4 t + (lane >> 4): plain [row][k] tiles, row
//              strides = 2 mod 32 floats (the 32 lanes of a half wave read 32 banks).  H -> LDS [TE][F]
//   3  layer 2 Wf = H W2^T + b2, the same loop over K-panels of 16 columns of W2, [F][16 + 2] floats each.  All panels resident when
//              the carve fits the CU's 160 KiB; else they stream through a ring of two (the next panel's global loads in flight under
//              this panel's MFMAs, one barrier per panel) -- the same code path, the resident case loads the panels once in front of
//              the tile loop.  Epilogue: (acc C[slot]) x1[col[slot]], a 16-byte gather, scalar when width, stride or alignment is off
//              the 16-byte grid (the same bits); the message tile overwrites H behind a barrier
//   4  sum     one column per lane, the tile's slots in order.  A row wholly inside the tile is stored to out; the tile's leading
//              (row starts at or before the tile) and trailing partial rows go to part[tile][0 | 1][width]
// k_schnet_fixup then adds a split row's pieces in tile order and writes the zero rows.  No float atomics.
//
// LDS carve (floats; SchCarve): W1 [F][ldr] | rbf [TE][ldr] | H [TE][ldh] | W2 panels [slots][F][18] | per-slot C, d | b1, b2 | per-slot
// row, col, kind.
//   F 128, G 50, TE 64: 33.0 + 16.5 + 32.5 + 72.0 KiB resident;  F 144, G 50: W2 streamed, TE 64;  F 256, G 64: streamed, TE 32.
//
// Summation order (fixed by the batch and by TE, which (width, G) fix -- never by the grid or by occupancy; the 16-byte and the
// scalar form give the same bits): rbf . W1 and H . W2 are the MFMA's chains over k steps 0, 1, .. from the bias, step t adding
// columns 4 t .. 4 t + 3; message = (Wf C) x1; per (row, column) the messages of one tile in CSR slot order onto 0; a row split
// over tiles: its pieces in tile order onto 0.
#include "gnnb_device.h"

namespace gnnb {

typedef float sch_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SCH_KP = 16;            // columns of W2 per K-panel
constexpr int SCH_PLD = SCH_KP + 2;   // a panel row (floats): = 2 mod 32
constexpr int SCH_LDS_MAX = 160 * 1024;

// row stride (floats) of an LDS tile of w columns: >= w and = 2 mod 32
constexpr int sch_ld(int w) { return ((w + 29) / 32) * 32 + 2; }

struct SchCarve {
    int F, G, TE;
    bool resident;
    constexpr int gp() const { return (G + 3) & ~3; }
    constexpr int fp4() const { return (F + 3) & ~3; }
    constexpr int ldr() const { return sch_ld(gp()); }
    constexpr int ldh() const { return sch_ld(fp4()); }
    constexpr int npan() const { return (fp4() + SCH_KP - 1) / SCH_KP; }
    constexpr int slots() const { return resident ? npan() : 2; }
    constexpr size_t bytes() const { return 4 * ((size_t)F * ldr() + (size_t)TE * ldr() + (size_t)TE * ldh() + (size_t)slots() * F * SCH_PLD + 2 * (size_t)F + 5 * (size_t)TE); }
    constexpr bool fits() const { return bytes() <= (size_t)SCH_LDS_MAX; }
};
// TE 64 with W2 resident, else TE 64 streamed, else TE 32 streamed
constexpr SchCarve sch_carve(int F, int G)
{
    if (SchCarve{F, G, 64, true}.fits())
        return SchCarve{F, G, 64, true};
    if (SchCarve{F, G, 64, false}.fits())
        return SchCarve{F, G, 64, false};
    return SchCarve{F, G, 32, false};
}
static_assert(sch_carve(128, 50).resident && sch_carve(128, 50).TE == 64, "width 128, 50 gaussians: W2 resident");
static_assert(!sch_carve(144, 50).resident && sch_carve(144, 50).TE == 64, "width 144: W2 streamed");
static_assert(sch_carve(256, 64).TE == 32 && sch_carve(256, 64).fits(), "the widest layer fits at TE 32");
static_assert(SCHNET_TE_MIN == 32, "the workspace sizes part[] for tiles of at least 32 slots");

// shifted softplus, softplus(v) - ln 2 = max(v, 0) + log(1 + exp(-|v|)) - ln 2: the hardware's exp2 / log2, absolute error ~ 1e-7
__device__ __forceinline__ float sch_ssp(float v)
{
    return fmaxf(v, 0.0f) + __logf(1.0f + __expf(-fabsf(v))) - 0.69314718055994531f;
}

__global__ __launch_bounds__(WG) void k_schnet_slot_fill(int32_t *__restrict__ slot_row, int E)
{
    const int k = blockIdx.x * WG + threadIdx.x;
    if (k < E)
        slot_row[k] = -1;
}

// slot -> destination row of the prepared batch (behind k_schnet_slot_fill: a slot no row owns stays -1)
__global__ __launch_bounds__(WG) void k_schnet_slot_rows(const int4 *__restrict__ node_rec, int N, int E, int32_t *__restrict__ slot_row)
{
    const int v = blockIdx.x * WG + threadIdx.x;
    if (v >= N)
        return;
    int rp0, deg;
    row_record(node_rec, v, E, rp0, deg);
    for (int k = rp0; k < rp0 + deg; k++)
        slot_row[k] = v;
}

// one K-panel of W2 (columns 16 p ..) -> LDS [F][SCH_PLD], columns past F zero
__device__ __forceinline__ void sch_stage_panel(const float *__restrict__ w2, int ldw2, int F, int p, float *dst)
{
    for (int i = threadIdx.x; i < F * SCH_KP; i += WG) {
        const int n = i >> 4, kk = i & 15, k = SCH_KP * p + kk;
        dst[n * SCH_PLD + kk] = k < F ? w2[(size_t)n * ldw2 + k] : 0.0f;
    }
}

// NSW: the most 16-column slices a wave owns (its accumulators: 4 NSW registers)
template <int TE, int NSW>
__global__ __launch_bounds__(WG) void k_schnet_cfconv(const float *__restrict__ x1, int ldx, int F, const float *__restrict__ dist,
                                                      const float *__restrict__ w1, int ldw1, const float *__restrict__ b1,
                                                      const float *__restrict__ w2, int ldw2, const float *__restrict__ b2, int G,
                                                      double delta, float coeff, float pi_over_c, float *__restrict__ out, int ldo,
                                                      const int32_t *__restrict__ slot_row, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ eid, const int4 *__restrict__ node_rec,
                                                      float *__restrict__ part, int part_w, int N, int E, int T, int resident, int xvec)
{
    extern __shared__ __attribute__((aligned(16))) float sch_lds[];
    constexpr int NSG = TE / 16, WPG = 4 / NSG; // slot groups of a tile; waves that share one (each takes every WPG-th slice)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int sg = wave % NSG, j0 = wave / NSG;
    const SchCarve cv{F, G, TE, resident != 0};
    const int Gp = cv.gp(), Fp4 = cv.fp4(), ldr = cv.ldr(), ldh = cv.ldh(), NP = cv.npan();
    const int NS = (F + 15) >> 4;
    const int nsw = (NS - j0 + WPG - 1) / WPG; // this wave's slices: j0, j0 + WPG, ..
    float *sW1 = sch_lds, *sR = sW1 + F * ldr, *sH = sR + TE * ldr, *sW2 = sH + TE * ldh;
    float *sC = sW2 + (size_t)cv.slots() * F * SCH_PLD, *sD = sC + TE;
    float *sB1 = sD + TE, *sB2 = sB1 + F; // (the biases: read per tile from global memory, 64 predicated loads cost more than the MFMAs)
    int *sRow = reinterpret_cast<int *>(sB2 + F), *sCol = sRow + TE, *sKind = sCol + TE;

    // ---- once per workgroup: W1 (pad columns zero), and every panel of W2 when they are resident
    for (int i = tid; i < F * ldr; i += WG) {
        const int n = i / ldr, g = i - n * ldr;
        sW1[i] = g < G ? w1[(size_t)n * ldw1 + g] : 0.0f;
    }
    for (int i = tid; i < F; i += WG)
        sB1[i] = b1[i], sB2[i] = b2[i];
    if (resident)
        for (int p = 0; p < NP; p++)
            sch_stage_panel(w2, ldw2, F, p, sW2 + (size_t)p * F * SCH_PLD);

    // the wave's operand rows: slot 16 sg + li of the tile, weight row 16 j + li of slice j (clamped: a row past F is computed on
    // row F - 1's weights and never stored)
    const int srow = 16 * sg + li;
    int a1[NSW], a2[NSW];
#pragma unroll
    for (int jj = 0; jj < NSW; jj++) {
        const int n = min(16 * (j0 + jj * WPG) + li, F - 1);
        a1[jj] = n * ldr + lg, a2[jj] = n * SCH_PLD + lg;
    }
    auto bias_acc = [&](const float *b, sch_f32x4 (&acc)[NSW]) {
#pragma unroll
        for (int jj = 0; jj < NSW; jj++) {
            const int c0 = 16 * (j0 + jj * WPG) + 4 * lg;
#pragma unroll
            for (int r = 0; r < 4; r++)
                acc[jj][r] = b[min(c0 + r, F - 1)]; // (a column past F: computed and dropped)
        }
    };

    const int tb = (int)((long long)T * blockIdx.x / gridDim.x), te = (int)((long long)T * (blockIdx.x + 1) / gridDim.x);
    for (int t = tb; t < te; t++) {
        const int t0 = t * TE;
        __syncthreads(); // the tile before is summed: the message tile and the per-slot arrays are free (first tile: W1 / W2 staged)
        // ---- 1: the tile's slots
        if (tid < TE) {
            const int k = t0 + tid;
            int r = -1, j = 0, kind = 0;
            float d = 0.0f, C = 0.0f;
            if (k < E) {
                r = slot_row[k];
                if (r >= N)
                    r = -1;
            }
            if (r >= 0) {
                j = min(max(col[k], 0), N - 1);
                d = dist[min(max(eid[k], 0), E - 1)];
                int rp0, deg;
                row_record(node_rec, r, E, rp0, deg);
                kind = (rp0 >= t0 && rp0 + deg - t0 <= TE) ? 0 : (rp0 <= t0 ? 1 : 2); // whole | leading | trailing
                C = 0.5f * (cosf(d * pi_over_c) + 1.0f);
            }
            sRow[tid] = r, sCol[tid] = j, sKind[tid] = kind, sC[tid] = C, sD[tid] = d;
        }
        __syncthreads();
        for (int i = tid; i < TE * Gp; i += WG) {
            const int s = i / Gp, g = i - s * Gp;
            float v = 0.0f;
            if (g < G && sRow[s] >= 0) {
                const float dd = sD[s] - (float)((double)g * delta);
                v = expf(coeff * (dd * dd));
            }
            sR[s * ldr + g] = v;
        }
        __syncthreads();
        // ---- 2: H = ssp(rbf W1^T + b1)
        sch_f32x4 acc[NSW];
        bias_acc(sB1, acc);
        {
            const float *bp = sR + srow * ldr + lg;
            // (straight-line: a slice past the wave's own is computed on clamped rows and dropped -- a branch round every MFMA keeps the
            // LDS reads from being scheduled ahead of the MFMAs they feed)
#pragma unroll 2
            for (int st = 0; st < (Gp >> 2); st++) {
                const float bv = bp[4 * st];
                float av[NSW];
#pragma unroll
                for (int jj = 0; jj < NSW; jj++)
                    av[jj] = sW1[a1[jj] + 4 * st];
#pragma unroll
                for (int jj = 0; jj < NSW; jj++)
                    acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[jj], bv, acc[jj], 0, 0, 0);
            }
        }
#pragma unroll
        for (int jj = 0; jj < NSW; jj++)
            if (jj < nsw) {
                const int c0 = 16 * (j0 + jj * WPG) + 4 * lg;
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (c0 + r < Fp4) // (the pad columns of H are layer 2's k steps: zero)
                        sH[srow * ldh + c0 + r] = c0 + r < F ? sch_ssp(acc[jj][r]) : 0.0f;
            }
        if (!resident)
            sch_stage_panel(w2, ldw2, F, 0, sW2);
        __syncthreads();
        // ---- 3: Wf = H W2^T + b2, panel by panel
        bias_acc(sB2, acc);
        {
            const float *hp = sH + srow * ldh + lg;
            for (int p = 0; p < NP; p++) {
                float pf[SCH_KP];
                const bool more = !resident && p + 1 < NP;
                if (more) { // the next panel's loads, in flight under this panel's MFMAs
#pragma unroll
                    for (int q = 0; q < SCH_KP; q++) {
                        const int i = tid + q * WG, n = i >> 4, k = SCH_KP * (p + 1) + (i & 15);
                        pf[q] = (i < F * SCH_KP && k < F) ? w2[(size_t)n * ldw2 + k] : 0.0f;
                    }
                }
                const float *wp = sW2 + (size_t)(resident ? p : (p & 1)) * F * SCH_PLD;
                const int kst = min(4, (Fp4 - SCH_KP * p) >> 2);
#pragma unroll 2
                for (int tt = 0; tt < kst; tt++) {
                    const float bv = hp[SCH_KP * p + 4 * tt];
                    float av[NSW];
#pragma unroll
                    for (int jj = 0; jj < NSW; jj++)
                        av[jj] = wp[a2[jj] + 4 * tt];
#pragma unroll
                    for (int jj = 0; jj < NSW; jj++)
                        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[jj], bv, acc[jj], 0, 0, 0);
                }
                if (more) {
                    float *dst = sW2 + (size_t)((p + 1) & 1) * F * SCH_PLD; // (read last by panel p - 1, behind that panel's barrier)
#pragma unroll
                    for (int q = 0; q < SCH_KP; q++) {
                        const int i = tid + q * WG;
                        if (i < F * SCH_KP)
                            dst[(i >> 4) * SCH_PLD + (i & 15)] = pf[q];
                    }
                }
                if (!resident)
                    __syncthreads();
            }
        }
        __syncthreads(); // every wave has read H: the messages take its place
        {
            const float Cs = sC[srow];
            const float *xr = x1 + (size_t)sCol[srow] * ldx;
#pragma unroll
            for (int jj = 0; jj < NSW; jj++)
                if (jj < nsw) {
                    const int c0 = 16 * (j0 + jj * WPG) + 4 * lg;
                    float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (xvec) {
                        if (c0 < F)
                            row_load_vec<4>(xr + c0, xv);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (c0 + r < F)
                                xv[r] = xr[c0 + r];
                    }
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (c0 + r < F)
                            sH[srow * ldh + c0 + r] = (acc[jj][r] * Cs) * xv[r];
                }
        }
        __syncthreads();
        // ---- 4: the segmented sum, one column per lane
        if (tid < F) {
            int cur = -1, kind = 0;
            float a = 0.0f;
            auto flush = [&]() {
                if (cur < 0)
                    return;
                if (kind == 0)
                    out[(size_t)cur * ldo + tid] = a;
                else
                    part[((size_t)t * 2 + (kind - 1)) * part_w + tid] = a;
            };
            for (int s = 0; s < TE; s++) {
                const int r = sRow[s];
                if (r < 0)
                    continue;
                if (r != cur) {
                    flush();
                    cur = r, kind = sKind[s], a = 0.0f;
                }
                a += sH[s * ldh + tid];
            }
            flush();
        }
    }
}

// rows split over tiles: their pieces in tile order; rows without in-edges: zero.  A thread owns four columns of a row
__global__ __launch_bounds__(WG) void k_schnet_fixup(const int4 *__restrict__ node_rec, const float *__restrict__ part, int part_w,
                                                     float *__restrict__ out, int ldo, int F, int N, int E, int TE, int T)
{
    const int chunks = (F + 3) >> 2;
    const long long idx = (long long)blockIdx.x * WG + threadIdx.x;
    if (idx >= (long long)N * chunks)
        return;
    const int v = (int)(idx / chunks), c0 = (int)(idx - (long long)v * chunks) * 4;
    int rp0, deg;
    row_record(node_rec, v, E, rp0, deg);
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (deg > 0) {
        const int ta = rp0 / TE, tz = min((rp0 + deg - 1) / TE, T - 1);
        if (ta >= tz)
            return; // (wholly inside one tile: k_schnet_cfconv stored it)
        for (int t = ta; t <= tz; t++) {
            const float *p = part + ((size_t)t * 2 + (rp0 <= t * TE ? 0 : 1)) * part_w + c0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (c0 + q < F)
                    a[q] += p[q];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (c0 + q < F)
            out[(size_t)v * ldo + c0 + q] = a[q];
}

__global__ __launch_bounds__(WG) void k_schnet_ssp(float *__restrict__ y, size_t n)
{
    const size_t i = (size_t)blockIdx.x * WG + threadIdx.x;
    if (i < n)
        y[i] = sch_ssp(y[i]);
}

size_t schnet_scratch_bytes(int max_edges, int width)
{
    const size_t E = (size_t)std::max(max_edges, 1), tiles = (E + SCHNET_TE_MIN - 1) / SCHNET_TE_MIN;
    return ((E * 4 + 15) & ~(size_t)15) + tiles * 2 * (size_t)width * 4;
}

SchnetScratch schnet_scratch_at(char *base, int max_edges, int width)
{
    const size_t E = (size_t)std::max(max_edges, 1);
    return {reinterpret_cast<int32_t *>(base), reinterpret_cast<float *>(base + ((E * 4 + 15) & ~(size_t)15)), width, max_edges};
}

hipError_t launch_schnet_slots(const BatchTables &t, const SchnetScratch &sc, hipStream_t s)
{
    if (t.num_edges > sc.max_edges || !sc.slot_row)
        return hipErrorInvalidValue;
    if (t.num_nodes <= 0 || t.num_edges <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_schnet_slot_fill, dim3((t.num_edges + WG - 1) / WG), dim3(WG), 0, s, sc.slot_row, t.num_edges);
    hipLaunchKernelGGL(k_schnet_slot_rows, dim3((t.num_nodes + WG - 1) / WG), dim3(WG), 0, s, t.node_rec, t.num_nodes, t.num_edges, sc.slot_row);
    return hipGetLastError();
}

hipError_t launch_schnet_ssp(float *y, size_t n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_schnet_ssp, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, s, y, n);
    return hipGetLastError();
}

hipError_t launch_schnet_cfconv(const BatchTables &t, const SchnetScratch &sc, const float *x1, int ldx, int width, const float *edge_dist,
                                const float *w1, int ldw1, const float *b1, const float *w2, int ldw2, const float *b2, int gaussians,
                                float cutoff, float *out, int ldo, hipStream_t s)
{
    const int F = width, G = gaussians, N = t.num_nodes, E = t.num_edges;
    if (F < 1 || F > SCHNET_MAX_WIDTH || G < 1 || G > SCHNET_MAX_GAUSSIANS || !(cutoff > 0.0f) || !std::isfinite(cutoff) || ldx < F || ldo < F ||
        ldw1 < G || ldw2 < F || E > sc.max_edges || F > sc.part_w)
        return hipErrorInvalidValue;
    if (N <= 0)
        return hipSuccess;
    const SchCarve cv = sch_carve(F, G);
    if (!cv.fits())
        return hipErrorInvalidValue;
    const int TE = cv.TE, T = E > 0 ? (E + TE - 1) / TE : 0;
    if (T > 0) {
        // mu_k = k delta rounded once (torch.linspace rounds the same product); G = 1: the one centre is 0 and the width is the cutoff
        const double delta = G > 1 ? (double)cutoff / (G - 1) : (double)cutoff;
        const float mu1 = (float)delta;
        const float coeff = (float)(-0.5 / ((double)mu1 * (double)mu1));
        const float pi_over_c = (float)(3.14159265358979323846 / (double)cutoff);
        const int xvec = (F % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)x1 & 15) == 0);
        const int NS = (F + 15) / 16, nsw = TE == 64 ? NS : (NS + 1) / 2;
        hipError_t rc = hipSuccess;
        auto go = [&](auto tetag, auto nstag) {
            auto kern = k_schnet_cfconv<decltype(tetag)::value, decltype(nstag)::value>;
            if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), cv.bytes())) != hipSuccess)
                return;
            const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, cv.bytes(), 2);
            const int grid = std::min(T, std::max(occ.blocks * occ.cus, 1));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), cv.bytes(), s, x1, ldx, F, edge_dist, w1, ldw1, b1, w2, ldw2, b2, G, delta, coeff,
                               pi_over_c, out, ldo, sc.slot_row, t.col, t.eid, t.node_rec, sc.part, sc.part_w, N, E, T, cv.resident ? 1 : 0, xvec);
        };
        if (TE == 64) {
            if (nsw <= 2)
                go(IntTag<64>{}, IntTag<2>{});
            else if (nsw <= 4)
                go(IntTag<64>{}, IntTag<4>{});
            else if (nsw <= 8)
                go(IntTag<64>{}, IntTag<8>{});
            else if (nsw <= 12)
                go(IntTag<64>{}, IntTag<12>{});
            else
                go(IntTag<64>{}, IntTag<16>{});
        } else {
            if (nsw <= 4)
                go(IntTag<32>{}, IntTag<4>{});
            else
                go(IntTag<32>{}, IntTag<8>{});
        }
        if (rc != hipSuccess)
            return rc;
    }
    const long long threads = (long long)N * ((F + 3) / 4);
    hipLaunchKernelGGL(k_schnet_fixup, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), 0, s, t.node_rec, sc.part, sc.part_w, out, ldo, F, N, E,
                       TE, T);
    return hipGetLastError();
}

} // namespace gnnb
