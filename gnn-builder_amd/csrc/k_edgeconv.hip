// k_edgeconv.hip -- EdgeConv (DGCNN): the edge MLP's second linear on the matrix cores under a segmented max (gnnb_edgeconv.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
//
// k_edgeconv_max (no reference in gnnbuilder; models.py, class EdgeConv_GNNB; PyG's EdgeConv(nn, aggr="max")):
//   hid_ij = relu(a_i + b_j)            [a | b] = x [(W1a - W1b) ; W1b]^T + [b1 ; 0]: the layer's one node GEMM (edgeconv_fold)    [H]
//   m_ij   = W2 hid_ij                                                                                                          [F]
//   out_i  = act(max_{j -> i} m_ij + b2 + skip_i)       (a row without in-edges: act(skip_i); b2 commutes with the max)          [N, F]
// on the CSR-by-destination tables of the prepared batch.  max does not commute with W2, so the product stays per edge: 2 H F flops
// per edge against two gathered rows.  Unfused it is [E, H] and [E, F] in HBM and a GEMM over E rows; here neither leaves the chip.
//
// Work split: tiles of TE consecutive CSR slots taken by persistent workgroups of 4 waves, as k_schnet_cfconv, on its
// slot -> row map (k_schnet_slot_rows; -1: a gap slot) and its per-tile part[] buffer.  Per tile, four barriers:
//   1  slots   slot -> (row, source, kind: whole | leading | trailing) by the first TE lanes
//   2  hidden  Hid [TE][ldh] straight into LDS.  A half wave owns TE / 8 CONSECUTIVE slots and 32 chunks of four columns: the b row
//              is a 16-byte gather per slot, the a row stays in registers over a run of slots that share the destination and is
//              loaded again only where the row changes.  Gap slots and the pad columns up to the last K-panel are 0.  Scalar loads
//              when H, the stride or the address is off the 16-byte grid: the same bits (one add, one max)
//   3  product M = Hid W2^T by v_mfma_f32_16x16x4_f32 (exact fp32 products in every math mode), operands swapped -- A = 16 weight
//              rows, B = 16 slots --, so a lane's accumulator holds four consecutive columns of ONE slot.  W2 in K-panels of 16
//              columns, [F][16 + 4] floats: resident when the carve fits the CU's 160 KiB, else streamed through a ring of two (the
//              next panel's global loads in flight under this panel's MFMAs, one barrier per panel) on the same code path.  Within a
//              panel, k step t of lane group g multiplies column 4 g + t: ONE 16-byte LDS read per operand feeds four MFMAs.  The
//              messages go to a tile of their OWN (no barrier between the last MFMA read of Hid and the first message store)
//   4  max     one column per lane from -inf (messages are routinely all negative), the tile's slots in order.  A row wholly inside
//              the tile is stored: act(max + b2 + skip); the tile's leading and trailing partial rows go to part[tile][0 | 1][width]
// k_edgeconv_fixup then takes the max of a split row's pieces (+ b2), writes act(skip) for the rows without in-edges (0 and NO bias).
// No float atomics.
//
// LDS carve (floats; EcCarve): Hid [TE][ldh] | M [TE][ldm] | W2 panels [slots][F][20] | row, col, kind [3 TE]; ldh, ldm = 4 mod 32.
//   H = F = 128: 33.0 + 33.0 + 80.0 KiB, TE 64, resident;  144: streamed, TE 64;  256: streamed, TE 32.
//
// Order: m_ij is the MFMA's chain from 0 over the panels in order, within panel p step t adding columns 16 p + t + {0, 4, 8, 12};
// the max is order-free, so the result does not depend on TE, the grid, the tile split, resident or streamed: the same bits.
#include "gnnb_device.h"

namespace gnnb {

typedef float ec_f32x4 __attribute__((ext_vector_type(4)));

constexpr int EC_KP = 16;          // columns of W2 per K-panel
constexpr int EC_PLD = EC_KP + 4;  // a panel row (floats): 16-byte aligned, = 20 mod 32
constexpr int EC_LDS_MAX = 160 * 1024;

// row stride (floats) of an LDS tile of w columns: >= w, a multiple of 4 (16-byte reads) and = 4 mod 32
constexpr int ec_ld(int w) { return ((w + 31) / 32) * 32 + 4; }

struct EcCarve {
    int H, F, TE;
    bool resident;
    constexpr int npan() const { return (H + EC_KP - 1) / EC_KP; }
    constexpr int ldh() const { return ec_ld(npan() * EC_KP); }
    constexpr int ldm() const { return ec_ld(F); }
    constexpr int slots() const { return resident ? npan() : 2; }
    constexpr size_t bytes() const { return 4 * ((size_t)TE * ldh() + (size_t)TE * ldm() + (size_t)slots() * F * EC_PLD + 3 * (size_t)TE); }
    constexpr bool fits() const { return bytes() <= (size_t)EC_LDS_MAX; }
};
// TE 64 with W2 resident, else TE 64 streamed, else TE 32 streamed
constexpr EcCarve ec_carve(int H, int F)
{
    if (EcCarve{H, F, 64, true}.fits())
        return EcCarve{H, F, 64, true};
    if (EcCarve{H, F, 64, false}.fits())
        return EcCarve{H, F, 64, false};
    return EcCarve{H, F, 32, false};
}
static_assert(ec_carve(128, 128).resident && ec_carve(128, 128).TE == 64, "width 128: W2 resident");
static_assert(!ec_carve(144, 144).resident && ec_carve(144, 144).TE == 64, "width 144: W2 streamed, 64 slots");
static_assert(!ec_carve(256, 256).resident && ec_carve(256, 256).TE == 32 && ec_carve(256, 256).fits(), "the widest layer fits at TE 32");
static_assert(SCHNET_TE_MIN == 32, "the workspace sizes part[] for tiles of at least 32 slots");

// one K-panel of W2 (columns 16 p ..) -> LDS [F][EC_PLD], columns past H zero
__device__ __forceinline__ void ec_stage_panel(const float *__restrict__ w2, int ldw2, int F, int H, int p, float *dst)
{
    for (int i = threadIdx.x; i < F * EC_KP; i += WG) {
        const int n = i >> 4, kk = i & 15, k = EC_KP * p + kk;
        dst[n * EC_PLD + kk] = k < H ? w2[(size_t)n * ldw2 + k] : 0.0f;
    }
}

// act(v + skip): what every stored element goes through (the kernel's whole rows and the fix-up's)
__device__ __forceinline__ float ec_finish(float v, const float *__restrict__ skip, size_t at, int act)
{
    if (skip)
        v += skip[at];
    return act_apply(v, act);
}

// NSW: the most 16-column slices a wave owns (its accumulators: 4 NSW registers)
template <int TE, int NSW>
__global__ __launch_bounds__(WG) void k_edgeconv_max(const float *__restrict__ ab, int ldab, int H, const float *__restrict__ w2, int ldw2,
                                                     const float *__restrict__ b2, int F, const float *__restrict__ skip, int lds, int act,
                                                     float *__restrict__ out, int ldo, const int32_t *__restrict__ slot_row,
                                                     const int32_t *__restrict__ col, const int4 *__restrict__ node_rec, float *__restrict__ part,
                                                     int part_w, int N, int E, int T, int resident, int vec)
{
    extern __shared__ __attribute__((aligned(16))) float ec_lds[];
    constexpr int NSG = TE / 16, WPG = 4 / NSG; // slot groups of a tile; waves that share one (each takes every WPG-th slice)
    constexpr int SPH = TE / 8;                 // consecutive slots of a half wave in phase 2
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int sg = wave % NSG, j0 = wave / NSG;
    const EcCarve cv{H, F, TE, resident != 0};
    const int ldh = cv.ldh(), ldm = cv.ldm(), NP = cv.npan();
    const int NS = (F + 15) >> 4;
    const int nsw = (NS - j0 + WPG - 1) / WPG; // this wave's slices: j0, j0 + WPG, ..
    float *sHid = ec_lds, *sMsg = sHid + TE * ldh, *sW2 = sMsg + TE * ldm;
    int *sRow = reinterpret_cast<int *>(sW2 + (size_t)cv.slots() * F * EC_PLD), *sCol = sRow + TE, *sKind = sCol + TE;

    if (resident) // once per workgroup: every panel of W2
        for (int p = 0; p < NP; p++)
            ec_stage_panel(w2, ldw2, F, H, p, sW2 + (size_t)p * F * EC_PLD);
    const float bias = (b2 && tid < F) ? b2[tid] : 0.0f; // (phase 4: a lane owns column tid)

    // the wave's operand rows: slot 16 sg + li of the tile, weight row 16 j + li of slice j (clamped: a row past F is computed on
    // row F - 1's weights and never stored); lane group lg reads columns 4 lg .. 4 lg + 3 of a panel
    const int srow = 16 * sg + li;
    int a2[NSW];
#pragma unroll
    for (int jj = 0; jj < NSW; jj++)
        a2[jj] = min(16 * (j0 + jj * WPG) + li, F - 1) * EC_PLD + 4 * lg;
    const int hw = tid >> 5, hl = tid & 31, nch = (NP * EC_KP) >> 2; // phase 2: the half wave, its lane, 4-column chunks of a Hid row

    const int tb = (int)((long long)T * blockIdx.x / gridDim.x), te = (int)((long long)T * (blockIdx.x + 1) / gridDim.x);
    for (int t = tb; t < te; t++) {
        const int t0 = t * TE;
        __syncthreads(); // the tile before is reduced: the message tile and the per-slot arrays are free (first tile: W2 staged)
        // ---- 1: the tile's slots
        if (tid < TE) {
            const int k = t0 + tid;
            int r = -1, j = 0, kind = 0;
            if (k < E) {
                r = slot_row[k];
                if (r >= N)
                    r = -1;
            }
            if (r >= 0) {
                j = min(max(col[k], 0), N - 1);
                int rp0, deg;
                row_record(node_rec, r, E, rp0, deg);
                kind = (rp0 >= t0 && rp0 + deg - t0 <= TE) ? 0 : (rp0 <= t0 ? 1 : 2); // whole | leading | trailing
            }
            sRow[tid] = r, sCol[tid] = j, sKind[tid] = kind;
        }
        __syncthreads();
        // ---- 2: Hid = relu(a[row] + b[col]); the a chunk lives over a run of slots of one row
        for (int c = hl; c < nch; c += 32) {
            const int k0 = 4 * c;
            int cur = -1;
            float av[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
            for (int q = 0; q < SPH; q++) {
                const int s = hw * SPH + q, r = sRow[s];
                ec_f32x4 h = {0.0f, 0.0f, 0.0f, 0.0f};
                if (r >= 0 && k0 < H) {
                    const float *bp = ab + (size_t)sCol[s] * ldab + H + k0;
                    float bv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (vec) {
                        if (r != cur)
                            row_load_vec<4>(ab + (size_t)r * ldab + k0, av);
                        row_load_vec<4>(bp, bv);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (k0 + e < H) {
                                if (r != cur)
                                    av[e] = ab[(size_t)r * ldab + k0 + e];
                                bv[e] = bp[e];
                            }
                    }
                    cur = r;
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        h[e] = k0 + e < H ? fmaxf(av[e] + bv[e], 0.0f) : 0.0f;
                }
                *reinterpret_cast<ec_f32x4 *>(sHid + s * ldh + k0) = h;
            }
        }
        if (!resident)
            ec_stage_panel(w2, ldw2, F, H, 0, sW2);
        __syncthreads();
        // ---- 3: M = Hid W2^T, panel by panel
        ec_f32x4 acc[NSW];
#pragma unroll
        for (int jj = 0; jj < NSW; jj++)
            acc[jj] = ec_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        {
            const float *hp = sHid + srow * ldh + 4 * lg;
            for (int p = 0; p < NP; p++) {
                float pf[EC_KP];
                const bool more = !resident && p + 1 < NP;
                if (more) { // the next panel's loads, in flight under this panel's MFMAs
#pragma unroll
                    for (int q = 0; q < EC_KP; q++) {
                        const int i = tid + q * WG, n = i >> 4, k = EC_KP * (p + 1) + (i & 15);
                        pf[q] = (i < F * EC_KP && k < H) ? w2[(size_t)n * ldw2 + k] : 0.0f;
                    }
                }
                const float *wp = sW2 + (size_t)(resident ? p : (p & 1)) * F * EC_PLD;
                // (straight-line over the compile-time slice count: a slice past the wave's own is computed on clamped rows and dropped)
                const ec_f32x4 bv = *reinterpret_cast<const ec_f32x4 *>(hp + EC_KP * p);
                ec_f32x4 av[NSW];
#pragma unroll
                for (int jj = 0; jj < NSW; jj++)
                    av[jj] = *reinterpret_cast<const ec_f32x4 *>(wp + a2[jj]);
#pragma unroll
                for (int tt = 0; tt < 4; tt++)
#pragma unroll
                    for (int jj = 0; jj < NSW; jj++)
                        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[jj][tt], bv[tt], acc[jj], 0, 0, 0);
                if (more) {
                    float *dst = sW2 + (size_t)((p + 1) & 1) * F * EC_PLD; // (read last by panel p - 1, behind that panel's barrier)
#pragma unroll
                    for (int q = 0; q < EC_KP; q++) {
                        const int i = tid + q * WG;
                        if (i < F * EC_KP)
                            dst[(i >> 4) * EC_PLD + (i & 15)] = pf[q];
                    }
                }
                if (!resident)
                    __syncthreads();
            }
        }
#pragma unroll
        for (int jj = 0; jj < NSW; jj++)
            if (jj < nsw) {
                const int c0 = 16 * (j0 + jj * WPG) + 4 * lg;
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (c0 + r < F)
                        sMsg[srow * ldm + c0 + r] = acc[jj][r];
            }
        __syncthreads();
        // ---- 4: the segmented max, one column per lane
        if (tid < F) {
            int cur = -1, kind = 0;
            float a = -INFINITY;
            auto flush = [&]() {
                if (cur < 0)
                    return;
                if (kind == 0)
                    out[(size_t)cur * ldo + tid] = ec_finish(a + bias, skip, (size_t)cur * lds + tid, act);
                else
                    part[((size_t)t * 2 + (kind - 1)) * part_w + tid] = a;
            };
            for (int s = 0; s < TE; s++) {
                const int r = sRow[s];
                if (r < 0)
                    continue;
                if (r != cur) {
                    flush();
                    cur = r, kind = sKind[s], a = -INFINITY;
                }
                a = fmaxf(a, sMsg[s * ldm + tid]);
            }
            flush();
        }
    }
}

// rows split over tiles: the max of their pieces, + b2; rows without in-edges: 0 and no bias; both through skip and the activation.
// A thread owns four columns of a row
__global__ __launch_bounds__(WG) void k_edgeconv_fixup(const int4 *__restrict__ node_rec, const float *__restrict__ part, int part_w,
                                                       const float *__restrict__ b2, const float *__restrict__ skip, int lds, int act,
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
            return; // (wholly inside one tile: k_edgeconv_max stored it)
#pragma unroll
        for (int q = 0; q < 4; q++)
            a[q] = -INFINITY;
        for (int t = ta; t <= tz; t++) {
            const float *p = part + ((size_t)t * 2 + (rp0 <= t * TE ? 0 : 1)) * part_w + c0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (c0 + q < F)
                    a[q] = fmaxf(a[q], p[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (b2 && c0 + q < F)
                a[q] += b2[c0 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (c0 + q < F)
            out[(size_t)v * ldo + c0 + q] = ec_finish(a[q], skip, (size_t)v * lds + c0 + q, act);
}

hipError_t launch_edgeconv_max(const BatchTables &t, const SchnetScratch &sc, const float *ab, int ldab, int hidden, const float *w2, int ldw2,
                               const float *b2, int width, const float *skip, int lds, int act, float *out, int ldo, hipStream_t s)
{
    const int H = hidden, F = width, N = t.num_nodes, E = t.num_edges;
    if (H < 1 || H > EDGECONV_MAX_WIDTH || F < 1 || F > EDGECONV_MAX_WIDTH || ldab < 2 * H || ldw2 < H || ldo < F || (skip && lds < F) ||
        E > sc.max_edges || F > sc.part_w || !sc.slot_row)
        return hipErrorInvalidValue;
    if (N <= 0)
        return hipSuccess;
    const EcCarve cv = ec_carve(H, F);
    if (!cv.fits())
        return hipErrorInvalidValue;
    const int TE = cv.TE, T = E > 0 ? (E + TE - 1) / TE : 0;
    if (T > 0) {
        const int vec = (H % 4 == 0) && (ldab % 4 == 0) && (((uintptr_t)ab & 15) == 0);
        const int NS = (F + 15) / 16, nsw = TE == 64 ? NS : (NS + 1) / 2;
        hipError_t rc = hipSuccess;
        auto go = [&](auto tetag, auto nstag) {
            auto kern = k_edgeconv_max<decltype(tetag)::value, decltype(nstag)::value>;
            if ((rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), cv.bytes())) != hipSuccess)
                return;
            const Occupancy occ = kernel_occupancy(reinterpret_cast<const void *>(kern), WG, cv.bytes(), 2);
            const int grid = std::min(T, std::max(occ.blocks * occ.cus, 1));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), cv.bytes(), s, ab, ldab, H, w2, ldw2, b2, F, skip, lds, act, out, ldo, sc.slot_row, t.col,
                               t.node_rec, sc.part, sc.part_w, N, E, T, cv.resident ? 1 : 0, vec);
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
    hipLaunchKernelGGL(k_edgeconv_fixup, dim3((unsigned)((threads + WG - 1) / WG)), dim3(WG), 0, s, t.node_rec, sc.part, sc.part_w, b2, skip, lds, act,
                       out, ldo, F, N, E, TE, T);
    return hipGetLastError();
}

} // namespace gnnb
