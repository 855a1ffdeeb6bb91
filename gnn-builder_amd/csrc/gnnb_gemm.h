// gnnb_gemm.h -- what the GEMM translation units of libgnnb_hip.so share (gfx950 only): one kernel family per unit
// (k_linear.hip, k_linear_dma.hip, k_linear_reg.hip, k_linear_wlds.hip) and gemm_launch.hip, host only, which picks the family
// (launch_linear), plans k_linear_dma's grid and keeps the stream-K scratch.  Nothing outside those five units includes this.
#pragma once
#include "gnnb_device.h"

namespace gnnb {

// chunk geometry of the tiled kernels (k_linear, k_linear_dma): K goes by in 32-wide chunks (GemmArgs::cpre counts them)
static constexpr int BM = 128;
static constexpr int BK = 32;
static constexpr int LDS_LD = BK + 4; // padded row, floats

// k_linear_dma's output tile and its workgroups per CU -- what the planner and the stream-K scratch size need of the kernel's
// shape; the other shape constants, and the measurements behind these, are with the kernel (k_linear_dma.hip)
static constexpr int DM = 128, DN = 128, DWGPC = 2;

// Stream-K limits.  Tail-only runs (fewer tiles than resident workgroups) for K >= 1024 (32 chunks): measured at C4's 13F GEMM
// (52 chunks, 1153 tiles) 112.5 against 106 TFLOP/s with row slices, at C5's K = 512 (16 chunks: runs of 7) 105 against 108 --
// short runs are all pipeline prologue and fix-up (SK_MIN_TOTAL, SK_MIN_Q).  With every tile in the space (at least one whole
// round of tiles) a run is tiles * chunks / 512 long, but nearly every tile then pays a fix-up (64 KB parked and read back): at
// K = 256 (8 chunks, 577 tiles) that took the GEMM from 74 to 54 TFLOP/s, at K = 512 it is a wash, at K = 1664 it is +1.5 % on
// a 1.13-round shape: K >= 1024 as well (SK_ALL_MIN_TOTAL).
static constexpr int SK_MIN_Q = 6, SK_MIN_TOTAL = 32, SK_ALL_MIN_TOTAL = 32, SK_MAX_WG = 512, SK_MAX_STREAMS = 16;

// How one k_linear_dma launch hands out its tiles_m x tiles_n output tiles of `total` K chunks each (see the kernel for the
// three forms).  Two 64-KB workgroups are resident per CU and share its matrix pipe, so what has to come out even is the work
// per CU: with resident = DWGPC * cus and rem = tiles % cus -- the last, partial round of tiles; all of them when there are
// fewer tiles than CUs -- the first row that applies is taken:
//
//   | form               | condition                                                            | split_from  | split | q                                         |
//   |--------------------|----------------------------------------------------------------------|-------------|-------|-------------------------------------------|
//   | whole tiles        | rem == 0, or pooled, or tail_split == 0                              | tiles       | 1     | 0                                         |
//   | all-tiles stream-K | SK, tiles >= resident, total >= SK_ALL_MIN_TOTAL, tiles total < 2^30 | 0           | 1     | ceil(tiles total / resident)              |
//   | tail stream-K      | SK, total >= SK_MIN_TOTAL, rem total < 2^30                          | tiles - rem | 1     | max(ceil(rem total / resident), SK_MIN_Q) |
//   | row slices x 4     | 4 rem <= resident, not narrow                                        | tiles - rem | 4     | 0                                         |
//   | row slices x 2     | 2 rem <= resident                                                    | tiles - rem | 2     | 0                                         |
//   | whole tiles        | otherwise (the slices of the last round would not fit one round)     | tiles       | 1     | 0                                         |
//
//   SK = tail_split == 2, resident <= SK_MAX_WG and stream-K allowed.
//   grid = min(resident, max(split_from, ceil((tiles - split_from) total / q)))  under stream-K: one run per workgroup,
//          min(resident, split_from + split (tiles - split_from))                otherwise: one item per workgroup.
//
// all-tiles: at least one whole round of tiles, so EVERY tile goes into the (tile, chunk) space and every resident workgroup
// takes one equal run of it (a partial tile, whole tiles, a partial tile) -- no last round is left; a tile is shared by two
// workgroups at most.  tail: fewer tiles than resident workgroups, or a K too short for the above: equal runs of the last
// round's space, at least SK_MIN_Q chunks long.  pooled (the pooling epilogue): whole tiles only -- its blocks are 32-row
// aligned and every wave joins its barrier.  narrow (N <= 64, 1 x 4 waves of 32 columns): no 32-row slices.  A row-class launch
// plans like a plain one.
// Pure: the launcher reads the option and the CU count, and asks for the scratch only when the plan wants it; a launch that is
// refused the scratch (stream capture, SK_MAX_STREAMS, allocation failure) plans again with allow_stream_k = false.
struct DmaPlan {
    int grid = 0, split = 1, split_from = 0, q = 0;
    bool wants_scratch = false;
};
inline DmaPlan plan_linear_dma(int tiles_m, int tiles_n, int total, int cus, int tail_split, bool pooled, bool narrow,
                               bool allow_stream_k)
{
    const int tiles = tiles_m * tiles_n, resident = DWGPC * cus, rem = tiles % cus;
    DmaPlan p;
    p.split_from = tiles;
    if (rem > 0 && !pooled && tail_split != 0) {
        const bool sk = tail_split == 2 && resident <= SK_MAX_WG && allow_stream_k;
        if (sk && tiles >= resident && total >= SK_ALL_MIN_TOTAL && (long long)tiles * total < (1ll << 30)) {
            p.q = (int)(((long long)tiles * total + resident - 1) / resident);
            p.split_from = 0;
        } else if (sk && total >= SK_MIN_TOTAL && (long long)rem * total < (1ll << 30)) {
            p.q = std::max((rem * total + resident - 1) / resident, SK_MIN_Q);
            p.split_from = tiles - rem;
        } else {
            p.split = (4 * rem <= resident && !narrow) ? 4 : (2 * rem <= resident ? 2 : 1);
            if (p.split > 1)
                p.split_from = tiles - rem;
        }
    }
    p.wants_scratch = p.q > 0;
    p.grid = p.q > 0 ? std::min(std::max(p.split_from, (int)(((long long)(tiles - p.split_from) * total + p.q - 1) / p.q)), resident)
                     : std::min(p.split_from + p.split * (tiles - p.split_from), resident);
    return p;
}

// Diagnostic build only: phase clocks of the persistent small-K kernels (k_linear_reg, k_linear_wlds)
#ifdef GNNB_PROBE
#define GNNB_PT(var, since) do { const unsigned long long _n = clock64(); var += _n - since; since = _n; } while (0)
#else
#define GNNB_PT(var, since) do { } while (0)
#endif

// ---- the families' predicates and launchers (launch_linear, gemm_launch.hip, tries them in this order)
// k_linear_wlds.hip: K, N in {64, 128}, one unscaled 16-B aligned segment, no skip
bool linear_wlds_eligible(const GemmArgs &g, const float *w, int ldw, const float *bias, const float *skip, const float *y, int N);
hipError_t launch_linear_wlds(const GemmArgs &g, const float *w, int ldw, const float *bias, const float *skip, float *y, int M,
                              int N, int act, hipStream_t s);
// k_linear_reg.hip: one unscaled segment of K <= 128
bool linear_reg_eligible(const GemmArgs &g);
hipError_t launch_linear_reg(const GemmArgs &g, const float *w, int ldw, const float *bias, const float *skip, float *y, int M,
                             int N, int act, hipStream_t s);
// k_linear_dma.hip: 16-B aligned rows, segment widths whole chunks (the caller has looked at N).  plan.q > 0: `sk` names the scratch
bool linear_dma_eligible(const GemmArgs &g, const float *w, int ldw);
hipError_t launch_linear_dma(const DmaPlan &plan, StreamK sk, const GemmArgs &g, const float *w, int ldw, const float *bias,
                             const float *skip, float *y, int M, int N, int act, hipStream_t s, const PoolEpilogue *pep,
                             const RowClasses *rcp);
// k_linear.hip: everything else (rcp: one workgroup per class tile)
hipError_t launch_linear_tiles(const GemmArgs &g, const float *w, int ldw, const float *bias, const float *skip, float *y, int M,
                               int N, int act, hipStream_t s, const RowClasses *rcp);

} // namespace gnnb
