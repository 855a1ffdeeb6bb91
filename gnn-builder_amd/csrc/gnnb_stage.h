// gnnb_stage.h -- what the staged producer kernels share (k_first.hip: k_conv_first; k_first_mean.hip: k_sage_first_mean;
// k_pna_first.hip: k_pna_first; k_pna.hip: k_pna_pagg) and the carve and launch plan of k_aggregate_ring (k_aggregate.hip), each
// stated ONCE, in the manner of gnnb_stack_plan.h: a kernel takes its region offsets from its carve, its launcher the dynamic-LDS
// size from the same carve's total(), and what a launcher decides is a pure function of plain integers.
// Host side: no HIP call and no options() in here (the launchers read the options, the device and the pointers and pass them in);
// everything a kernel uses is constexpr, which the HIP compiler takes as host and device code alike.
// Device side: the skeleton of a staged kernel -- stage struct, tile-table window, stage planner -- as __forceinline__ functions
// with the capacity as a template constant.  (The DMA issue loops and the register-resident weight loader stay in the units:
// as shared inline functions they changed the kernels' machine code.)
#pragma once
#include <stddef.h>

#include "gnnb_device.h"
#include "gnnb_stack_plan.h"

namespace gnnb {

// =====================================================================================
// host side: capacities, carves, grid, promise, plans
// =====================================================================================
// rows / CSR entries of a stage, per kernel (all four: 8 waves, two workgroups per CU)
constexpr int STAGE_NW = 8, STAGE_WG = STAGE_NW * 64;
constexpr int F1_CAP = 128, F1_ECAP = 8 * F1_CAP; // k_conv_first
constexpr int FM_CAP = 56, FM_ECAP = 448;         // k_sage_first_mean
constexpr int PF_CAP = 64, PF_ECAP = 512;         // k_pna_first
constexpr int PA_CAP = 64, PA_ECAP = 512;         // k_pna_pagg
// tiles per workgroup: as ZF_TCAP, the run's tile table lives in one register per lane (+ its end)
constexpr int STAGE_TCAP = ZF_TCAP;
static_assert(F1_ECAP == 1024 && STAGE_TCAP == 62 && STAGE_TCAP + 1 < 64, "a run and its end fit the 64 lanes of the window");

constexpr int stage_xs_b(int cap, int f) { return ((cap * f * 4) + 15) & ~15; } // `cap` unpadded x rows of f floats, 16-B aligned

// LDS carves (bytes, every region 16-B aligned).  All four: TWO input buffers of in_b() bytes first, then the kernel's own tiles.
//   k_conv_first   input buffer {x rows | records | dinv | CSR slice}; A0 [cap][16 KQ + 4]; a 16 x 36 output-transpose scratch per wave
struct F1Carve {
    int f, kq; // input width, 16-wide k blocks of the product
    constexpr int xs_b() const { return stage_xs_b(F1_CAP, f); }
    constexpr int rec_o() const { return xs_b(); }
    constexpr int dinv_o() const { return rec_o() + F1_CAP * STACK_NODE_REC_B; }
    constexpr int col_o() const { return dinv_o() + F1_CAP * 4; }
    constexpr int in_b() const { return col_o() + F1_ECAP * 4; }
    constexpr size_t a0_off() const { return 2 * (size_t)in_b(); }
    constexpr size_t total() const { return a0_off() + (size_t)F1_CAP * (16 * kq + 4) * 4 + (size_t)STAGE_NW * 16 * 36 * 4; }
};
//   k_sage_first_mean   input buffer {x rows | records | CSR slice}; A0 [cap][16 KQ + 4]; the output tile YT [cap][Nout + 4]
struct FmCarve {
    int f, kq, nout;
    constexpr int xs_b() const { return stage_xs_b(FM_CAP, f); }
    constexpr int rec_o() const { return xs_b(); }
    constexpr int col_o() const { return rec_o() + FM_CAP * STACK_NODE_REC_B; }
    constexpr int in_b() const { return col_o() + FM_ECAP * 4; }
    constexpr size_t a0_off() const { return 2 * (size_t)in_b(); }
    constexpr size_t total() const { return a0_off() + (size_t)FM_CAP * (16 * kq + 4) * 4 + (size_t)FM_CAP * (nout + 4) * 4; }
};
//   k_pna_first   input buffer {x rows | records | CSR slice | amp | att}; SW = W_pre [F][2F] + b_pre [F]; PQ [cap][2F + 1];
//                 A0 [cap][16 KQ + 4] (the output tile is written over it)
struct PfCarve {
    int f, kq;
    constexpr int xs_b() const { return stage_xs_b(PF_CAP, f); }
    constexpr int rec_o() const { return xs_b(); }
    constexpr int col_o() const { return rec_o() + PF_CAP * STACK_NODE_REC_B; }
    constexpr int amp_o() const { return col_o() + PF_ECAP * 4; }
    constexpr int att_o() const { return amp_o() + PF_CAP * 4; }
    constexpr int in_b() const { return att_o() + PF_CAP * 4; }
    constexpr size_t sw_off() const { return 2 * (size_t)in_b(); }
    constexpr int sw_f() const { return (f * (2 * f) + f + 3) & ~3; }         // floats
    constexpr int pq_f() const { return (PF_CAP * (2 * f + 1) + 3) & ~3; }    // floats
    constexpr size_t total() const { return sw_off() + (size_t)sw_f() * 4 + (size_t)pq_f() * 4 + (size_t)PF_CAP * (16 * kq + 4) * 4; }
};
//   k_pna_pagg   two buffers {x rows, padded to F + 4 floats -> P | records | CSR slice}, nothing else
struct PaCarve {
    int f;
    constexpr int xs_b() const { return PA_CAP * (f + 4) * 4; }
    constexpr int rec_o() const { return xs_b(); }
    constexpr int col_o() const { return rec_o() + PA_CAP * STACK_NODE_REC_B; }
    constexpr int in_b() const { return col_o() + PA_ECAP * 4; }
    constexpr size_t total() const { return 2 * (size_t)in_b(); }
};
//   k_aggregate_ring   `ns` slots of slot_b() bytes, a slot = {x rows | q rows (PNA) | records | dinv, padded to 16 B | GCN
//                      coefficients (GCN, float4 rows) | CSR slice of RING_ECAP_PER_ROW entries per row}.  per_row() is what a
//                      staged row costs: the launcher sizes `cap` with it, and the offsets add up to at most cap per_row() + 15.
//                      (COPY stages no records: its offsets past the rows are never used and its rows cost the row alone.)
constexpr int RING_MAX_SLOTS = 4;
constexpr int RING_ECAP_PER_ROW = 4; // (a stage whose CSR slice is longer than 4 per row -- multigraphs, hubs -- is cut shorter by the planner)
struct RingCarve {
    int cap, w;             // rows per stage, row width (floats)
    bool hasq, hasrec, hasgc; // PNA; every mode but COPY; GCN with float4 rows
    constexpr int off_q() const { return cap * w * 4; }
    constexpr int off_rec() const { return off_q() + (hasq ? cap * w * 4 : 0); }
    constexpr int off_dinv() const { return off_rec() + cap * STACK_NODE_REC_B; }
    constexpr int off_gc() const { return off_dinv() + ((cap * 4 + 15) & ~15); }
    constexpr int off_col() const { return off_gc() + (hasgc ? cap * 16 : 0); }
    constexpr int ecap() const { return cap * RING_ECAP_PER_ROW; }
    static constexpr size_t per_row(int w, bool hasq, bool hasrec, bool hasgc)
    {
        return (size_t)w * 4 * (hasq ? 2 : 1) + (hasrec ? STACK_NODE_REC_B + 4 + 4 * RING_ECAP_PER_ROW : 0) + (hasgc ? 16 : 0);
    }
    constexpr int slot_b() const { return (int)((((size_t)cap * per_row(w, hasq, hasrec, hasgc)) + 31) & ~(size_t)15); } // (+ 16: the normalisers are padded to 16 B)
    constexpr size_t total(int ns) const { return (size_t)ns * slot_b(); }
};
// (pinned totals, worked out by hand from the launchers' expressions as they stood before the carves were shared: a drift fails the build)
static_assert(F1Carve{11, 1}.total() == 57344, "k_conv_first, F 11 (BASELINE config 2 / 4 inputs): 2 x (5632 + 4096 + 512 + 4096) + 10240 + 18432");
static_assert(F1Carve{9, 1}.total() == 55296, "k_conv_first, F 9 (config 3): 2 x (4608 + 4096 + 512 + 4096) + 10240 + 18432");
static_assert(FmCarve{9, 2, 256}.total() == 77504, "k_sage_first_mean, config 5 (F 9, d 256): 2 x (2016 + 1792 + 1792) + 8064 + 58240");
static_assert(PfCarve{11, 9}.total() == 59648, "k_pna_first, config 4 (F 11, 13 F = 143): 2 x (2816 + 2048 + 2048 + 256 + 256) + 1024 + 5888 + 37888");
static_assert(PaCarve{128}.total() == 75776, "k_pna_pagg, F 128 (config 4): 2 x (33792 + 2048 + 2048)");
static_assert(RingCarve{143, 128, false, true, false}.total(2) == 161344 && RingCarve{143, 128, false, true, false}.off_col() == 78368,
              "k_aggregate_ring, SUM, float4 rows of 128 (config 3), default options: 158 KB / 2 slots / 564 B per row = 143 rows; slot (80652 + 31) & ~15 = 80672");
static_assert(RingCarve{139, 128, false, true, true}.total(2) == 161280, "k_aggregate_ring, GCN, float4 rows of 128: 80896 / 580 = 139 rows; slot (80620 + 31) & ~15 = 80640");
static_assert(RingCarve{139, 128, false, true, true}.off_col() + 139 * RING_ECAP_PER_ROW * 4 <= RingCarve{139, 128, false, true, true}.slot_b() &&
                  RingCarve{4096, 1, true, true, false}.off_col() + 4096 * RING_ECAP_PER_ROW * 4 <= RingCarve{4096, 1, true, true, false}.slot_b(),
              "the regions of a slot end inside it");
static_assert(F1Carve{32, 2}.total() == 87040, "the widest k_conv_first: 2 x (16384 + 4096 + 512 + 4096) + 18432 + 18432 (one workgroup per CU)");
// every admissible carve fits a CU: the stage carves over every width their plans admit (k_pna_pagg with the two workgroups per
// CU it is built for), the ring over every mode, width 1..512, slot count and the ends of the budget range with the plan's cap rule
constexpr int ring_cap_of(size_t budget, int ns, size_t per_row)
{
    const int cap = (int)((budget / ns) / per_row);
    return cap < 1 ? 1 : (cap > 4096 ? 4096 : cap);
}
constexpr bool stage_carves_fit()
{
    for (int f = 1; f <= 32; f++)
        for (int kq = 1; kq <= 2; kq++)
            if (F1Carve{f, kq}.total() > (size_t)STACK_LDS_MAX)
                return false;
    for (int f = 1; f <= 16; f++)
        for (int kq = 1; kq <= 2; kq++)
            for (int nout = 64; nout <= 256; nout *= 2)
                if (FmCarve{f, kq, nout}.total() > (size_t)STACK_LDS_MAX)
                    return false;
    for (int f = 1; f <= 12; f++)
        if (PfCarve{f, (13 * f + 15) / 16}.total() > (size_t)STACK_LDS_MAX)
            return false;
    for (int f = 32; f <= 128; f *= 2)
        if (2 * PaCarve{f}.total() > (size_t)STACK_LDS_MAX)
            return false;
    return true;
}
constexpr bool ring_carves_fit(bool hasq, bool hasrec, bool hasgc)
{
    for (int w = 1; w <= 512; w++)
        for (int ns = 1; ns <= RING_MAX_SLOTS; ns++)
            for (int kb = 8; kb <= 158; kb += 150) {
                const RingCarve cv{ring_cap_of((size_t)kb * 1024, ns, RingCarve::per_row(w, hasq, hasrec, hasgc)), w, hasq, hasrec, hasgc};
                if (cv.total(ns) > (size_t)STACK_LDS_MAX || (hasrec && cv.off_col() + cv.ecap() * 4 > cv.slot_b()))
                    return false;
            }
    return true;
}
static_assert(stage_carves_fit(), "a stage carve passes 160 KB");
static_assert(ring_carves_fit(false, true, false) && ring_carves_fit(false, true, true) && ring_carves_fit(true, true, false) &&
                  ring_carves_fit(false, false, false),
              "a ring carve passes 160 KB, or a slot's regions end outside it");

// The grid of a staged producer: one workgroup per resident slot (two per CU), at most one per tile, at least one -- and MORE
// than the resident slots when a workgroup's run would pass STAGE_TCAP tiles.  Unlike stack_grid(), which refuses such a batch
// (its kernels have a fallback route), this rule WIDENS the grid: the later workgroups wait for a slot, every run stays inside
// the tile-table window.
constexpr long long producer_grid(int num_tiles, int cus)
{
    long long grid = 2LL * cus < num_tiles ? 2LL * cus : (long long)num_tiles;
    if (grid < 1)
        grid = 1;
    if ((num_tiles + grid - 1) / grid > STAGE_TCAP)
        grid = ((long long)num_tiles + STAGE_TCAP - 1) / STAGE_TCAP;
    return grid;
}

// "The max_graph_nodes promise covers every graph of the batch and whole graphs fit `cap` rows" (what graph prep validates on the
// device: flag 8).  A stage is a run of whole tiles, and a tile ends at the first graph boundary past tile_rows rows, so a tile
// holds at most promise + tile_rows - 1 rows.  A batch with a large segment fails it: the promise covers graphs
// [0, promise_graphs) only and graph prep validates nothing about the rest -- those graphs need not fit a stage, and a kernel
// that keeps a stage's rows on chip alone would give them clamped sources, unflagged.  Such a batch runs layer by layer.
struct PromiseIn {
    int max_graph_nodes, tile_rows, promise_graphs, num_graphs, large_n;
};
constexpr bool whole_graphs_fit(const PromiseIn &p, int cap)
{
    return p.max_graph_nodes > 0 && p.max_graph_nodes + p.tile_rows - 1 <= cap && p.promise_graphs >= p.num_graphs && p.large_n < 0;
}

// ---- the launch plans.  ok = false: hipErrorNotSupported, nothing launched.  (An empty batch is the launcher's own first line.)
//
// launch_conv_first.  The first row that applies:
//   | condition                                                                  | result                          |
//   |----------------------------------------------------------------------------|---------------------------------|
//   | agg_kind not GCN / SUM / MEAN; F < 1; K outside 1..32; Nout outside 1..256 | not supported                   |
//   | cat > 0 and not (cat == F, K == 2 F, MEAN); cat == 0 and K != F            | not supported                   |
//   | tile_lo != 0 (a large segment's tiles only); x not 4-B aligned             | not supported                   |
//   | otherwise                                                                  | KQ = 1 (K <= 16) or 2, MODE = agg_kind, CAT = (cat > 0) |
struct ConvFirstIn {
    int agg_kind, f, k, nout, cat, tile_lo, num_tiles, cus;
    bool x_aligned; // x at 4 B
};
struct ConvFirstPlan {
    bool ok = false, cat = false;
    int kq = 0, mode = 0;
    long long grid = 0;
    size_t lds = 0;
};
inline ConvFirstPlan plan_conv_first(const ConvFirstIn &in)
{
    ConvFirstPlan p;
    if (!(in.agg_kind == GNNB_AGG_GCN || in.agg_kind == GNNB_AGG_SUM || in.agg_kind == GNNB_AGG_MEAN) || in.f < 1 || in.k > 32 || in.k < 1 ||
        in.nout < 1 || in.nout > 256)
        return p;
    if ((in.cat > 0 && (in.cat != in.f || in.k != 2 * in.f || in.agg_kind != GNNB_AGG_MEAN)) || (in.cat == 0 && in.k != in.f))
        return p;
    if (in.tile_lo != 0 || !in.x_aligned)
        return p;
    p.kq = in.k <= 16 ? 1 : 2;
    p.mode = in.agg_kind;
    p.cat = in.cat > 0;
    p.lds = F1Carve{in.f, p.kq}.total();
    p.grid = producer_grid(in.num_tiles, in.cus);
    p.ok = true;
    return p;
}

// launch_sage_first_mean (K = 2 F).  The first row that applies:
//   | condition                                                                  | result                          |
//   |----------------------------------------------------------------------------|---------------------------------|
//   | option sage_first_mean off; F < 1; 2 F > 32; Nout not in {64, 128, 256}    | not supported                   |
//   | tile_lo != 0; x not 4-B aligned; y or mean_out not 16-B aligned            | not supported                   |
//   | whole_graphs_fit(FM_CAP) fails                                             | not supported                   |
//   | otherwise                                                                  | KQ = 1 (2 F <= 16) or 2, glog2 = log2(Nout / 4) |
struct SageFirstMeanIn {
    bool enabled; // option sage_first_mean
    int f, nout, tile_lo, num_tiles, cus;
    bool x_aligned, out_aligned; // x at 4 B; y and mean_out at 16 B
    PromiseIn promise;
};
struct SageFirstMeanPlan {
    bool ok = false;
    int kq = 0, glog2 = 0;
    long long grid = 0;
    size_t lds = 0;
};
inline SageFirstMeanPlan plan_sage_first_mean(const SageFirstMeanIn &in)
{
    SageFirstMeanPlan p;
    const int k = 2 * in.f;
    if (!in.enabled || in.f < 1 || k > 32 || !(in.nout == 256 || in.nout == 128 || in.nout == 64) || in.tile_lo != 0 || !in.x_aligned)
        return p;
    if (!whole_graphs_fit(in.promise, FM_CAP) || !in.out_aligned)
        return p;
    p.kq = k <= 16 ? 1 : 2;
    p.glog2 = lane_group_log2(in.nout / 4);
    p.lds = FmCarve{in.f, p.kq, in.nout}.total();
    p.grid = producer_grid(in.num_tiles, in.cus);
    p.ok = true;
    return p;
}

// launch_pna_first (the product is 13 F wide).  The first row that applies:
//   | condition                                                                  | result                          |
//   |----------------------------------------------------------------------------|---------------------------------|
//   | option pna_first off; F outside 1..12; Nout not in {64, 128}; ldw < 13 F   | not supported                   |
//   | tile_lo != 0; x not 4-B or y not 16-B aligned; no amp / att tables         | not supported                   |
//   | whole_graphs_fit(PF_CAP) fails                                             | not supported                   |
//   | KQ = ceil(13 F / 16): Nout > 16 KQ (the output tile is written over A0)    | not supported                   |
//   | KQ outside 8..10 (F < 9: no instantiation)                                 | not supported                   |
//   | otherwise                                                                  | KQ 8 (F 9), 9 (F 10, 11), 10 (F 12); CSL = 3 (Nout 128) or 2; glog2 = log2(Nout / 4) |
struct PnaFirstIn {
    bool enabled; // option pna_first
    int f, nout, ldw, tile_lo, num_tiles, cus;
    bool aligned, scalers; // x at 4 B and y at 16 B; the batch has its amp and att tables
    PromiseIn promise;
};
struct PnaFirstPlan {
    bool ok = false;
    int kq = 0, csl = 0, glog2 = 0;
    long long grid = 0;
    size_t lds = 0;
};
inline PnaFirstPlan plan_pna_first(const PnaFirstIn &in)
{
    PnaFirstPlan p;
    if (!in.enabled || in.f < 1 || in.f > 12 || !(in.nout == 128 || in.nout == 64) || in.tile_lo != 0 || in.ldw < 13 * in.f || !in.aligned ||
        !in.scalers)
        return p;
    if (!whole_graphs_fit(in.promise, PF_CAP))
        return p;
    p.kq = (13 * in.f + 15) / 16;
    if (in.nout > 16 * p.kq || p.kq < 8 || p.kq > 10)
        return p;
    p.csl = in.nout == 128 ? 3 : 2;
    p.glog2 = lane_group_log2(in.nout / 4);
    p.lds = PfCarve{in.f, p.kq}.total();
    p.grid = producer_grid(in.num_tiles, in.cus);
    p.ok = true;
    return p;
}

// launch_pna_pagg.  The first row that applies:
//   | condition                                                                  | result                          |
//   |----------------------------------------------------------------------------|---------------------------------|
//   | option pna_pagg off; F not in {32, 64, 128}; tile_lo != 0                  | not supported                   |
//   | whole_graphs_fit(PA_CAP) fails                                             | not supported                   |
//   | x, wb or out not 16-B aligned; ldw no multiple of 4                        | not supported                   |
//   | otherwise                                                                  | KQ = F / 16; MX = 2 (math 3: f16x3, REDUCED precision) or 0 |
struct PnaPaggIn {
    bool enabled; // option pna_pagg
    int f, ldw, tile_lo, math, num_tiles, cus;
    bool aligned; // x, wb, out at 16 B
    PromiseIn promise;
};
struct PnaPaggPlan {
    bool ok = false;
    int kq = 0, mx = 0;
    long long grid = 0;
    size_t lds = 0;
};
inline PnaPaggPlan plan_pna_pagg(const PnaPaggIn &in)
{
    PnaPaggPlan p;
    if (!in.enabled || !(in.f == 128 || in.f == 64 || in.f == 32) || in.tile_lo != 0)
        return p;
    if (!whole_graphs_fit(in.promise, PA_CAP))
        return p;
    if (!in.aligned || (in.ldw & 3))
        return p;
    p.kq = in.f / 16;
    p.mx = in.math == 3 ? 2 : 0;
    p.lds = PaCarve{in.f}.total();
    p.grid = producer_grid(in.num_tiles, in.cus);
    p.ok = true;
    return p;
}

// launch_aggregate_ring_t<MODE, VEC> (never "not supported"; empty = nothing to walk, success).  In this order:
//   | value      | rule                                                                                         |
//   |------------|----------------------------------------------------------------------------------------------|
//   | tile_lo    | the batch's, clamped to 0..num_tiles; empty when no tile is left                              |
//   | glog2      | lanes per row: lane_group_log2(w / VEC)                                                        |
//   | wgs        | option agg_ring_wg_per_cu, at least 1                                                          |
//   | budget     | option agg_lds_kb clamped to 8..158 KB when set, else 158 / wgs KB                             |
//   | ns         | option agg_ring_slots clamped to 1..RING_MAX_SLOTS                                             |
//   | nw         | option agg_ring_waves clamped to 1..16; 0 = 16 (measured: 16 waves issue a stage's DMA and drain its stores faster than 8) |
//   | cap        | one ring per workgroup, stages as large as the budget allows: budget / ns / per_row, clamped to 1..4096 |
//   | grid       | persistent: cus x wgs, at most one per tile, at least 1                                        |
//   | use_cut    | graph prep's row-balanced ranges: option agg_balance, tile_lo == 0, a table made for exactly this grid |
//   | slack      | tile_rows / 2 (at least 1) + 2: what the equal-stage cut may add to a stage                    |
//   | nt         | option agg_nt_store: the NT instantiation                                                      |
struct RingIn {
    int mode, vec, w, num_tiles, tile_lo, tile_rows, cus;
    int wg_per_cu, lds_kb, slots, waves, balance, nt_store; // options agg_ring_wg_per_cu, agg_lds_kb, agg_ring_slots, agg_ring_waves, agg_balance, agg_nt_store
    bool has_cut;  // the batch has a cut table
    int cut_n;     // ... made for this many workgroups
};
struct RingPlan {
    bool empty = true, use_cut = false, nt = false;
    int tile_lo = 0, glog2 = 0, nw = 0, ns = 0, cap = 0, ecap = 0, slot_bytes = 0, slack = 0, tile_rows = 0, grid = 0;
    size_t lds = 0;
};
inline RingPlan plan_aggregate_ring(const RingIn &in)
{
    RingPlan p;
    p.tile_lo = in.tile_lo < 0 ? 0 : (in.tile_lo > in.num_tiles ? in.num_tiles : in.tile_lo);
    if (in.num_tiles - p.tile_lo <= 0)
        return p;
    p.empty = false;
    p.glog2 = lane_group_log2(in.w / in.vec);
    const bool hasq = in.mode == GNNB_AGG_PNA, hasrec = in.mode != GNNB_AGG_COPY, hasgc = in.mode == GNNB_AGG_GCN && in.vec == 4;
    const size_t per_row = RingCarve::per_row(in.w, hasq, hasrec, hasgc);
    const int wgs = in.wg_per_cu > 1 ? in.wg_per_cu : 1;
    const size_t budget = (size_t)(in.lds_kb > 0 ? (in.lds_kb < 8 ? 8 : in.lds_kb > 158 ? 158 : in.lds_kb) : 158 / wgs) * 1024;
    p.ns = in.slots < 1 ? 1 : (in.slots > RING_MAX_SLOTS ? RING_MAX_SLOTS : in.slots);
    p.nw = in.waves <= 0 ? 16 : (in.waves > 16 ? 16 : in.waves);
    const int cap = (int)((budget / p.ns) / per_row);
    p.cap = cap < 1 ? 1 : (cap > 4096 ? 4096 : cap);
    const RingCarve cv{p.cap, in.w, hasq, hasrec, hasgc};
    p.ecap = cv.ecap();
    p.slot_bytes = cv.slot_b();
    p.lds = cv.total(p.ns);
    p.grid = in.cus * wgs;
    if (p.grid > in.num_tiles - p.tile_lo)
        p.grid = in.num_tiles - p.tile_lo;
    if (p.grid < 1)
        p.grid = 1;
    p.use_cut = in.balance && p.tile_lo == 0 && in.has_cut && in.cut_n == p.grid;
    p.slack = (in.tile_rows / 2 > 1 ? in.tile_rows / 2 : 1) + 2;
    p.tile_rows = in.tile_rows > 1 ? in.tile_rows : 1;
    p.nt = in.nt_store != 0;
    return p;
}

// =====================================================================================
// device side: the skeleton of a staged kernel
// =====================================================================================
// a stage: rows [nb, nb + rows) and CSR entries [e0, e0 + ne) of a run of whole tiles; next_t = the tile the next stage starts at
struct Stage {
    int ok, nb, rows, e0, ne, next_t;
};

// The window of the tile table a workgroup keeps in registers for its run [t0, t1) (run_cuts, never empty here): lane l holds the
// first row (tf) and the first CSR entry (te) of tile t0 + l (the launcher keeps runs at STAGE_TCAP tiles: the run's end is a lane
// of the window too).  Clamped: the tables of a malformed (flagged) batch may hold stale entries and must still stay in range.
__device__ __forceinline__ void stage_window(const int32_t *tile_first, const int32_t *tile_edge, int num_tiles, int N, int E, int lane, int t0,
                                             int t1, int &tf, int &te)
{
    const int ti = min(t0 + min(lane, t1 - t0), num_tiles);
    tf = min(max(tile_first[ti], 0), N);
    te = min(max(tile_edge[ti], 0), E);
}

// The longest run of whole tiles from tile `ts` whose rows fit a stage of CAP rows (the three kernels that need the
// max_graph_nodes promise; a CSR slice past the kernel's ECAP is not staged: rows of degree > 4 read `col` from global memory).
// k_conv_first, which also takes graphs beyond a stage, has its own planner.
template <int CAP>
__device__ __forceinline__ Stage stage_plan(int ts, int t0, int t1, int lane, int tf, int te)
{
    Stage st;
    st.ok = ts < t1 ? 1 : 0;
    st.nb = st.rows = st.e0 = st.ne = 0;
    st.next_t = ts;
    if (!st.ok)
        return st;
    const int rel = ts - t0;
    const int nb = __builtin_amdgcn_readlane(tf, rel), e0 = __builtin_amdgcn_readlane(te, rel);
    const unsigned long long fit = __ballot(lane > rel && lane <= t1 - t0 && tf - nb <= CAP);
    st.nb = nb;
    st.e0 = e0;
    int endl = rel + 1; // (nothing fits: the next tile alone, cut to the stage -- only if the max_graph_nodes promise is broken)
    if (fit) {
        const unsigned long long nofit = ~fit & (~0ull << (rel + 1));
        endl = nofit ? __builtin_ctzll(nofit) - 1 : 63 - __builtin_clzll(fit);
    }
    st.rows = min(max(__builtin_amdgcn_readlane(tf, endl) - nb, 0), CAP);
    st.ne = max(__builtin_amdgcn_readlane(te, endl) - e0, 0);
    st.next_t = t0 + endl;
    return st;
}

} // namespace gnnb
