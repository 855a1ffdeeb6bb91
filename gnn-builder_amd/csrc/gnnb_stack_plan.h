// gnnb_stack_plan.h -- the LDS carves and the launch plans of the conv-stack kernels (k_stack.hip: k_gcn2_fused; k_stack_zf.h:
// k_gcn2_zf), each stated ONCE: the kernel takes its region sizes and offsets from the carve, the launcher its dynamic-LDS size
// from the same carve's total(), and graph prep its stage rows, tile capacities and grids from the same plan constants.
// Plain integer arithmetic: no HIP call and no options() in here (the launchers read the options and the device and pass them in);
// everything a kernel uses is constexpr, which the HIP compiler takes as host and device code alike.
#pragma once
#include <stddef.h>

#include "gnnb_hip.h"

namespace gnnb {

// ---- layout constants both kernels share
constexpr int STACK_NODE_REC_B = 32;  // a node's record pair in BatchTables::node_rec (2 x int4), staged beside its x row
constexpr int STACK_NODE_REC_Q = STACK_NODE_REC_B / 16; // ... in int4
constexpr int STACK_ROW_REC_B = 48;   // the per-row aggregation record P0 writes (3 x int4: offsets, coefficients, {dinv^2, rp0, deg, dinv})
constexpr int STACK_ROW_REC_Q = STACK_ROW_REC_B / 16; // ... in int4
constexpr int STACK_REC_DMA_B = 1024; // the node records go to LDS in one 16-B DMA piece per lane: 1 KiB per wave
constexpr int STACK_GRAPH_WIN = 64;   // graph boundaries of a stage the boundary window in LDS holds (more: read from global memory)
constexpr int STACK_LDS_MAX = 160 * 1024; // LDS of a gfx950 CU

// =====================================================================================
// k_gcn2_zf
// =====================================================================================
// Two shapes: wide = ONE 16-wave workgroup per CU, 176-row stages (11 MFMA units), input widths up to 16 (one MFMA k block:
// with two the carve would pass 160 KB); narrow = TWO 8-wave workgroups per CU, 96-row stages (6 units).
constexpr int ZF_WIDE_ROWS = 176, ZF_NARROW_ROWS = 96;
constexpr int ZF_TCAP = 62; // tiles per workgroup: the run's table lives in one register per lane (+ its end)
// option zf_shape: 0 = narrow everywhere, 1 / 2 = wide wherever it exists
constexpr bool zf_wide_shape(int f0, int zf_shape) { return f0 <= 16 && zf_shape != 0; }
constexpr int zf_stage_rows_of(int f0, int zf_shape) { return zf_wide_shape(f0, zf_shape) ? ZF_WIDE_ROWS : ZF_NARROW_ROWS; }
constexpr int zf_wg_per_cu(bool wide) { return wide ? 1 : 2; }

// LDS carve (bytes, every region 16-B aligned), in this order:
//   ROWS   xs | srec                     ONE buffer (P0 is its only reader; refilled one stage ahead)
//   SMALL  sdinv | node_ptr of <= GMAX graphs (+ end)    TWO buffers
//   A0     [cap][LD0]                    P0 -> M0
//   H      [cap][ldh]                    M0 -> M1, then Z in place -> P1
//   REC    [cap] x 48 B                  TWO buffers (P0 of the next stage writes while P1 of this one reads)
//   SCOL   [ECAP] int32                  TWO buffers: the stage's slice of the CSR `col` array, for rows of degree > 4
//                                        (a tracked global read there costs a full memory round trip per neighbour)
//   SB1, SPLAN, SB0, STAB                biases, the plan of the stage after next, the planner wave's tile-table copy
// (What depends on the stage rows and KQ0 alone is a static function of them: the kernel needs those as compile-time constants
// of its template parameters.  What also depends on the run-time widths f0 / h1 is a member function.)
struct ZfCarve {
    int cap, f0, kq0, h0, h1; // stage rows, input width, 16-wide k blocks of layer 0, hidden width, last layer's width

    static constexpr int SB_B = 128 * 4;   // b1 / b0 zero-padded to 128 floats
    static constexpr int SPLAN_B = 2 * 16; // the stage after next, planned by ONE wave (2 x int4)
    static constexpr int STAB_B = 3 * 64 * 4; // the planner wave's copy of the run's tile-table entries (3 x 64)

    static constexpr int gmax(int cap) { return cap <= 96 ? STACK_GRAPH_WIN : 2 * STACK_GRAPH_WIN; } // graph boundaries of a stage kept in LDS (more: empty graphs piling up)
    static constexpr int ecap(int cap) { return cap <= 96 ? 512 : 1024; }
    static constexpr int small_b(int cap) { return cap * 4 + ((gmax(cap) + 1) * 4 + 15) / 16 * 16; }
    static constexpr int a0_b(int cap, int kq0) { return cap * (16 * kq0) * 4; } // A0 row: F0 values zero-padded to whole 16-wide MFMA k blocks
    static constexpr int rec_b(int cap) { return cap * STACK_ROW_REC_B; }

    constexpr int xs_b() const { return ((cap * f0 * 4) + 15) & ~15; }
    constexpr int rows_b() const { return xs_b() + cap * STACK_NODE_REC_B; }
    constexpr int ldh() const { return (h0 > h1 ? h0 : h1) + 4; } // padded H / Z row (floats): conflict-free fragment reads, base + immediate
    constexpr int ldhb() const { return ldh() * 4; }
    constexpr int h_b() const { return cap * ldhb(); }
    constexpr int tail_b() const { return SB_B + SPLAN_B + SB_B + STAB_B; }

    constexpr int a0_off() const { return rows_b() + 2 * small_b(cap); }
    constexpr int h_off() const { return rows_b() + 2 * small_b(cap) + a0_b(cap, kq0); }
    constexpr size_t total() const
    {
        return (size_t)h_off() + (size_t)h_b() + 2 * (size_t)rec_b(cap) + 2 * (size_t)ecap(cap) * 4 + (size_t)tail_b();
    }
};
// (pinned totals, worked out by hand from the carve as it stood before it was shared: a drift fails the build)
static_assert(ZfCarve{176, 11, 1, 128, 128}.total() == 146944, "k_gcn2_zf, wide shape, BASELINE config 2: 13376 + 2*1232 + 11264 + 92928 + 16896 + 8192 + 1824");
static_assert(ZfCarve{96, 11, 1, 128, 128}.total() == 80576, "k_gcn2_zf, 96-row shape, BASELINE config 2: 7296 + 2*656 + 6144 + 50688 + 9216 + 4096 + 1824");
static_assert(ZfCarve{96, 32, 2, 128, 128}.total() == 94784, "k_gcn2_zf, 96-row shape, widest input: 15360 + 2*656 + 12288 + 50688 + 9216 + 4096 + 1824");
static_assert(ZfCarve{176, 16, 1, 128, 128}.total() <= STACK_LDS_MAX && ZfCarve{96, 32, 2, 128, 128}.total() <= STACK_LDS_MAX,
              "the largest carve of either shape fits a CU");
static_assert(ZfCarve{176, 32, 2, 128, 128}.total() > STACK_LDS_MAX, "why the wide shape stops at input width 16: with two k blocks of A0 the widest input does not fit");

// What launch_gcn2_zf decides, as a pure function of plain integers.  The first row that applies:
//
//   | condition                                                                          | result                              |
//   |------------------------------------------------------------------------------------|-------------------------------------|
//   | promise <= 0, or promise + tile_rows - 1 > stage rows                              | not supported (no promise that whole graphs fit a stage) |
//   | f0 outside 1..32, h0 not in {32, 64, 128}, h1 outside 4..128 or not a multiple of 4 | not supported                       |
//   | an operand misaligned (w1, pooled, b1: 16 B; x: 4 B)                               | not supported                       |
//   | carve total > 160 KB                                                               | not supported                       |
//   | wide shape (f0 <= 16 and zf_shape != 0)                                            | NW 16, 11 units, 176 rows, one workgroup per CU; MX = 1 (math 2), 2 (math 3), else 0; H1FULL = (h1 == h0) |
//   | otherwise                                                                          | NW 8, 6 units, 96 rows, two workgroups per CU, MX 0, H1FULL no |
//
//   KQ0 = 1 (f0 <= 16) or 2, KQ1 = h0 / 16.  (math 1, the bf16x6 mode, does not switch this kernel off: its fp32 form is faster
//   than the bf16x6 form of k_gcn2_fused and the mode must never be slower than the default.)
//   head (the MLP head runs inside the kernel, HEAD instantiations): one is on offer (head_ld > 0: option zf_head, the small
//   form's shape conditions hold), it has at least two linears, its input is the pooled row (num_pools h1) and its activation
//   tiles -- one per group of four waves + two -- fit the H region.
// The grid is stack_grid() below: it needs the occupancy of the instantiation this plan picks.
struct ZfPlanIn {
    int f0, h0, h1, math, promise, tile_rows, zf_shape;
    bool aligned;                                // w1, pooled, b1 at 16 B and x at 4 B
    int head_ld, head_nlin, head_in, num_pools;  // head_ld = head_small_ldact() of the head on offer, 0 = none
};
struct ZfPlan {
    bool ok = false, wide = false, h1full = false, head = false;
    int cap = 0, kq0 = 0, kq1 = 0, nw = 0, units = 0, mx = 0, wg_per_cu = 0, head_ldact = 0;
    size_t lds = 0;
};
inline ZfPlan plan_gcn2_zf(const ZfPlanIn &in)
{
    ZfPlan p;
    p.wide = zf_wide_shape(in.f0, in.zf_shape);
    p.cap = zf_stage_rows_of(in.f0, in.zf_shape);
    if (in.promise <= 0 || in.promise + in.tile_rows - 1 > p.cap)
        return p;
    if (in.f0 < 1 || in.f0 > 32 || !(in.h0 == 32 || in.h0 == 64 || in.h0 == 128) || in.h1 < 4 || in.h1 > 128 || (in.h1 & 3))
        return p;
    if (!in.aligned)
        return p;
    p.kq0 = in.f0 <= 16 ? 1 : 2;
    p.kq1 = in.h0 / 16;
    const ZfCarve cv{p.cap, in.f0, p.kq0, in.h0, in.h1};
    p.lds = cv.total();
    if (p.lds > (size_t)STACK_LDS_MAX)
        return p;
    p.nw = p.wide ? 16 : 8;
    p.units = p.cap / 16;
    p.wg_per_cu = zf_wg_per_cu(p.wide);
    p.mx = p.wide ? (in.math == 2 ? 1 : in.math == 3 ? 2 : 0) : 0; // (the bf16x3 / f16x3 forms of M1 exist in the wide shape only)
    p.h1full = p.wide && in.h1 == in.h0;
    const int groups = p.nw / 4;
    if (in.head_ld > 0 && in.head_nlin >= 2 && in.head_in == in.num_pools * in.h1 &&
        (size_t)(groups + 2) * 16 * in.head_ld * 4 <= (size_t)cv.h_b()) {
        p.head = true;
        p.head_ldact = in.head_ld;
    }
    p.ok = true;
    return p;
}

// =====================================================================================
// k_gcn2_fused
// =====================================================================================
constexpr int g2_units(int math) { return math ? 3 : 4; } // 16-row MFMA units per stage (bf16x6: three)
constexpr int G2_TCAP = 64;      // tile-table entries a workgroup keeps in LDS
constexpr int G2_WG = 512;       // 8 waves; two workgroups per CU = 4 waves per SIMD
constexpr int G2_NW = G2_WG / 64;
constexpr int G2_WG_PER_CU = 2;
// A run of n tiles takes n + 1 table entries, so the LDS window admits runs of G2_TCAP - 1 tiles: that is what the launcher
// checks (min_grid) and what the kernel and the stage-cut planner clamp a run to.  Graph prep sizes its tiles against ONE LESS
// (G2_TCAP - 2 per workgroup): historical slack, kept as it is -- it decides tile_rows for very large batches.
constexpr int G2_RUN_TILES = G2_TCAP - 1;
constexpr int G2_PREP_TILES = G2_TCAP - 2;

// LDS carve (bytes, every region 16-B aligned), in this order:
//   ROWS   xs | srec                ONE buffer: read by P0 only, refilled right behind P0
//   SMALL  sdinv | node_ptr of <= 64 graphs (+ end)   TWO buffers (P1 and the pooling still read them)
//   H      [cap][ldh]
//   A1     fp32: [cap][h0 + 4]; bf16x6: three bf16 planes [cap][2 h0 + 16 B].  A0 lives in its head (P0 writes it, M0 reads
//          it, P1 overwrites it), so the region is as large as the larger of the two
//   REC    [cap] x 48 B
//   tile tables  stile | sgraph, G2_TCAP + 1 entries each
// (h_off, lda1, prow_b and plane_b feed total() and a1_used_b(); the kernel spells these four itself, with a comment at each:
// taken from here they moved the f16x3 deep variants' machine code)
struct G2Carve {
    int cap, f0, kq0, h0, h1, math; // math: 0 fp32, 1 bf16x6 (the kernel's MATH)

    static constexpr int GRAPH_WIN_B = (STACK_GRAPH_WIN + 1 + 3) * 4; // 65 boundary words, padded to 16 B: 272
    static constexpr int TABLES_B = 2 * (G2_TCAP + 1) * 4;

    constexpr int xs_b() const { return ((cap * f0 * 4) + 15) & ~15; }
    constexpr int rows_b() const { return xs_b() + cap * STACK_NODE_REC_B; }
    constexpr int small_b() const { return cap * 4 + GRAPH_WIN_B; }
    constexpr int ldh() const { return (h0 > h1 ? h0 : h1) + 4; } // padded H row (floats)
    constexpr int h_off() const { return rows_b() + 2 * small_b(); }
    constexpr int h_b() const { return cap * ldh() * 4; }
    constexpr int lda1() const { return h0 + 4; }
    constexpr int prow_b() const { return h0 * 2 + 16; }
    constexpr int plane_b() const { return cap * prow_b(); }
    constexpr int a1_used_b() const { return math ? 3 * plane_b() : cap * lda1() * 4; } // where REC starts behind A1
    constexpr int a0_b() const { return cap * (16 * kq0) * 4; }
    constexpr size_t a1_b() const { return a1_used_b() > a0_b() ? (size_t)a1_used_b() : (size_t)a0_b(); }
    constexpr int rec_b() const { return cap * STACK_ROW_REC_B; }
    constexpr size_t total() const
    {
        return (size_t)h_off() + (size_t)h_b() + a1_b() + (size_t)rec_b() + (size_t)TABLES_B;
    }
};
static_assert(G2Carve::GRAPH_WIN_B == 272, "65 graph-boundary words in 68");
static_assert(G2Carve{64, 11, 1, 128, 128, 0}.total() == 77096, "k_gcn2_fused, fp32, BASELINE config 2 / 3 widths: 4864 + 2*528 + 33792 + 33792 + 3072 + 520");
static_assert(G2Carve{48, 11, 1, 128, 128, 1}.total() == 71912, "k_gcn2_fused, bf16x6: 3648 + 2*464 + 25344 + 39168 + 2304 + 520");
static_assert(2 * G2Carve{64, 16, 1, 128, 128, 0}.total() <= STACK_LDS_MAX, "two workgroups per CU at every one-block input width");

// the deep (more than two GCN layers) variants have no register to spare: at hidden 128 only ReLU stacks take f16x3, GELU never
constexpr bool g2_deep_takes_h3(int act, int kq1) { return act == GNNB_ACT_RELU || (act != GNNB_ACT_GELU && kq1 < 8); }

// What launch_gcn2_fused decides, as a pure function of plain integers.  The first row that applies:
//
//   | condition                                                                          | result                              |
//   |------------------------------------------------------------------------------------|-------------------------------------|
//   | nl < 2; nl > 2 without usable middle weights (present, 16-B aligned, stride % 4 == 0) | not supported                    |
//   | GIN with h1 > h0, or without usable middle weights and biases                      | not supported                       |
//   | promise <= 0, or promise + tile_rows - 1 > stage rows                              | not supported                       |
//   | f0 outside 1..32, h0 not in {32, 64, 128}, h1 outside 4..128 or not a multiple of 4 | not supported                       |
//   | an operand misaligned (w1, pooled: 16 B; x: 4 B)                                   | not supported                       |
//   | GIN                                                                                | MATH 0, variant GIN, H3 = (math == 3) |
//   | two GCN layers, math != 0                                                          | MATH 1 (bf16x6, 48-row stages), plain |
//   | more than two GCN layers                                                           | MATH 0, variant DEEP, H3 = (math == 3 and g2_deep_takes_h3) |
//   | otherwise                                                                          | MATH 0, plain                       |
//
//   Stage rows = 16 g2_units(MATH); KQ0 = 1 (f0 <= 16) or 2, KQ1 = h0 / 16; always G2_WG threads, two workgroups per CU.
//   (The opt-in modes exist for some forms only; every other model runs its fp32 kernel in either mode -- a mode may never
//   make a model slower by sending it down the layer-by-layer path.)
struct G2PlanIn {
    int f0, h0, h1, act, nl, gin, math, promise, tile_rows;
    bool mid_ok, bmid; // middle weights present + 16-B aligned + stride % 4 == 0; middle biases present
    bool aligned;      // w1, pooled at 16 B and x at 4 B
};
struct G2Plan {
    bool ok = false, h3 = false;
    int math = 0, cap = 0, kq0 = 0, kq1 = 0, variant = 0; // variant: 0 plain, 1 DEEP, 2 GIN
    size_t lds = 0;
};
inline G2Plan plan_gcn2_fused(const G2PlanIn &in)
{
    G2Plan p;
    if (in.nl < 2 || (in.nl > 2 && !in.mid_ok))
        return p;
    if (in.gin && (in.h1 > in.h0 || !in.mid_ok || !in.bmid))
        return p;
    p.math = (in.math && in.nl == 2 && !in.gin) ? 1 : 0;
    p.cap = 16 * g2_units(p.math);
    if (in.promise <= 0 || in.promise + in.tile_rows - 1 > p.cap)
        return p;
    if (in.f0 < 1 || in.f0 > 32 || !(in.h0 == 32 || in.h0 == 64 || in.h0 == 128) || in.h1 < 4 || in.h1 > 128 || (in.h1 & 3))
        return p;
    if (!in.aligned)
        return p;
    p.kq0 = in.f0 <= 16 ? 1 : 2;
    p.kq1 = in.h0 / 16;
    p.lds = G2Carve{p.cap, in.f0, p.kq0, in.h0, in.h1, p.math}.total();
    p.variant = in.gin ? 2 : (!p.math && in.nl > 2) ? 1 : 0;
    p.h3 = in.math == 3 && (p.variant == 2 || (p.variant == 1 && g2_deep_takes_h3(in.act, p.kq1)));
    p.ok = true;
    return p;
}

// =====================================================================================
// both: the grid
// =====================================================================================
// One workgroup per resident slot (cus x blocks_per_cu: the occupancy of the picked instantiation at its LDS size), at most one
// per tile; a workgroup's run may span tiles_per_wg tiles (ZF_TCAP, G2_RUN_TILES), so fewer workgroups than min_grid cannot
// walk the batch: not supported.
struct StackGrid {
    bool ok;
    long long min_grid, grid;
};
constexpr StackGrid stack_grid(int num_tiles, int tiles_per_wg, int cus, int blocks_per_cu)
{
    StackGrid g{false, ((long long)num_tiles + tiles_per_wg - 1) / tiles_per_wg, (long long)cus * blocks_per_cu};
    if (g.grid > num_tiles)
        g.grid = num_tiles;
    g.ok = g.grid >= g.min_grid;
    return g;
}

// ---- what graph prep asks (before a batch's tables exist): values as the plans above give them
// node tiles k_gcn2_zf can walk in one launch
constexpr long zf_tile_capacity_of(int f0, int zf_shape, int cus) { return (long)ZF_TCAP * zf_wg_per_cu(zf_wide_shape(f0, zf_shape)) * cus; }
// ... k_gcn2_fused, at G2_PREP_TILES per workgroup (see above)
constexpr long g2_tile_capacity_of(int cus) { return (long)G2_PREP_TILES * G2_WG_PER_CU * cus; }
// workgroups k_gcn2_fused launches for that many node tiles when the occupancy is the G2_WG_PER_CU it is built for (the stage-cut
// planner cuts for this grid; the launcher takes the cuts only when its own grid is the same)
constexpr int g2_grid_of(int num_tiles, int cus)
{
    const long long g = stack_grid(num_tiles, G2_RUN_TILES, cus, G2_WG_PER_CU).grid;
    return (int)(g > 1 ? g : 1);
}

} // namespace gnnb
