// k_linear_dma.hip -- dense update on the fp32 matrix cores, LDS-DMA chunk pipeline: k_linear_dma (row slices, stream-K, pooling
// epilogue, row classes) and k_pool_combine, which finishes what the pooling epilogue parks
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include "gnnb_gemm.h"

namespace gnnb {

// -------------------------------------------------------------------------------------
// LDS-DMA form of the tiled GEMM (k_linear.hip, where the operation is stated) for the regular case -- rows 16-B aligned, segment widths whole
// 32-wide chunks (GraphSAGE at d = 256: [mean | x] . [Wl | Wr]^T, K = 2 x 256; PNA at d = 128: 13 x 128 with
// two row-scaled segments, the scaler applied to the A fragments).
// Same 32x32x2 MFMA schedule (and summation order) as k_linear, but the A and W chunks go global -> LDS directly
// (untracked global_load_lds, no VGPR staging, no ds_write).  LDS rows are unpadded [row][32 floats]; 16-B pieces
// are XOR-swizzled through the DMA *source* address (slot = piece ^ (row & 7)), which keeps the ds_read_b128
// fragment reads conflict-free.
//
// Shape: two 4-wave workgroups per CU (they fill each other's barrier gaps), 128 x 128 output tile, two chunk buffers;
// the constants below also express the other shape that was built and measured -- ONE 8-wave workgroup per CU, 256 x
// 128 tile, three-deep chunk ring (DM 256, DWG 512, DNBUF 3, DWGPC 1): 579 / 544 us against 592 / 535 us at the C4 /
// C5 shapes, a wash, every barrier idles the whole CU.  What mattered was in the generated code: without its chunk DMA
// the kernel ran at 84 % of the fp32 MFMA peak, with it at 65 % -- see the note on compiler-tracked loads in the item
// body.
// (DM, DN, DWGPC: gnnb_gemm.h -- the planner and the stream-K scratch size need them)
static constexpr int DWG = 256, DNBUF = 2, DNW = DWG / 64;
// The swizzle key of a chunk row.  Round 6 (profiles/r06_c{4,5}_kernels_pmc.json: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.43-0.50 in
// this kernel): with slot = piece ^ (row & 7) a ds_read_b128 -- served in groups of SIXTEEN lanes over 64 banks (256 B), rows
// {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of the 32-row fragment -- puts rows r and r + 8 (mod 16) of one parity on the same slot:
// every fragment read a two-way conflict.  Rows are 128 B: the row's parity selects the half of the 256-B bank window, so the key
// must separate the EIGHT rows of one parity inside a group: key = (row >> 1) & 7 does (even rows of the first group: 0 1 6 7 2 3 4 5).
__device__ __forceinline__ int dkey(int r) { return (r >> 1) & 7; }
static constexpr int DBUF_B = (DM + DN) * BK * 4; // 32 KB: A chunk | W chunk
// MATH 1 (opt-in, gnnb_set_option("math", 1)): the same chunks, but each 16-wide k block is multiplied as six
// v_mfma_f32_32x32x16_bf16 products of an exact 3-way bf16 split of BOTH operands (see split3), the fragments split in
// the wave after the LDS read -- 24 MFMA of 8 passes instead of 32 of 16 per k block and accumulator quartet.
// MATH 2 (opt-in, gnnb_set_option("math", 3), REDUCED precision, round 5): hi + mid fp16 pieces of both operands, three
// v_mfma_f32_32x32x16_f16 products per k block -- ~22 significant bits per product, fp16's range (gnnb_device.h).
// POOL: the pooling epilogue as its own instantiation (as a run-time branch of the one kernel it cost the plain GEMM 6-8 %:
// 109 -> 101 TFLOP/s at the C4 shape, round 4)
// RC (round 4, PNA with a degree promise): the rows of A and Y are taken through a permutation that sorts them into DEGREE
// CLASSES, and every 128-row tile multiplies by the weight matrix of its class (RowClasses): PNA's scalers depend on the
// in-degree only, so [x | A | amp(d) A | att(d) A] . W^T = [x | A] . (W_x | W_1 + amp(d) W_2 + att(d) W_3)^T -- 5 F wide
// instead of 13 F.  M is then the length of the sorted space (whole tiles), perm[position] = row or -1 (padding: loads
// re-read row 0, nothing is stored).
template <int MATH, int MODE>
__global__ __launch_bounds__(DWG) void k_linear_dma(GemmArgs g, const float *__restrict__ W, int ldw,
                                                    const float *__restrict__ bias,
                                                    const float *__restrict__ skip, float *__restrict__ Y, int M,
                                                    int N, int act, int tiles_m, int tiles_n, int split_from, int split,
                                                    PoolEpilogue pe, StreamK sk, RowClasses rc, int bias_in_lds,
                                                    int32_t *__restrict__ err, int32_t *__restrict__ err_host) // MATH 2: GNNB_FLAG_RANGE (gnnb_device.h RangeProbe)
{
    constexpr bool POOL = MODE == 1, RC = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1; // 2 x 2 waves: 64 rows x 64 columns each (a 32-row slice: 1 x 4 waves, 32 columns each)
    const int total = g.cpre[g.nseg];
    const int li = lane & 31, lh = lane >> 5;
    const uint32_t smem_a = (uint32_t)(uintptr_t)(lds_vptr)smem;
    // DMA lane geometry: an instruction covers 8 rows x eight 16-B pieces; LDS slot p of row r holds piece p ^ dkey(r)
    const int drow = lane >> 3;
    // (the key of local row r0 + drow, r0 a multiple of 8: with the key's shift of 1 it carries bit 3 of r0 -- two lane constants)
    const uint32_t dpiece_b0 = (uint32_t)(((lane & 7) ^ dkey(drow)) << 4), dpiece_b1 = (uint32_t)(((lane & 7) ^ dkey(8 + drow)) << 4);

    // PERSISTENT over work items (grid = what is resident: two workgroups per CU); the chunk pipeline runs straight
    // across item boundaries.  TAIL SPLIT: tiles / CUs is rarely whole (PNA at C4: 1153 tiles on 256 CUs = 4.5 per CU,
    // paid as 5).  Tiles from `split_from` on -- the last, partial round -- are handed out as `split` (2 or 4) row
    // slices each, so that the round costs a half or a quarter tile.  A slice keeps the tile's MFMA order per output
    // element: 64 rows = one 32-row accumulator block per wave instead of two, 32 rows = 1 x 4 waves of 32 x 32.
    // STREAM-K (round 4, sk.q > 0): the tiles from `split_from` on are not sliced by rows -- a 32-row slice keeps the whole K
    // loop, whose chunks are then too small to cover the DMA round trip: at the C4 shape the quarter-tile round cost 80 us
    // where a quarter of a round is 57, and 153 us when 4 x 129 slices just missed the 512 resident workgroups.  Instead
    // their (tile, chunk) space is cut into equal runs of q chunks, one run per workgroup: a partial tile, whole tiles, a
    // partial tile.  A workgroup multiplies its run at full tile width; where it holds only a part of a tile's K it parks the
    // accumulators in sk.part[2 * workgroup + (0: the run's first tile, 1: its last)], and the LAST workgroup to arrive at a
    // tile (sk.cnt, one counter per SHARED tile, indexed by the first run that touches the tile -- a run begins inside one tile
    // at most, so the index is unique and < gridDim.x <= SK_MAX_WG whatever the tile count --, reset by that workgroup) adds
    // the parts up IN RUN ORDER and runs the epilogue:
    // deterministic, one summation order per shape.  The launcher puts ALL tiles into that space when there is at least one
    // whole round of them (split_from = 0: no last round is left), else the tiles of the partial round.
    // The bias through LDS (round 5, not in the row-class mode, whose bias changes with the tile): read from global memory
    // inside the epilogue it is a load the compiler tracks, and the s_waitcnt in front of its first use also waits for the
    // chunk DMA of the NEXT item that is in flight by then -- ~9.5 k cycles per tile with nothing of the workgroup on the
    // matrix pipe (tools/gemm_k_sweep.py: t = 56.8 us + 0.506 us K at 4 tiles per workgroup before).  Staged HERE, in front
    // of the first DMA issue; the epilogue reads it with ds_read (lgkmcnt).  The launcher adds the bytes when N is small enough.
    float *const sbias = reinterpret_cast<float *>(smem + (size_t)DNBUF * DBUF_B + 16);
    const bool bias_lds = !RC && bias != nullptr && bias_in_lds != 0;
    if (bias_lds)
        for (int i = tid; i < N; i += DWG)
            sbias[i] = bias[i];
    const int num_tiles = tiles_m * tiles_n;
    const bool skm = sk.q > 0;
    const int num_items = skm ? split_from : split_from + split * (num_tiles - split_from); // handed out round-robin
    const int sk_total = skm ? (num_tiles - split_from) * total : 0;
    const int sk_g0 = min((int)blockIdx.x * sk.q, sk_total), sk_g1 = min(sk_g0 + sk.q, sk_total);
    const int sk_t0 = sk_g0 / total;
    const int sk_nseg = sk_g1 > sk_g0 ? (sk_g1 - 1) / total - sk_t0 + 1 : 0;
    const int n_rr = (int)blockIdx.x < num_items ? (num_items - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int n_work = n_rr + sk_nseg;
    if (n_work == 0)
        return;
    // work item v of this workgroup: rows [m0, m0 + mrows) x columns from n0, chunks [c0, c1); skt = the tail tile of a
    // stream-K run (-1: the item owns its whole K and stores from its accumulators)
    auto decode = [&](int v, int &m0, int &n0, int &mrows, int &c0, int &c1, int &skt) {
        if (v < n_rr) {
            const int it = (int)blockIdx.x + v * (int)gridDim.x;
            const bool part = it >= split_from;
            const int j = it - split_from;
            const int t = part ? split_from + j / split : it;
            mrows = part ? DM / split : DM;
            m0 = (t / tiles_n) * DM + (part ? (j % split) * mrows : 0);
            n0 = (t % tiles_n) * DN;
            c0 = 0, c1 = total, skt = -1;
        } else {
            const int tr = sk_t0 + (v - n_rr), t = split_from + tr;
            mrows = DM;
            m0 = (t / tiles_n) * DM;
            n0 = (t % tiles_n) * DN;
            c0 = max(sk_g0 - tr * total, 0), c1 = min(sk_g1 - tr * total, total);
            skt = (c0 == 0 && c1 == total) ? -1 : tr;
        }
    };

    // issue cursor: runs ahead of the multiply cursor, across item boundaries (its item's origin is decoded once per item:
    // the integer divisions are scalar instructions in front of every wave's next MFMA)
    int iss_v = 0, iss_c = 0, iss_c1 = 0, iss_buf = 0;
    int iss_m0 = 0, iss_n0 = 0, iss_mrows = 0;
    constexpr int DA_PER_ = DM / 8 / DNW;
    // (RC) the issue item's rows for this lane's DA_PER_ DMA instructions and its class's weight matrix
    int irow[DA_PER_];
    const float *iss_w = W;
    auto issue_rows = [&]() {
        if (!RC)
            return;
        // (the cursor as explicit scalars: behind the per-lane loads below the compiler no longer proved it uniform and moved
        // the whole address arithmetic of the chunk issue -- ~100 instructions per chunk -- from the scalar to the vector unit)
        iss_m0 = __builtin_amdgcn_readfirstlane(iss_m0);
        iss_n0 = __builtin_amdgcn_readfirstlane(iss_n0);
        iss_mrows = __builtin_amdgcn_readfirstlane(iss_mrows);
        iss_c = __builtin_amdgcn_readfirstlane(iss_c);
        iss_c1 = __builtin_amdgcn_readfirstlane(iss_c1);
        iss_v = __builtin_amdgcn_readfirstlane(iss_v);
        iss_buf = __builtin_amdgcn_readfirstlane(iss_buf);
#pragma unroll
        for (int i = 0; i < DA_PER_; i++) {
            const int pos = min(iss_m0 + (wave * DA_PER_ + i) * 8 + drow, M - 1);
            irow[i] = max(rc.perm[pos], 0);
        }
        iss_w = W + (size_t)__builtin_amdgcn_readfirstlane(rc.tile_cls[min(iss_m0 / DM, tiles_m - 1)]) * rc.w_stride; // (uniform: a scalar base for the DMA)
        // (consumed HERE: left pending, every use inside the chunk loop would be guarded by s_waitcnt vmcnt(0), which also
        // waits for the chunk DMA in flight -- see the note on the row scalers below)
#pragma unroll
        for (int i = 0; i < DA_PER_; i++)
            asm volatile("" : "+v"(irow[i]));
    };
    {
        int skt_;
        decode(0, iss_m0, iss_n0, iss_mrows, iss_c, iss_c1, skt_);
        issue_rows();
    }
    int vm = 0; // vector-memory instructions this wave has issued (DMA + epilogue stores): for the counted waits
    // The next chunk's DMA goes out in FOUR parts, one per k step of the chunk being multiplied (a burst of eight
    // instructions behind the barrier kept every wave of the workgroup off the matrix pipe at the same moment):
    // issue_begin() resolves the addresses on the scalar unit, issue_part(j) fires part j, issue_end() moves the cursor.
    struct IssueCtx {
        const float *ga, *gw;
        uint32_t la, lw, lda_b, ldw_b;
        int ra_max, rw_max, mrows;
        bool valid;
    };
    auto issue_begin = [&]() -> IssueCtx {
        IssueCtx ic;
        ic.valid = iss_v < n_work;
        if (!ic.valid)
            return ic;
        const int m0 = iss_m0, n0 = iss_n0;
        ic.mrows = iss_mrows;
        const int c = iss_c;
        // segment lookup with static indexing only (keeps the kernarg struct out of scratch)
        const float *ap = g.a[0];
        int lda = g.lda[0], koff = g.koff[0], cbase = 0;
#pragma unroll
        for (int sgm = 1; sgm < 4; sgm++) {
            if (sgm < g.nseg && c >= g.cpre[sgm]) {
                ap = g.a[sgm];
                lda = g.lda[sgm];
                koff = g.koff[sgm];
                cbase = g.cpre[sgm];
            }
        }
        const int kk = (c - cbase) * BK;
        // scalar bases (tile origin, clamped into the matrix) + per-lane 32-bit offsets: the address arithmetic stays
        // on the scalar unit
        const int m0c = min(m0, M - 1), n0c = min(n0, N - 1);
        ic.ga = RC ? ap + kk : ap + (size_t)m0c * lda + kk;
        ic.gw = (RC ? iss_w : W) + (size_t)n0c * ldw + koff + kk;
        ic.ra_max = M - 1 - m0c, ic.rw_max = N - 1 - n0c; // rows past M / N re-read the last valid row (never stored)
        ic.la = smem_a + (uint32_t)iss_buf * DBUF_B, ic.lw = ic.la + DM * BK * 4;
        ic.lda_b = (uint32_t)lda * 4, ic.ldw_b = (uint32_t)ldw * 4;
        if (RC) {
            // (the class lookup sits behind per-lane loads in the cursor's update: the compiler no longer proves the bases
            // uniform -- they are, and the DMA takes them as scalars)
            auto uni = [](const float *p) {
                const uint64_t v = (uint64_t)(uintptr_t)p;
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
                return reinterpret_cast<const float *>((uintptr_t)(((uint64_t)hi << 32) | lo));
            };
            ic.ga = uni(ic.ga);
            ic.gw = uni(ic.gw);
            ic.la = __builtin_amdgcn_readfirstlane(ic.la);
            ic.lw = __builtin_amdgcn_readfirstlane(ic.lw);
        }
        return ic;
    };
    constexpr int DPARTS = BK / 8, DA_PER = DM / 8 / DNW, DW_PER = DN / 8 / DNW; // A / W instructions per wave and chunk
    static_assert(DA_PER <= DPARTS && DW_PER <= DPARTS, "one A and one W instruction per part at most");
    auto issue_part = [&](const IssueCtx &ic, int i) {
        if (!ic.valid)
            return;
        if (i < DA_PER) {
            const int r0 = (wave * DA_PER + i) * 8;
            if (r0 < ic.mrows) {
                dma16_to_lds_s(ic.ga, (uint32_t)(RC ? irow[i < DA_PER_ ? i : 0] : min(r0 + drow, ic.ra_max)) * ic.lda_b + ((r0 & 8) ? dpiece_b1 : dpiece_b0), ic.la + (uint32_t)r0 * 128);
                vm++;
            }
        }
        if (i < DW_PER) {
            const int r0 = (wave * DW_PER + i) * 8;
            dma16_to_lds_s(ic.gw, (uint32_t)min(r0 + drow, ic.rw_max) * ic.ldw_b + ((r0 & 8) ? dpiece_b1 : dpiece_b0), ic.lw + (uint32_t)r0 * 128);
            vm++;
        }
    };
    auto issue_end = [&](const IssueCtx &ic) -> int { // returns vm after the chunk's DMA (its "mark"), -1 when there was none
        if (!ic.valid)
            return -1;
        iss_buf = iss_buf + 1 == DNBUF ? 0 : iss_buf + 1;
        if (++iss_c == iss_c1) {
            if (++iss_v < n_work) {
                int skt_;
                decode(iss_v, iss_m0, iss_n0, iss_mrows, iss_c, iss_c1, skt_);
                issue_rows();
            }
        }
        return vm;
    };
    auto issue_next = [&]() -> int {
        const IssueCtx ic = issue_begin();
#pragma unroll
        for (int i = 0; i < DPARTS; i++)
            issue_part(ic, i);
        return issue_end(ic);
    };

    // marks of the chunks in flight (DNBUF - 1 of them): mk0 = the chunk multiplied next, mk1 = the one after it
    int mk0 = issue_next(), mk1 = DNBUF > 2 ? issue_next() : -1;
    int buf = 0;
    const bool vec = (N % 4 == 0) && (((uintptr_t)Y & 15) == 0) && (bias == nullptr || ((uintptr_t)bias & 15) == 0) &&
                     (skip == nullptr || ((uintptr_t)skip & 15) == 0);

    // one work item with MC 32-row accumulator blocks per wave (2 = whole tile, 1 = a slice, 0 = a wave that only
    // keeps the chunk pipeline going).  A compile-time MC: with a run-time block count the accumulators of the
    // conditional block leave the AGPRs at every loop header.
    auto run_item = [&](auto mtag, auto ntag, int m0, int n0, int rbase, int wcol, int c0, int c1, int skt, int skseg) {
        constexpr int MC = decltype(mtag)::value; // 32-row blocks of the wave
        constexpr int NT = decltype(ntag)::value; // 32-column blocks of the wave, from column `wcol` of the tile
        f32x16 acc[MC > 0 ? MC : 1][NT];
#pragma unroll
        for (int mi = 0; mi < (MC > 0 ? MC : 1); mi++)
#pragma unroll
            for (int ni = 0; ni < NT; ni++)
#pragma unroll
                for (int i = 0; i < 16; i++)
                    acc[mi][ni][i] = 0.0f;

        // (pooling epilogue: the graph ids of the rows of this wave's 32-row blocks -- lane r + 1 holds row r, lanes 0 / 33 the
        // rows just outside --, fetched HERE and consumed below like the scalers: inside the epilogue every block paid a
        // memory round trip for them)
        int gidv[MC > 0 ? MC : 1];
#pragma unroll
        for (int mi = 0; mi < (MC > 0 ? MC : 1); mi++) {
            gidv[mi] = -1;
            if (MC > 0 && POOL) {
                const int r = m0 + rbase + mi * 32 - 1 + lane;
                if (lane < 34 && r >= 0 && r < M)
                    gidv[mi] = pe.node_graph[r];
            }
            // (RC: the row this lane's accumulator block goes to -- the same registers, the two modes exclude each other)
            if (MC > 0 && RC) {
                const int pos = m0 + rbase + mi * 32 + li;
                gidv[mi] = pos < M ? rc.perm[pos] : -1;
            }
        }
        // per-row scalers of the scaled segments (PNA: amp . A, att . A), fetched once per item for the lane's A rows
        float sc[4][MC > 0 ? MC : 1];
        if (MC > 0) {
#pragma unroll
            for (int sgm = 0; sgm < 4; sgm++)
#pragma unroll
                for (int mi = 0; mi < MC; mi++) {
                    const int row = min(m0 + rbase + mi * 32 + li, M - 1);
                    sc[sgm][mi] = (sgm < g.nseg && g.rs[sgm] != nullptr) ? g.rs[sgm][row] : 1.0f;
                }
            // these are loads the compiler tracks: left pending, their first use INSIDE the chunk loop is guarded by
            // s_waitcnt vmcnt(0) in every iteration -- which also waits for the chunk DMA just issued, i.e. serialises
            // "request the next chunk" and "multiply this one" (found in round 2: the kernel had been running that
            // way).  Consumed here, once per item; the chunk loop then has no tracked load in flight.
#pragma unroll
            for (int sgm = 0; sgm < 4; sgm++)
#pragma unroll
                for (int mi = 0; mi < MC; mi++)
                    asm volatile("" : "+v"(sc[sgm][mi]));
#pragma unroll
            for (int mi = 0; mi < MC; mi++)
                asm volatile("" : "+v"(gidv[mi]));
        }

        for (int c = c0; c < c1; c++) {
            // this chunk has landed for this wave when at most the operations issued after it are outstanding (VM
            // operations retire in order; loads the compiler tracks itself only make the wait stricter) ...
            vmcnt_wait_n(min(vm - mk0, 63));
            __syncthreads(); // ... and for everyone; and everyone is done reading the buffer refilled next
            const IssueCtx ic = issue_begin();
            if (MC == 0) {
#pragma unroll
                for (int i = 0; i < DPARTS; i++)
                    issue_part(ic, i);
            }
            const float *a = reinterpret_cast<const float *>(smem + (size_t)buf * DBUF_B);
            const float *b = reinterpret_cast<const float *>(smem + (size_t)buf * DBUF_B + DM * BK * 4);
            buf = buf + 1 == DNBUF ? 0 : buf + 1;
            if (MC > 0) {
                float s[MC > 0 ? MC : 1]; // this chunk's segment (uniform), static indexing
                bool scaled = g.rs[0] != nullptr;
#pragma unroll
                for (int mi = 0; mi < MC; mi++)
                    s[mi] = sc[0][mi];
#pragma unroll
                for (int sgm = 1; sgm < 4; sgm++)
                    if (sgm < g.nseg && c >= g.cpre[sgm]) {
#pragma unroll
                        for (int mi = 0; mi < MC; mi++)
                            s[mi] = sc[sgm][mi];
                        scaled = g.rs[sgm] != nullptr;
                    }
                if (MATH == 2) {
                    // "f16x3" (opt-in, REDUCED precision: math 3): hi + mid fp16 pieces of both operands, three products
                    // (mid.hi, hi.mid, hi.hi) per 16-wide k block -- half the MFMAs and less than half the split work of the
                    // bf16x6 form, ~22 significant bits per product, fp16's range (gnnb_device.h)
#pragma unroll
                    for (int kb2 = 0; kb2 < BK / 16; kb2++) {
                        u32x4 ah[MC > 0 ? MC : 1], am[MC > 0 ? MC : 1], wh[NT], wm[NT];
                        const int piece = 4 * kb2 + 2 * lh;
#pragma unroll
                        for (int mi = 0; mi < MC; mi++) {
                            const int r = rbase + mi * 32 + li;
                            float4 f0 = *reinterpret_cast<const float4 *>(a + r * BK + ((piece ^ dkey(r)) << 2));
                            float4 f1 = *reinterpret_cast<const float4 *>(a + r * BK + (((piece + 1) ^ dkey(r)) << 2));
                            if (scaled) {
                                f0.x *= s[mi], f0.y *= s[mi], f0.z *= s[mi], f0.w *= s[mi];
                                f1.x *= s[mi], f1.y *= s[mi], f1.z *= s[mi], f1.w *= s[mi];
                            }
                            split2x8_f16(f0, f1, ah[mi], am[mi]);
                        }
#pragma unroll
                        for (int ni = 0; ni < NT; ni++) {
                            const int r = wcol + ni * 32 + li;
                            const float4 f0 = *reinterpret_cast<const float4 *>(b + r * BK + ((piece ^ dkey(r)) << 2));
                            const float4 f1 = *reinterpret_cast<const float4 *>(b + r * BK + (((piece + 1) ^ dkey(r)) << 2));
                            split2x8_f16(f0, f1, wh[ni], wm[ni]);
                        }
                        issue_part(ic, 2 * kb2);
                        issue_part(ic, 2 * kb2 + 1);
#define GNNB_DMA_F3(WP, AP)                                                                                        \
    _Pragma("unroll") for (int mi = 0; mi < MC; mi++) _Pragma("unroll") for (int ni = 0; ni < NT; ni++)             \
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_f16x8(WP[ni]), as_f16x8(AP[mi]), acc[mi][ni], 0, 0, 0);
                        GNNB_DMA_F3(wm, ah)
                        GNNB_DMA_F3(wh, am)
                        GNNB_DMA_F3(wh, ah)
#undef GNNB_DMA_F3
                    }
                } else if (MATH) {
                    // lane (li, lh) of a 32x32x16 bf16 MFMA holds k = 8 lh .. + 7 of row / column li for both operands:
                    // two 16-B pieces per fragment and k block
#pragma unroll
                    for (int kb2 = 0; kb2 < BK / 16; kb2++) {
                        u32x4 ah[MC > 0 ? MC : 1], am[MC > 0 ? MC : 1], al[MC > 0 ? MC : 1], wh[NT], wm[NT], wl[NT];
                        const int piece = 4 * kb2 + 2 * lh;
#pragma unroll
                        for (int mi = 0; mi < MC; mi++) {
                            const int r = rbase + mi * 32 + li;
                            float4 f0 = *reinterpret_cast<const float4 *>(a + r * BK + ((piece ^ dkey(r)) << 2));
                            float4 f1 = *reinterpret_cast<const float4 *>(a + r * BK + (((piece + 1) ^ dkey(r)) << 2));
                            if (scaled) {
                                f0.x *= s[mi], f0.y *= s[mi], f0.z *= s[mi], f0.w *= s[mi];
                                f1.x *= s[mi], f1.y *= s[mi], f1.z *= s[mi], f1.w *= s[mi];
                            }
                            split3x8(f0, f1, ah[mi], am[mi], al[mi]);
                        }
#pragma unroll
                        for (int ni = 0; ni < NT; ni++) {
                            const int r = wcol + ni * 32 + li;
                            const float4 f0 = *reinterpret_cast<const float4 *>(b + r * BK + ((piece ^ dkey(r)) << 2));
                            const float4 f1 = *reinterpret_cast<const float4 *>(b + r * BK + (((piece + 1) ^ dkey(r)) << 2));
                            split3x8(f0, f1, wh[ni], wm[ni], wl[ni]);
                        }
                        issue_part(ic, 2 * kb2);
                        issue_part(ic, 2 * kb2 + 1);
                        // six partial products, smallest first; W piece first (swapped operands, float4 epilogue)
#define GNNB_DMA_BF6(WP, AP)                                                                                       \
    _Pragma("unroll") for (int mi = 0; mi < MC; mi++) _Pragma("unroll") for (int ni = 0; ni < NT; ni++)             \
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(WP[ni]), as_bf16x8(AP[mi]), acc[mi][ni], 0, 0, 0);
                        GNNB_DMA_BF6(wm, am)
                        GNNB_DMA_BF6(wh, al)
                        GNNB_DMA_BF6(wl, ah)
                        GNNB_DMA_BF6(wh, am)
                        GNNB_DMA_BF6(wm, ah)
                        GNNB_DMA_BF6(wh, ah)
#undef GNNB_DMA_BF6
                    }
                } else {
                // (requesting the fragments of k step j + 1 before the MFMAs of step j -- two register sets -- was
                // measured: 601 vs 583 us at the C4 shape)
#pragma unroll
                for (int kb = 0; kb < BK; kb += 8) {
                    float4 fa[MC > 0 ? MC : 1], fb[NT];
                    const int piece = (kb >> 2) + lh; // 16-B piece holding k = kb + 4 lh .. + 3
#pragma unroll
                    for (int mi = 0; mi < MC; mi++) {
                        const int r = rbase + mi * 32 + li;
                        fa[mi] = *reinterpret_cast<const float4 *>(a + r * BK + ((piece ^ dkey(r)) << 2));
                    }
                    if (scaled) { // the row scaler multiplies the A operand, as in the register-staged kernel
#pragma unroll
                        for (int mi = 0; mi < MC; mi++)
                            fa[mi].x *= s[mi], fa[mi].y *= s[mi], fa[mi].z *= s[mi], fa[mi].w *= s[mi];
                    }
#pragma unroll
                    for (int ni = 0; ni < NT; ni++) {
                        const int r = wcol + ni * 32 + li;
                        fb[ni] = *reinterpret_cast<const float4 *>(b + r * BK + ((piece ^ dkey(r)) << 2));
                    }
                    issue_part(ic, kb / 8); // (behind this step's fragment reads, in front of its MFMAs)
                    // operands SWAPPED (W fragment first): the 32x32 accumulator then holds, per lane, FOUR
                    // CONSECUTIVE output columns of one row per register group -- the epilogue stores float4
#pragma unroll
                    for (int mi = 0; mi < MC; mi++)
#pragma unroll
                        for (int ni = 0; ni < NT; ni++) {
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ni].x, fa[mi].x, acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ni].y, fa[mi].y, acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ni].z, fa[mi].z, acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[ni].w, fa[mi].w, acc[mi][ni], 0, 0, 0);
                        }
                }
                }
            }
            // the marks move on: mk0 = the chunk multiplied next
            if (DNBUF > 2) {
                mk0 = mk1;
                mk1 = issue_end(ic);
            } else {
                mk0 = issue_end(ic);
            }
        }
        if (MC == 0)
            return;
        // (f16x3: the reduced mode's overflow contract -- what this run of chunks gave, parked stream-K parts included, is looked at
        // before any epilogue; rows past M re-read valid rows.  The atomic, rare, is one more vector-memory instruction: counted)
        if constexpr (MATH == 2) {
            RangeProbe rp;
#pragma unroll
            for (int mi = 0; mi < MC; mi++)
#pragma unroll
                for (int ni = 0; ni < NT; ni++)
                    rp.see_vec<f32x16, 16>(acc[mi][ni]);
            if (rp.any())
                vm += rp.report(err, err_host);
        }

        // ---- pooling epilogue (the model's LAST conv layer): act(acc + bias) is pooled per graph instead of stored.
        // Per 32-row block of the wave: the block goes through an 8-KB scratch in the chunk buffer that was consumed last
        // (free until the next item's first barrier; 16-B chunks XOR-swizzled by the row: conflict-free both ways), then
        // lane c walks column c down the rows IN ORDER with a running sum / max and the rows' graph ids (lane r + 1 of
        // `gid`, read with v_readlane; lanes 0 / 33 hold the rows just outside the block).  A graph that lies inside the
        // block is finished here; a piece of a graph that continues outside goes to part[block][0 = reaches the block's
        // first row, 1 = only its last][column] for launch_pool_combine.  Rows past M carry id -1 and are dropped.
        if constexpr (POOL) {
            auto pool_epi = [&](auto tag) {
                constexpr int ACT = decltype(tag)::value;
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // every wave has read its last fragments
                char *scr = smem + (size_t)((buf + DNBUF - 1) % DNBUF) * DBUF_B + (size_t)wave * 8192;
                const int colg = n0 + wcol + lane; // this lane's column in the row walk
                const bool col_ok = colg < N;
                const bool any_col = __ballot(col_ok) != 0;
#pragma unroll
                for (int mi = 0; mi < MC; mi++) {
                    const int blk0 = m0 + rbase + mi * 32;
                    const int gid = gidv[mi];
#pragma unroll
                    for (int ni = 0; ni < NT; ni++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int cw = ni * 32 + 8 * q + 4 * lh; // column inside the wave's 64
                            const int cg = n0 + wcol + cw;
                            float4 v = make_float4(acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]);
                            if (bias && vec && cg + 3 < N) {
                                const float4 bv = bias_lds ? *reinterpret_cast<const float4 *>(sbias + cg) : *reinterpret_cast<const float4 *>(bias + cg);
                                v.x += bv.x, v.y += bv.y, v.z += bv.z, v.w += bv.w;
                            } else if (bias) {
                                v.x += cg + 0 < N ? bias[cg + 0] : 0.0f;
                                v.y += cg + 1 < N ? bias[cg + 1] : 0.0f;
                                v.z += cg + 2 < N ? bias[cg + 2] : 0.0f;
                                v.w += cg + 3 < N ? bias[cg + 3] : 0.0f;
                            }
                            v.x = act_t<ACT>(v.x), v.y = act_t<ACT>(v.y), v.z = act_t<ACT>(v.z), v.w = act_t<ACT>(v.w);
                            *reinterpret_cast<float4 *>(scr + li * 256 + ((((cw >> 2)) ^ (li & 15)) << 4)) = v;
                        }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // own scratch writes (wave-private region: no barrier)
                    const int blk = blk0 >> 5;
                    float sum = 0.0f, mx = -INFINITY;
                    int cur = __builtin_amdgcn_readlane(gid, 1), nrows = 0;
                    bool open_start = cur >= 0 && __builtin_amdgcn_readlane(gid, 0) == cur;
                    auto flush = [&](int g, int n, bool os, bool oe) { // (g, n, os, oe: wave-uniform)
                        // the stores are COUNTED (wave-uniformly: the instruction issues when any lane has a column): left
                        // uncounted, the first counted wait of the next tile drained them -- a full write round trip per tile
                        // with every wave of the workgroup idle (found in the row-class mode: 341 -> 272 us there)
                        if (g >= 0 && g < pe.num_graphs && any_col)
                            vm += (!os && !oe) ? pe.np : 1;
                        if (g < 0 || g >= pe.num_graphs || !col_ok)
                            return;
                        if (!os && !oe) {
#pragma unroll
                            for (int kk = 0; kk < 3; kk++) {
                                if (kk >= pe.np)
                                    break;
                                float rr = sum;
                                if (pe.pools[kk] == GNNB_POOL_MEAN)
                                    rr = sum / (float)n;
                                else if (pe.pools[kk] == GNNB_POOL_MAX)
                                    rr = mx;
                                pe.pooled[((size_t)g * pe.np + kk) * N + colg] = rr;
                            }
                        } else {
                            pe.part[((size_t)blk * 2 + (os ? 0 : 1)) * N + colg] = make_float2(sum, mx);
                        }
                    };
                    const char *col_p = scr + ((lane & 3) << 2);
                    const int cch = lane >> 2;
#pragma unroll 1
                    for (int r8 = 0; r8 < 32; r8 += 8) { // eight rows per step: their LDS reads go out together
                        float v8[8];
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            v8[i] = *reinterpret_cast<const float *>(col_p + (r8 + i) * 256 + ((cch ^ ((r8 + i) & 15)) << 4));
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const int id = __builtin_amdgcn_readlane(gid, r8 + i + 1);
                            if (id != cur) { // (wave-uniform)
                                flush(cur, nrows, open_start, false);
                                cur = id;
                                sum = 0.0f;
                                mx = -INFINITY;
                                nrows = 0;
                                open_start = false;
                            }
                            sum += v8[i];
                            mx = fmaxf(mx, v8[i]);
                            nrows++;
                        }
                    }
                    flush(cur, nrows, open_start, cur >= 0 && __builtin_amdgcn_readlane(gid, 33) == cur);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the walk's reads are done before the next block's writes
                }
            };
            GNNB_DISPATCH_ACT(act, pool_epi)
            return;
        }

        // ---- stream-K run: park the accumulators; the last workgroup at the tile adds the runs up and goes on to the epilogue.
        // The parts are exchanged between workgroups on DIFFERENT XCDs (one L2 each): stores and loads at agent scope (sc1:
        // write-through / read from the coherent level) and a wait for the stores, instead of a release fence -- which
        // writes back the whole L2 (buffer_wbl2) per wave: measured 655 us against 540 for the row slices at the C4 shape.
        if (MC == 2 && !POOL && skt >= 0) {
            // part layout: [accumulator register 0..63][lane] (256-B rows: every store / load instruction is one contiguous piece)
            float *mine = sk.part + ((size_t)(2 * blockIdx.x + skseg) * 4 + wave) * 4096 + lane;
#pragma unroll
            for (int mi = 0; mi < MC; mi++)
#pragma unroll
                for (int ni = 0; ni < NT; ni++)
#pragma unroll
                    for (int i = 0; i < 16; i++)
                        __hip_atomic_store(mine + ((mi * NT + ni) * 16 + i) * 64, acc[mi][ni][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the parts are at the coherent level before the arrival is counted
            __syncthreads();
            int *flag = reinterpret_cast<int *>(smem + (size_t)DNBUF * DBUF_B);
            const int w_first = (skt * total) / sk.q, w_last = ((skt + 1) * total - 1) / sk.q;
            if (tid == 0)
                *flag = __hip_atomic_fetch_add(sk.cnt + w_first, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            const bool last = *flag == w_last - w_first;
            if (!last)
                return;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); // (buffer_inv: the loads below see the other XCDs' parts)
#pragma unroll
            for (int mi = 0; mi < MC; mi++)
#pragma unroll
                for (int ni = 0; ni < NT; ni++)
#pragma unroll
                    for (int i = 0; i < 16; i++)
                        acc[mi][ni][i] = 0.0f;
            for (int wq = w_first; wq <= w_last; wq++) { // run order = k order
                const int sg = wq * sk.q < skt * total ? 1 : 0; // the tile is that workgroup's second segment when its run began in the tile before
                const float *theirs = sk.part + ((size_t)(2 * wq + sg) * 4 + wave) * 4096 + lane;
#pragma unroll
                for (int mi = 0; mi < MC; mi++)
#pragma unroll
                    for (int ni = 0; ni < NT; ni++)
#pragma unroll
                        for (int i = 0; i < 16; i++)
                            acc[mi][ni][i] += theirs[((mi * NT + ni) * 16 + i) * 64];
            }
            if (tid == 0)
                sk.cnt[w_first] = 0; // (nobody else comes to this tile in this launch; the next launch finds it cleared)
        }

        // D = W_tile . A_tile^T: lane (li, lh) holds Y[row = m_base + li][col = n_base + 8 (reg >> 2) + 4 lh + (reg & 3)]
        // (RC: the bias of the tile's class -- rc.bias_stride floats apart, 0: one bias for all)
        const float *const bias_all = bias;
        [[maybe_unused]] const float *bias = RC && bias_all ? bias_all + (size_t)__builtin_amdgcn_readfirstlane(rc.tile_cls[min(m0 / DM, tiles_m - 1)]) * rc.bias_stride
                                                           : bias_all;
        auto epilogue = [&](auto tag) {
            constexpr int ACT = decltype(tag)::value;
#pragma unroll
            for (int mi = 0; mi < MC; mi++) {
                const int rowg = RC ? gidv[mi] : m0 + rbase + mi * 32 + li;
                if (RC ? rowg < 0 : rowg >= M)
                    continue;
#pragma unroll
                for (int ni = 0; ni < NT; ni++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int colg = n0 + wcol + ni * 32 + 8 * q + 4 * lh;
                        if (vec && colg + 3 < N) {
                            float4 v = make_float4(acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2],
                                                   acc[mi][ni][4 * q + 3]);
                            if (bias) {
                                const float4 bv = bias_lds ? *reinterpret_cast<const float4 *>(sbias + colg) : *reinterpret_cast<const float4 *>(bias + colg);
                                v.x += bv.x, v.y += bv.y, v.z += bv.z, v.w += bv.w;
                            }
                            if (skip) {
                                const float4 sk = *reinterpret_cast<const float4 *>(skip + (size_t)rowg * N + colg);
                                v.x += sk.x, v.y += sk.y, v.z += sk.z, v.w += sk.w;
                            }
                            v.x = act_t<ACT>(v.x), v.y = act_t<ACT>(v.y), v.z = act_t<ACT>(v.z), v.w = act_t<ACT>(v.w);
                            *reinterpret_cast<float4 *>(Y + (size_t)rowg * N + colg) = v;
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; r++)
                                if (colg + r < N) {
                                    float v = acc[mi][ni][4 * q + r] + (bias ? bias[colg + r] : 0.0f);
                                    if (skip)
                                        v += skip[(size_t)rowg * N + colg + r];
                                    Y[(size_t)rowg * N + colg + r] = act_t<ACT>(v);
                                }
                        }
                    }
            }
        };
        GNNB_DISPATCH_ACT(act, epilogue)
        // the stores just issued sit between the prefetched chunk and the next waits: count them, or the first wait
        // of the next item would drain them.  Only blocks that certainly issued all eight 16-B stores are counted (an
        // under-count merely makes the next waits stricter; an over-count would let a wait return early).
        if (vec && n0 + wcol + 32 * NT <= N) {
#pragma unroll
            for (int mi = 0; mi < MC; mi++)
                if (RC ? __ballot(gidv[mi] < 0) == 0 : m0 + rbase + mi * 32 + 32 <= M) // (RC: a block without padding rows)
                    vm += 4 * NT;
        }
    };

    for (int v = 0; v < n_work; v++) {
        int m0, n0, mrows, c0, c1, skt;
        decode(v, m0, n0, mrows, c0, c1, skt);
        // whole tile: 2 x 2 waves of 64 x 64; 64-row slice: 2 x 2 waves of 32 x 64; 32-row slice: 1 x 4 waves of 32 x 32 (round
        // 4 -- it had been 32 x 64 on two of the four waves)
        // N <= 64 (one column tile, no 32-row slices): the same row layouts with 32-column wave tiles
        if constexpr (!POOL) {
            if (N <= 64) {
                if (mrows == DM)
                    run_item(IntTag<2>{}, IntTag<1>{}, m0, n0, wm * 64, wn * 32, c0, c1, skt, v > n_rr ? 1 : 0);
                else
                    run_item(IntTag<1>{}, IntTag<1>{}, m0, n0, wm * 32, wn * 32, c0, c1, -1, 0);
                continue;
            }
        }
        if (mrows == DM)
            run_item(IntTag<2>{}, IntTag<2>{}, m0, n0, wm * 64, wn * 64, c0, c1, skt, v > n_rr ? 1 : 0);
        else if (mrows == DM / 2)
            run_item(IntTag<1>{}, IntTag<2>{}, m0, n0, wm * 32, wn * 64, c0, c1, -1, 0);
        else
            run_item(IntTag<1>{}, IntTag<1>{}, m0, n0, 0, wave * 32, c0, c1, -1, 0);
    }
}

// the pieces of graphs that cross 32-row blocks, added up in block (= row) order; zeros for empty graphs.  Graphs inside
// one block were finished by the GEMM's epilogue and are left alone.
__global__ __launch_bounds__(WG) void k_pool_combine(PoolEpilogue pe, int M, int N)
{
    const int g = blockIdx.x;
    const int g0 = min(max(pe.graph_ptr[g], 0), M), g1 = min(max(pe.graph_ptr[g + 1], g0), M);
    const int n = g1 - g0;
    const int b0 = g0 >> 5, b1 = (g1 - 1) >> 5;
    if (n > 0 && b0 == b1)
        return;
    for (int c = threadIdx.x; c < N; c += WG) {
        float sum = 0.0f, mx = n > 0 ? -INFINITY : 0.0f;
        for (int b = b0; n > 0 && b <= b1; b++) {
            const int slot = b == b0 ? 1 : 0; // (the graph's first block holds its head -- open at the end only --, every later block a piece that reaches the block's first row)
            const float2 p = pe.part[((size_t)b * 2 + slot) * N + c];
            sum += p.x;
            mx = fmaxf(mx, p.y);
        }
        for (int kk = 0; kk < pe.np; kk++) {
            float rr = sum;
            if (pe.pools[kk] == GNNB_POOL_MEAN)
                rr = n > 0 ? sum / (float)n : 0.0f;
            else if (pe.pools[kk] == GNNB_POOL_MAX)
                rr = mx;
            pe.pooled[((size_t)g * pe.np + kk) * N + c] = rr;
        }
    }
}

hipError_t launch_pool_combine(const PoolEpilogue &pe, int M, int N, hipStream_t s)
{
    if (pe.num_graphs <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_pool_combine, dim3(pe.num_graphs), dim3(WG), 0, s, pe, M, N);
    return hipGetLastError();
}

bool linear_dma_eligible(const GemmArgs &g, const float *w, int ldw)
{
    bool plain = options().gemm_dma && (ldw % 4 == 0) && (((uintptr_t)w & 15) == 0);
    for (int sg = 0; sg < g.nseg && plain; sg++)
        plain = g.avec[sg] && g.wvec[sg] && (g.k[sg] % BK == 0) && (g.koff[sg] % 4 == 0);
    return plain;
}

hipError_t launch_linear_dma(const DmaPlan &plan, StreamK sk, const GemmArgs &g, const float *w, int ldw, const float *bias,
                             const float *skip, float *y, int M, int N, int act, hipStream_t s, const PoolEpilogue *pep,
                             const RowClasses *rcp)
{
    const PoolEpilogue pe = pep ? *pep : PoolEpilogue{};
    const RowClasses rc = rcp ? *rcp : RowClasses{};
    const int tm = (M + DM - 1) / DM, tn = (N + DN - 1) / DN;
    const int bias_in_lds = (bias && !rcp && N <= 2048) ? 1 : 0; // (8 KB at most beside the two 64-KB workgroups of a CU)
    const size_t lds = (size_t)DNBUF * DBUF_B + 16 + (bias_in_lds ? (((size_t)N * 4 + 15) & ~(size_t)15) : 0); // (+ the stream-K arrival flag, + the bias)
    const FlagWord flagw = launch_flag_word(); // (the workspace whose forward this launch belongs to; none: stand-alone gnnb_linear)
    sk.q = plan.q;
    hipError_t e = hipSuccess;
    auto go = [&](auto mathtag, auto modetag) {
        auto kern = k_linear_dma<decltype(mathtag)::value, decltype(modetag)::value>;
        e = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess)
            return;
        hipLaunchKernelGGL(kern, dim3(plan.grid), dim3(DWG), lds, s, g, w, ldw, bias, skip, y, M, N, act, tm, tn, plan.split_from,
                           plan.split, pe, sk, rc, bias_in_lds, flagw.err, flagw.err_host);
        e = hipGetLastError();
    };
    auto go_mode = [&](auto mathtag) { // MODE 1: the pooling epilogue, 2: row classes
        if (pep)
            go(mathtag, IntTag<1>{});
        else if (rcp)
            go(mathtag, IntTag<2>{});
        else
            go(mathtag, IntTag<0>{});
    };
    if (launch_math() == 3) // MATH 2 (f16x3: opt-in, reduced precision)
        go_mode(IntTag<2>{});
    else if (launch_math())
        go_mode(IntTag<1>{});
    else
        go_mode(IntTag<0>{});
    return e;
}

} // namespace gnnb
