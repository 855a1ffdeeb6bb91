// gemm_launch.hip -- the dense update's host side: launch_linear (which GEMM family, how k_linear_dma's grid is cut) and the
// stream-K scratch.  No kernel is defined here: each family's unit has its own launcher (gnnb_gemm.h).
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path).
#include <vector>

#include "gnnb_gemm.h"

namespace gnnb {

// Stream-K scratch: SK_PART_BYTES of parked accumulators + SK_CNT_INTS arrival counters (zero between launches).  A workspace
// owns its own (stream_k_scratch_create at gnnb_workspace_create, freed with it, handed to launch_linear): forwards of different
// workspaces -- on any streams, eager or replayed from hipGraphs -- never share one.  The standalone gnnb_linear entry has no
// workspace: it takes one scratch per (device, stream) from the map below -- launches on one stream run in order and may share
// it -- allocated at the first GEMM that wants it, and NEVER while the stream is being captured (a captured launch takes the
// row slices: a graph replayed on another stream, or beside an eager launch, must not carry the shared scratch's address).
// (the SK_* limits the planner reads, with their measurements: gnnb_gemm.h)
static constexpr size_t SK_PART_BYTES = (size_t)2 * SK_MAX_WG * DM * DN * sizeof(float);
static constexpr int SK_CNT_INTS = 1024; // the counter of a shared tile is indexed by a workgroup: < grid <= SK_MAX_WG
static_assert(SK_MAX_WG <= SK_CNT_INTS, "one arrival counter per resident workgroup at least");
static constexpr size_t SK_GUARD_BYTES = 4096; // behind the counters: a fixed pattern nothing may touch (stream_k_guard_intact)
static constexpr size_t SK_TAIL_BYTES = (size_t)SK_CNT_INTS * sizeof(int) + SK_GUARD_BYTES;
size_t stream_k_scratch_bytes() { return SK_PART_BYTES + SK_TAIL_BYTES; }
hipError_t stream_k_scratch_init(void *base, hipStream_t s)
{
    char *p = reinterpret_cast<char *>(base);
    hipError_t e = hipMemsetAsync(p + SK_PART_BYTES, 0, (size_t)SK_CNT_INTS * sizeof(int), s);
    if (e == hipSuccess)
        e = hipMemsetAsync(p + SK_PART_BYTES + (size_t)SK_CNT_INTS * sizeof(int), 0xA5, SK_GUARD_BYTES, s);
    return e;
}
hipError_t stream_k_scratch_init_sync(void *base) // (workspace creation: no stream involved)
{
    char *p = reinterpret_cast<char *>(base);
    hipError_t e = hipMemset(p + SK_PART_BYTES, 0, (size_t)SK_CNT_INTS * sizeof(int));
    if (e == hipSuccess)
        e = hipMemset(p + SK_PART_BYTES + (size_t)SK_CNT_INTS * sizeof(int), 0xA5, SK_GUARD_BYTES);
    return e;
}
// 1 = counters all zero (no launch in flight on `s`) and the guard pattern whole, 0 = not, -1 = the read-back failed
static int stream_k_tail_ok(const StreamK &k, hipStream_t s)
{
    std::vector<unsigned char> h(SK_TAIL_BYTES);
    if (hipMemcpyAsync(h.data(), k.cnt, SK_TAIL_BYTES, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return -1;
    for (size_t i = 0; i < SK_TAIL_BYTES; i++)
        if (h[i] != (i < (size_t)SK_CNT_INTS * sizeof(int) ? 0x00 : 0xA5))
            return 0;
    return 1;
}
StreamK stream_k_scratch_at(void *base)
{
    StreamK k;
    k.part = reinterpret_cast<float *>(base);
    k.cnt = reinterpret_cast<int *>(reinterpret_cast<char *>(base) + SK_PART_BYTES);
    return k;
}
static std::mutex g_sk_mu;
static std::map<std::pair<int, hipStream_t>, StreamK> g_sk_have;
int stream_k_guard_intact(const StreamK *owned, hipStream_t s)
{
    if (owned && owned->cnt)
        return stream_k_tail_ok(*owned, s);
    StreamK k;
    {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> lock(g_sk_mu);
        auto it = g_sk_have.find(std::make_pair(dev, s));
        if (it == g_sk_have.end())
            return 1; // (no scratch yet: nothing to damage)
        k = it->second;
    }
    return stream_k_tail_ok(k, s);
}
static bool stream_k_scratch(hipStream_t s, const StreamK *owned, StreamK &out)
{
    if (owned && owned->part && owned->cnt) {
        out = *owned;
        out.q = 0;
        return true;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return false;
    }
    std::map<std::pair<int, hipStream_t>, StreamK> &have = g_sk_have;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_sk_mu);
    auto it = have.find(std::make_pair(dev, s));
    if (it == have.end()) {
        if ((int)have.size() >= SK_MAX_STREAMS)
            return false;
        char *p = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&p), stream_k_scratch_bytes()) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (stream_k_scratch_init(p, s) != hipSuccess) { // (in stream order, in front of the first launch that counts)
            (void)hipGetLastError();
            (void)hipFree(p);
            return false;
        }
        it = have.emplace(std::make_pair(dev, s), stream_k_scratch_at(p)).first;
    }
    out = it->second;
    return true;
}

// refuse -> the small-K families -> k_linear_dma (plan, scratch, launch) -> the generic tiles
hipError_t launch_linear(const GemmArgs &g, const float *w, int ldw, const float *bias,
                         const float *skip, float *y, int M, int N, int act, hipStream_t s, const PoolEpilogue *pep,
                         const RowClasses *rcp, const StreamK *sk_owned)
{
    if (M <= 0 || N <= 0)
        return (pep || rcp) ? hipErrorNotSupported : hipSuccess;
    if (rcp && (pep || !rcp->perm || !rcp->tile_cls || M % DM != 0 || N <= 32))
        return hipErrorNotSupported; // (row classes: whole 128-row tiles, k_linear_dma or the generic kernel)
    static_assert(DM == BM, "a row-class tile is one workgroup tile of either kernel");
    if (!pep && !rcp) {
        if (linear_wlds_eligible(g, w, ldw, bias, skip, y, N))
            return launch_linear_wlds(g, w, ldw, bias, skip, y, M, N, act, s);
        if (linear_reg_eligible(g))
            return launch_linear_reg(g, w, ldw, bias, skip, y, M, N, act, s);
    } else if (pep && (skip != nullptr || linear_wlds_eligible(g, w, ldw, bias, skip, y, N) || linear_reg_eligible(g))) {
        return hipErrorNotSupported; // (the pooling epilogue exists in k_linear_dma: the large-K segmented GEMM)
    }
    // (N in 33 .. 64 -- the last layer of the reference's benchmark models, 128 -> 64 -- takes the same kernel with 32-column
    // wave tiles, when K is large enough to be worth the chunk pipeline: it ran in k_linear<1> at 0.20 of peak, a quarter of
    // the ref6 PNA step)
    const int total = g.cpre[g.nseg];
    const bool dma_narrow = N > 32 && N <= 64 && !pep && total >= 8;
    if ((N > 64 || dma_narrow) && linear_dma_eligible(g, w, ldw)) {
        const int tm = (M + DM - 1) / DM, tn = (N + DN - 1) / DN, cus = device_cu_count(), tail_split = (int)options().gemm_tail_split;
        DmaPlan plan = plan_linear_dma(tm, tn, total, cus, tail_split, pep != nullptr, dma_narrow, true);
        StreamK sk;
        if (plan.wants_scratch && !stream_k_scratch(s, sk_owned, sk))
            plan = plan_linear_dma(tm, tn, total, cus, tail_split, pep != nullptr, dma_narrow, false);
        return launch_linear_dma(plan, sk, g, w, ldw, bias, skip, y, M, N, act, s, pep, rcp);
    }
    if (pep)
        return hipErrorNotSupported;
    return launch_linear_tiles(g, w, ldw, bias, skip, y, M, N, act, s, rcp);
}

} // namespace gnnb
