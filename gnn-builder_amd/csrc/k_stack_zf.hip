// k_stack_zf.hip -- the instantiations of k_gcn2_zf WITHOUT the MLP-head tail (the default forward) and what graph prep asks
// about the kernel; the kernel and its launcher are in k_stack_zf.h.
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include "k_stack_zf.h"

namespace gnnb {

int zf_stage_rows(int f0) { return zf_stage_rows_of(f0, options().zf_shape); }
long gcn2_zf_tile_capacity(int f0) { return zf_tile_capacity_of(f0, options().zf_shape, device_cu_count()); }

#ifdef GNNB_ZF_ABLATE
// development only: a ring of 256 {min start, max end} slots, one per launch; gnnb_zf_dbg_spans copies them out
static unsigned long long *g_zf_spans = nullptr;
static int g_zf_launches = 0;
unsigned long long *zf_dbg_span_slot()
{
    if (!g_zf_spans)
        return nullptr;
    return g_zf_spans + 2 * (g_zf_launches++ & 255);
}
extern "C" int gnnb_zf_dbg_reset()
{
    if (!g_zf_spans)
        (void)hipMalloc((void **)&g_zf_spans, 256 * 2 * sizeof(unsigned long long));
    unsigned long long init[512];
    for (int i = 0; i < 256; i++) {
        init[2 * i] = ~0ull;
        init[2 * i + 1] = 0ull;
    }
    g_zf_launches = 0;
    (void)hipDeviceSynchronize();
    return (int)hipMemcpy(g_zf_spans, init, sizeof(init), hipMemcpyHostToDevice);
}
extern "C" int gnnb_zf_dbg_spans(unsigned long long *host, int *launches)
{
    *launches = g_zf_launches;
    return g_zf_spans ? (int)hipMemcpy(host, g_zf_spans, 256 * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost) : -1;
}
#endif

hipError_t launch_gcn2_zf(const BatchTables &t, const float *x, int f0, const float *w0, const float *b0,
                          int h0, const float *w1, const float *b1, int h1, int act,
                          const int32_t *pools, int num_pools, float *pooled, hipStream_t s, const float *w1f,
                          const HeadArgs *head_in, const HeadArgs *head_dev_in, float *head_out, bool *head_fused)
{
    return launch_gcn2_zf_impl<false>(t, x, f0, w0, b0, h0, w1, b1, h1, act, pools, num_pools, pooled, s, w1f, head_in, head_dev_in,
                                      head_out, head_fused);
}

} // namespace gnnb
