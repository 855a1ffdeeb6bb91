// k_stack_zf_head.hip -- the instantiations of k_gcn2_zf WITH the MLP-head tail (option zf_head: conv stack + pooling + head in one
// launch), as a translation unit of their own: see the note at the top of k_stack_zf.h.
// Part of libgnnb_hip.so (hand-written gfx950 / CDNA4 kernels of the GNNBuilder hot path); wavefront = 64 lanes.
#include "k_stack_zf.h"

namespace gnnb {

// (called by launch_gcn2_zf when the head is to run inside)
hipError_t launch_gcn2_zf_head(const BatchTables &t, const float *x, int f0, const float *w0, const float *b0,
                               int h0, const float *w1, const float *b1, int h1, int act,
                               const int32_t *pools, int num_pools, float *pooled, hipStream_t s, const float *w1f,
                               const HeadArgs *head_in, const HeadArgs *head_dev_in, float *head_out, bool *head_fused)
{
    return launch_gcn2_zf_impl<true>(t, x, f0, w0, b0, h0, w1, b1, h1, act, pools, num_pools, pooled, s, w1f, head_in, head_dev_in,
                                     head_out, head_fused);
}

} // namespace gnnb
