// gnnb_stack.h -- pieces shared by the LDS-resident conv-stack kernels (k_stack.hip: k_gcn2_fused; k_stack_zf.h: k_gcn2_zf): device
// helpers and the launchers' common host side.  Their carves, plans and capacities (ZF_TCAP, G2_TCAP): gnnb_stack_plan.h
#pragma once
#include "gnnb_device.h"
#include "gnnb_stack_plan.h"

namespace gnnb {

static_assert(16 * g2_units(0) == GNNB_G2_STAGE_ROWS && 16 * g2_units(1) == GNNB_G2_STAGE_ROWS_BF6, "graph prep picks the tile size against these");

// ---- host side: what the two launchers do alike
// the operands both kernels read with vector loads: w1, pooled (and zf's b1, when there is one) at 16 B, x at 4 B
inline bool stack_operands_aligned(const float *x, const float *w1, const float *pooled, const float *b1)
{
    return !((((uintptr_t)w1) & 15) || (((uintptr_t)pooled) & 15) || (((uintptr_t)x) & 3) || (b1 && (((uintptr_t)b1) & 15)));
}
// up to three pooling kinds as kernel arguments (0 past the model's count)
struct StackPools {
    int p0, p1, p2;
    StackPools(const int32_t *pools, int n) : p0(pools[0]), p1(n > 1 ? pools[1] : 0), p2(n > 2 ? pools[2] : 0) {}
};
// the (KQ0, KQ1) instantiations both kernels exist in: input width in one or two 16-wide k blocks x hidden width 128 / 64 / 32
template <class ActTag, class Go>
inline void stack_dispatch_kq(int kq0, int kq1, ActTag atag, Go &&go)
{
    if (kq0 == 1 && kq1 == 8) go(atag, IntTag<1>{}, IntTag<8>{});
    else if (kq0 == 1 && kq1 == 4) go(atag, IntTag<1>{}, IntTag<4>{});
    else if (kq0 == 1 && kq1 == 2) go(atag, IntTag<1>{}, IntTag<2>{});
    else if (kq0 == 2 && kq1 == 8) go(atag, IntTag<2>{}, IntTag<8>{});
    else if (kq0 == 2 && kq1 == 4) go(atag, IntTag<2>{}, IntTag<4>{});
    else go(atag, IntTag<2>{}, IntTag<2>{});
}

struct G2Stage {
    int ta, tb, nb, rows, ga, gb;
};

// Sum / max of a value over the four 16-lane rows of a wave (same lane index in each row) with the
// gfx950 row-swap instructions -- two VALU operations per step instead of an LDS crossbar round trip.
__device__ __forceinline__ float rows4_sum(float x)
{
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float rows4_max(float x)
{
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const float s = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
// Workgroup barrier of the fused kernel: LDS traffic drained, NO vector-memory drain.  __syncthreads()
// carries a fence, for which the compiler emits s_waitcnt vmcnt(0) whenever it has stores of its own in
// flight (the pooled outputs) -- and that would also wait for the untracked DMA of the next stage.
__device__ __forceinline__ void g2_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }


} // namespace gnnb
