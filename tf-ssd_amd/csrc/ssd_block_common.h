// Primitives shared by the fused MobileNetV2 block kernels (ssd_fused.hip, ssd_dwproj.hip, ssd_imgblock.hip,
// ssd_imgblock2.hip, ssd_bandblock.hip, ssd_band3.hip) and the LDS-DMA conv tiles (ssd_convdma.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ssd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// destination operand of __builtin_amdgcn_raw_ptr_buffer_load_lds (LDS-DMA)
typedef __attribute__((address_space(3))) void* lds_dst_t;

__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.0f), 6.0f); }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup fence
// over ALL address spaces, and since vmcnt also counts stores on gfx950 the compiler then
// drains every outstanding global load (s_waitcnt vmcnt(0)) at the first LDS access after
// the barrier -- which would stall on the weight / next-tile prefetch and the LDS-DMA copies
// that these kernels deliberately keep in flight across their phases.
__device__ __forceinline__ void lds_barrier() {
    // (an address-space-restricted __builtin_amdgcn_fence(..., "local") still drained vmcnt on
    // ROCm 7.2, hence the explicit LDS-counter wait + raw barrier; "memory" keeps the compiler
    // from moving LDS accesses across it)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Prefetch loads the compiler must not wait for: a 16-byte global load issued through inline
// asm is invisible to hipcc's s_waitcnt bookkeeping, so it stays in flight across the phase
// barriers; wait_prefetch() is the matching hand-placed wait (every destination is passed
// through an empty "+v" statement so no consumer can be scheduled above the wait).  Every
// issued load IS consumed (an unconsumed asm load's destination is dead to the compiler).
__device__ __forceinline__ f32x4 gload16_async(const float* ptr) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(ptr) : "memory");
    return v;
}
template <int N>
__device__ __forceinline__ void wait_prefetch(f32x4 (&r)[N]) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(r[i]));
}

}  // namespace ssd
