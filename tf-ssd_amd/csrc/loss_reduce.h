// Deterministic in-workgroup sums shared by the loss kernels (csrc/ssd_loss.hip, csrc/ssd_focal.hip): a wave butterfly,
// then the waves' sums added in wave order by every thread.  The tree is fixed by the workgroup size alone, so a sum's
// bits do not depend on the grid.  `sh` holds WAVES entries of LDS.
#pragma once
#include <hip/hip_runtime.h>

namespace ssd {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// deterministic block sums: per-thread partials (index order), wave butterfly, waves in order
template <int WAVES>
__device__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < WAVES; ++w) t += sh[w];
    return t;
}
template <int WAVES>
__device__ int block_sum_i(int v, int* sh) {
    v = wave_sum_i(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < WAVES; ++w) t += sh[w];
    return t;
}

}  // namespace ssd
