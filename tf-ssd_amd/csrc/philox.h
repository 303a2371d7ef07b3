// The counter-based generator of the device augmentation (ssd_augplan.hip, ssd_mosaic.hip): Philox4x32-10 and the draw
// conventions of include/ssd_hip.h.  Every draw is a pure function of (seed, sample id, slot).
#pragma once
#include <hip/hip_runtime.h>

namespace ssd {

struct philox4 {
    unsigned int w[4];
};

__device__ __forceinline__ philox4 philox4x32_10(const unsigned int c0, const unsigned int c1, const unsigned int c2,
                                                 const unsigned int c3, unsigned int k0, unsigned int k1) {
    philox4 c = {{c0, c1, c2, c3}};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c.w[0], p1 = 0xCD9E8D57ull * c.w[2];
        const philox4 n = {{(unsigned int)(p1 >> 32) ^ c.w[1] ^ k0, (unsigned int)p1, (unsigned int)(p0 >> 32) ^ c.w[3] ^ k1,
                            (unsigned int)p0}};
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ float draw_unit(const unsigned int word) { return (float)(word >> 8) * 0x1p-24f; }
__device__ __forceinline__ bool draw_bool(const unsigned int word) { return draw_unit(word) > 0.5f; }
__device__ __forceinline__ float draw_uniform(const unsigned int word, const float lo, const float hi) {
    return lo + draw_unit(word) * (hi - lo);
}
__device__ __forceinline__ int draw_below(const unsigned int word, const int n) {
    return (int)(((unsigned long long)word * (unsigned long long)(unsigned int)n) >> 32);
}

}  // namespace ssd
