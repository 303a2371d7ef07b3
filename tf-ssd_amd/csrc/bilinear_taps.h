// The four-tap bilinear arithmetic of tf.image.resize (half-pixel centres, no antialias) that augment_geometry_kernel
// (ssd_data.hip) and augment_mosaic_pixels_kernel (ssd_mosaic.hip) share: one copy, so both are bit-equal to
// oracle/augment_oracle.resize_bilinear.  Every fp32 operation rounds on its own: include only from files compiled with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace ssd {

// Output coordinate `o` of an axis resized from `in_size` to `out_size` samples: the two source samples and the weight of
// the second one.
__device__ __forceinline__ void bilinear_axis(const int o, const int in_size, const int out_size, int& i0, int& i1, float& l) {
    const float scale = (float)in_size / (float)out_size;
    const float f = ((float)o + 0.5f) * scale - 0.5f;
    const float ff = floorf(f);
    i0 = max((int)ff, 0);
    i1 = min((int)ceilf(f), in_size - 1);
    l = f - ff;
}

__device__ __forceinline__ float bilinear_blend(const float tl, const float tr, const float bl, const float br, const float lx,
                                                const float ly) {
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    return top + (bot - top) * ly;
}

}  // namespace ssd
