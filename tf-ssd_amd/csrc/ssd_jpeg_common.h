// What the JPEG decoder (ssd_jpeg.hip) and encoder (ssd_jpeg_enc.hip) both know about a baseline frame: the zigzag
// order, which samplings are taken, how an image's size and sampling become MCUs, component planes and the coefficient
// storage of struct ssd_jpeg_info, how a block index of that storage maps to a component and a place in its plane, the
// image of a batch that owns an index, and the constants of the "islow" DCT.  One copy, so the two directions cannot drift
// apart.
#pragma once
#include "common.h"

namespace ssd {

static const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// [3P] the 13-bit fixed-point constants of libjpeg's JDCT_ISLOW transforms, FIX(x) = round(x * 2^13), named by x
enum : int {
    kFix0_298631336 = 2446, kFix0_390180644 = 3196, kFix0_541196100 = 4433, kFix0_765366865 = 6270,
    kFix0_899976223 = 7373, kFix1_175875602 = 9633, kFix1_501321110 = 12299, kFix1_847759065 = 15137,
    kFix1_961570560 = 16069, kFix2_053119869 = 16819, kFix2_562915447 = 20995, kFix3_072711026 = 25172,
};

// luma sampling of a three-component frame whose chroma is sampled 1x1: 4:4:4, 4:2:2 and 4:2:0
__host__ __device__ __forceinline__ bool jpeg_sampling_ok(const int hs, const int vs) {
    return (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2);
}

// what an image's size and luma sampling come to: the kernels derive it from a descriptor, the host checks derive the same
struct jpeg_geometry {
    int mcus_x, mcus_y;
    int bw0, bh0;               // blocks per row / column of the luma plane; a chroma plane has mcus_x x mcus_y
    int n0, n1;                 // blocks of the luma plane / of one chroma plane (padded to whole MCUs)
    int nblocks;                // all components
};
__host__ __device__ __forceinline__ jpeg_geometry jpeg_geom(const int H, const int W, const int h_samp, const int v_samp,
                                                            const int components) {
    jpeg_geometry g;
    g.mcus_x = (W + 8 * h_samp - 1) / (8 * h_samp);
    g.mcus_y = (H + 8 * v_samp - 1) / (8 * v_samp);
    g.bw0 = g.mcus_x * h_samp; g.bh0 = g.mcus_y * v_samp;
    g.n1 = g.mcus_x * g.mcus_y;
    g.n0 = g.n1 * h_samp * v_samp;
    g.nblocks = g.n0 + (components == 3 ? 2 * g.n1 : 0);
    return g;
}

// block `local` of an image's storage (Y, Cb, Cr one after the other, each plane row-major in blocks)
struct jpeg_block_place {
    int comp, bw;               // the component and its plane's blocks per row
    int by, bx;
    long plane_at;              // where the component's uint8 plane begins, from the image's plane_offset
};
__host__ __device__ __forceinline__ jpeg_block_place jpeg_block(const jpeg_geometry& g, const int local) {
    jpeg_block_place p;
    p.comp = local < g.n0 ? 0 : (local < g.n0 + g.n1 ? 1 : 2);
    const int inplane = local - (p.comp == 0 ? 0 : (p.comp == 1 ? g.n0 : g.n0 + g.n1));
    p.bw = p.comp == 0 ? g.bw0 : g.mcus_x;
    p.by = inplane / p.bw; p.bx = inplane - p.by * p.bw;
    p.plane_at = p.comp == 0 ? 0L : (long)g.n0 * 64 + (long)(p.comp - 1) * g.n1 * 64;
    return p;
}

// the image whose [start, next start) holds `index`: the last b with start(b) <= index (empty ranges are skipped)
template <typename F>
__device__ __forceinline__ int find_image(const int B, const int index, F start) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start(mid) <= index) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Completes `o`, whose width, height, components, h_samp and v_samp are set, with what follows from them: the MCU and
// block counts and the coefficient storage.  Nothing else is touched (ssd_jpeg_encode's check compares whole structs, so
// the callers start from a zeroed one).
static inline void jpeg_complete_info(ssd_jpeg_info& o) {
    const jpeg_geometry g = jpeg_geom(o.height, o.width, o.h_samp[0], o.v_samp[0], o.components);
    o.mcus_x = g.mcus_x; o.mcus_y = g.mcus_y;
    long long bytes = 0;
    for (int c = 0; c < o.components; ++c) {
        o.blocks_w[c] = o.mcus_x * o.h_samp[c];
        o.blocks_h[c] = o.mcus_y * o.v_samp[c];
        o.coef_offset[c] = bytes;
        bytes += (long long)o.blocks_w[c] * o.blocks_h[c] * 128;
    }
    o.coef_bytes = bytes;
}

}  // namespace ssd
