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

// The Huffman tables of ITU-T T.81 Annex K as a DHT segment gives them, and the sizes that follow from writing them: the
// host coder (ssd_jpeg_enc.hip) and the device coder (ssd_jpeg_pack.hip) derive their code tables from this one copy.
struct std_huff {
    unsigned char cls_id;       // the DHT segment's Tc << 4 | Th
    unsigned char bits[16];
    int count;
    unsigned char vals[162];
};
// in stream order: DC0, AC0, DC1, AC1
static const std_huff kStdHuff[4] = {
    {0x00, {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {0x10, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    {0x01, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {0x11, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}};

// SOI + APP0 + 2 DQT + SOF0 + 4 DHT + SOS
static const size_t kEncHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * (21 + 12) + 2 * (21 + 162) + 14;
// the longest block: an 11-bit DC code + 11 bits, 63 x (a 16-bit AC code + 10 bits) = 1660 bits, every byte stuffed
static const size_t kEncBlockBytes = 2 * ((22 + 63 * 26 + 7) / 8);
// ssd_jpeg_encode_bound for an image of `blocks` emitted blocks: + the padded last byte (stuffed) + EOI
static inline size_t jpeg_encode_bound_bytes(const size_t blocks) { return kEncHeaderBytes + blocks * kEncBlockBytes + 2 + 2; }

}  // namespace ssd
