// Baseline JPEG encoding, the mirror image of ssd_jpeg.hip, split at the same place ("JPEG encoding"):
//   device ssd_jpeg_forward: RGB -> YCbCr + chroma downsampling (kernel 1, uint8 component planes in the workspace), then
//          8x8 forward DCT + quantisation (kernel 2, int16 coefficients in the storage layout of struct ssd_jpeg_info).
//          Integer arithmetic with one defined answer: [3P] libjpeg-turbo's 16-bit fixed-point colour conversion, its
//          h2v1 / h2v2 box downsampling with alternating bias, the JDCT_ISLOW forward DCT and the baseline quantiser,
//          restated from the published algorithms (include/ssd_hip.h spells the arithmetic out).
//   host   ssd_jpeg_quality_tables / ssd_jpeg_encode_info / ssd_jpeg_encode_bound / ssd_jpeg_encode_header /
//          ssd_jpeg_entropy_encode: the header and Huffman coding -- serial, bit-granular.  Plain C++: no HIP call, no global state, thread-safe (the data pool's
//          threads call them in parallel).
#include <cstring>

#include "ssd_jpeg_common.h"

namespace ssd {

// ---------------------------------------------------------------------------------------------------------------------
// host: tables of ITU-T T.81 Annex K

static const unsigned char kStdQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct enc_huff {
    unsigned short code[256];
    unsigned char len[256];     // 0: the symbol has no code
};

static void enc_build_huff(enc_huff& t, const std_huff& s) {
    memset(&t, 0, sizeof(t));
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i, ++k, ++code) {
            t.code[s.vals[k]] = (unsigned short)code;
            t.len[s.vals[k]] = (unsigned char)len;
        }
        code <<= 1;
    }
}

// what an H x W image with h x v luma sampling looks like as a struct ssd_jpeg_info (ssd_jpeg_parse fills in the same)
static int enc_fill_info(const int width, const int height, const int hs, const int vs, ssd_jpeg_info& o) {
    memset(&o, 0, sizeof(o));
    SSD_UNSUPPORTED_IF(!image_side_ok(width) || !image_side_ok(height), "ssd_jpeg_encode: %d x %d, outside 1..%d", height, width,
                       kMaxImageSide);
    SSD_UNSUPPORTED_IF(!jpeg_sampling_ok(hs, vs), "ssd_jpeg_encode: luma sampling %dx%d (1x1, 2x1 and 2x2 only)", hs, vs);
    o.width = width; o.height = height; o.components = 3;
    for (int c = 0; c < 3; ++c) { o.h_samp[c] = c ? 1 : hs; o.v_samp[c] = c ? 1 : vs; o.quant_index[c] = c ? 1 : 0; }
    jpeg_complete_info(o);
    return SSD_OK;
}

// `info` is what enc_fill_info makes of its own size and sampling, with baseline tables (1..255, chroma shared)
static int enc_check_info(const ssd_jpeg_info* info) {
    SSD_CHECK_ARG(info, "ssd_jpeg_encode: NULL pointer");
    ssd_jpeg_info want;
    const int rc = enc_fill_info(info->width, info->height, info->h_samp[0], info->v_samp[0], want);
    if (rc != SSD_OK) return rc == SSD_E_UNSUPPORTED ? SSD_E_INVALID : rc;
    memcpy(want.quant, info->quant, sizeof(want.quant));
    SSD_CHECK_ARG(memcmp(&want, info, sizeof(want)) == 0, "ssd_jpeg_encode: info is inconsistent (not what ssd_jpeg_encode_info fills in)");
    SSD_CHECK_ARG(memcmp(info->quant[1], info->quant[2], 128) == 0, "ssd_jpeg_encode: Cb and Cr do not share a quantisation table");
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i)
            SSD_CHECK_ARG(info->quant[c][i] >= 1 && info->quant[c][i] <= 255, "ssd_jpeg_encode: quantisation value %d outside 1..255",
                          info->quant[c][i]);
    return SSD_OK;
}

// Bytes into [out, out + n): past the end nothing is written, the count goes on (the caller compares it with n).
struct byte_writer {
    unsigned char* out;
    size_t n, at;
    unsigned long long acc;     // the low `bits` bits are not yet written
    int bits;

    inline void byte(const unsigned b) {
        if (at < n) out[at] = (unsigned char)b;
        ++at;
    }
    inline void be16(const unsigned v) { byte(v >> 8); byte(v & 255); }
    // len <= 16 bits of entropy-coded data, with byte stuffing
    inline void put(const unsigned code, const int len) {
        acc = (acc << len) | code;
        bits += len;
        while (bits >= 8) {
            const unsigned b = (unsigned)(acc >> (bits - 8)) & 255;
            byte(b);
            if (b == 0xFF) byte(0);
            bits -= 8;
        }
    }
};

static inline int enc_category(const int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// one block: the DC difference against `pred`, then run-length / category coding of the AC terms in zigzag order
static int enc_block(byte_writer& w, const enc_huff& dc, const enc_huff& ac, const short* coef, const bool dummy, int& pred) {
    const int v0 = dummy ? pred : coef[0];
    const int diff = v0 - pred;
    pred = v0;
    int s = enc_category(diff);
    SSD_CHECK_ARG(s <= 11, "ssd_jpeg_entropy_encode: a DC difference of %d is outside the baseline range", diff);
    w.put(dc.code[s], dc.len[s]);
    if (s) w.put((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
    if (dummy) {
        w.put(ac.code[0], ac.len[0]);
        return SSD_OK;
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = coef[kZigzag[k]];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) w.put(ac.code[0xF0], ac.len[0xF0]);
        s = enc_category(v);
        SSD_CHECK_ARG(s <= 10, "ssd_jpeg_entropy_encode: an AC coefficient of %d is outside the baseline range", v);
        const int rs = (run << 4) | s;
        w.put(ac.code[rs], ac.len[rs]);
        w.put((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
        run = 0;
    }
    if (run) w.put(ac.code[0], ac.len[0]);
    return SSD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// device

__host__ __device__ __forceinline__ jpeg_geometry jpeg_geom(const ssd_jpeg_enc_desc& d) {
    return jpeg_geom(d.H, d.W, d.h_samp, d.v_samp, 3);
}

__device__ __forceinline__ void enc_store(unsigned char* p, const unsigned (&w)[1]) { *reinterpret_cast<unsigned*>(p) = w[0]; }
__device__ __forceinline__ void enc_store(unsigned char* p, const unsigned (&w)[2]) { *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]); }

// One item of kernel 1: four chroma samples of chroma row cy (columns 4 ix ..) and the 4 HS x VS luma samples above them.
// Edges as the library handles them: the last real column is replicated to the right; the last real row is replicated
// only up to a whole row group, and below that the last DOWNSAMPLED row is repeated (chroma row ch - 1, luma row H - 1).
template <int HS, int VS>
__device__ __forceinline__ void enc_color_item(const unsigned char* __restrict__ src, const ssd_jpeg_enc_desc& d,
                                               const jpeg_geometry& g, const int cy, const int ix, unsigned char* __restrict__ py) {
    constexpr int NX = 4 * HS;
    const int ch = (d.H + VS - 1) / VS;
    const bool below = cy > ch - 1;
    const int cy_eff = below ? ch - 1 : cy;
    const int x0 = ix * NX;
    unsigned yw[VS][HS];
    int cb[NX], cr[NX];
#pragma unroll
    for (int j = 0; j < VS; ++j) {
        const int r = min(VS * cy_eff + j, d.H - 1);
        const unsigned char* row = src + (long)r * d.W * 3;
#pragma unroll
        for (int k = 0; k < HS; ++k) yw[j][k] = 0;
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            const unsigned char* p = row + min(x0 + k, d.W - 1) * 3;
            const int R = p[0], G = p[1], B = p[2];
            const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            const int Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            const int Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            yw[j][k >> 2] |= (unsigned)Y << (8 * (k & 3));
            cb[k] = j ? cb[k] + Cb : Cb;
            cr[k] = j ? cr[k] + Cr : Cr;
        }
    }
    const int ypitch = g.mcus_x * 8 * HS, cpitch = g.mcus_x * 8;
#pragma unroll
    for (int j = 0; j < VS; ++j)
        enc_store(py + (long)(VS * cy + j) * ypitch + x0, below ? yw[VS - 1] : yw[j]);
    unsigned wb = 0, wr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int b, r;
        if (HS == 1) { b = cb[i]; r = cr[i]; }
        else if (VS == 1) { b = (cb[2 * i] + cb[2 * i + 1] + (i & 1)) >> 1; r = (cr[2 * i] + cr[2 * i + 1] + (i & 1)) >> 1; }
        else { b = (cb[2 * i] + cb[2 * i + 1] + 1 + (i & 1)) >> 2; r = (cr[2 * i] + cr[2 * i + 1] + 1 + (i & 1)) >> 2; }
        wb |= (unsigned)b << (8 * i);
        wr |= (unsigned)r << (8 * i);
    }
    unsigned char* pcb = py + (long)g.n0 * 64 + (long)cy * cpitch + ix * 4;
    *reinterpret_cast<unsigned*>(pcb) = wb;
    *reinterpret_cast<unsigned*>(pcb + (long)g.n1 * 64) = wr;
}

// Kernel 1: colour conversion + downsampling into the uint8 component planes (Y, Cb, Cr one after the other at
// desc[b].plane_offset, each padded to whole MCUs).  One index space of items over the whole batch (desc[b].item_start is
// the prefix); every pixel is read once, every plane byte is written once, with aligned 4- and 8-byte stores.
__global__ __launch_bounds__(256) void jpeg_enc_color_kernel(const unsigned char* __restrict__ rgb,
                                                            const ssd_jpeg_enc_desc* __restrict__ desc, const int B,
                                                            const int total_items, unsigned char* __restrict__ planes) {
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= total_items) return;
    const int b = find_image(B, item, [&](const int i) { return desc[i].item_start; });
    const ssd_jpeg_enc_desc d = desc[b];
    const jpeg_geometry g = jpeg_geom(d);
    const int local = item - d.item_start;
    const int per_row = g.mcus_x * 2;
    const int cy = local / per_row, ix = local - cy * per_row;
    const unsigned char* src = rgb + d.src_offset;
    unsigned char* py = planes + d.plane_offset;
    if (d.h_samp == 1) enc_color_item<1, 1>(src, d, g, cy, ix, py);
    else if (d.v_samp == 1) enc_color_item<2, 1>(src, d, g, cy, ix, py);
    else enc_color_item<2, 2>(src, d, g, cy, ix, py);
}

// one 8-point pass of the "islow" forward DCT: 13-bit constants, int32.  FIRST (rows): the DC terms are << 2, the others
// descaled by 11 bits; second (columns): (v + 2) >> 2 and 15 bits; each descale is (v + 2^(n-1)) >> n.
template <bool FIRST>
__host__ __device__ __forceinline__ void fdct_islow_1d(const int d[8], int out[8]) {
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int n = FIRST ? 11 : 15, half = 1 << (n - 1);
    if (FIRST) { out[0] = (tmp10 + tmp11) << 2; out[4] = (tmp10 - tmp11) << 2; }
    else { out[0] = (tmp10 + tmp11 + 2) >> 2; out[4] = (tmp10 - tmp11 + 2) >> 2; }
    int z1 = (tmp12 + tmp13) * kFix0_541196100;
    out[2] = (z1 + tmp13 * kFix0_765366865 + half) >> n;
    out[6] = (z1 - tmp12 * kFix1_847759065 + half) >> n;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * kFix1_175875602;
    tmp4 *= kFix0_298631336; tmp5 *= kFix2_053119869; tmp6 *= kFix3_072711026; tmp7 *= kFix1_501321110;
    z1 *= -kFix0_899976223; z2 *= -kFix2_562915447; z3 = z3 * -kFix1_961570560 + z5; z4 = z4 * -kFix0_390180644 + z5;
    out[7] = (tmp4 + z1 + z3 + half) >> n;
    out[5] = (tmp5 + z2 + z4 + half) >> n;
    out[3] = (tmp6 + z2 + z3 + half) >> n;
    out[1] = (tmp7 + z1 + z4 + half) >> n;
}

// Kernel 2: forward DCT + quantisation.  One index space of 8x8 blocks over the whole batch (desc[b].block_start is the
// prefix; every block of the padded planes, so the storage holds no stale byte), 8 lanes per block, 32 blocks per
// workgroup.  Lane j loads row j of the block with one aligned 8-byte load and runs the row pass; the 8x8 int32
// intermediate is transposed through LDS (rows padded to 9 words); lane j runs column j and quantises it with a true
// integer division; a second transpose gives lane j the eight coefficients of row j: one aligned 16-byte store.
__global__ __launch_bounds__(256) void jpeg_enc_fdct_kernel(const unsigned char* __restrict__ planes,
                                                           const unsigned char* __restrict__ tables,
                                                           const ssd_jpeg_enc_desc* __restrict__ desc, const int B,
                                                           const int total_blocks, unsigned char* __restrict__ coef) {
    __shared__ int ws[32][8][9];
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int blk = blockIdx.x * 32 + slot;
    const bool live = blk < total_blocks;
    ssd_jpeg_enc_desc d;
    int local = 0, comp = 0;
    if (live) {
        const int b = find_image(B, blk, [&](const int i) { return desc[i].block_start; });
        d = desc[b];
        local = blk - d.block_start;
        const jpeg_block_place p = jpeg_block(jpeg_geom(d), local);
        comp = p.comp;
        const uint2 s = *reinterpret_cast<const uint2*>(planes + (d.plane_offset + p.plane_at) + ((long)(p.by * 8 + j) * p.bw + p.bx) * 8);
        int in[8], out[8];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            in[c] = (int)((s.x >> (8 * c)) & 255) - 128;
            in[c + 4] = (int)((s.y >> (8 * c)) & 255) - 128;
        }
        fdct_islow_1d<true>(in, out);
#pragma unroll
        for (int c = 0; c < 8; ++c) ws[slot][j][c] = out[c];
    }
    __syncthreads();
    int q[8];
    if (live) {
        const unsigned short* qt = reinterpret_cast<const unsigned short*>(tables + d.quant_offset) + (comp ? 64 : 0);
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws[slot][r][j];
        fdct_islow_1d<false>(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int q8 = (int)qt[r * 8 + j] * 8;
            const int a = (abs(out[r]) + (q8 >> 1)) / q8;
            q[r] = out[r] < 0 ? -a : a;
        }
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[slot][r][j] = q[r];
    }
    __syncthreads();
    if (live) {
        unsigned w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            w[c] = ((unsigned)ws[slot][j][2 * c] & 0xFFFFu) | ((unsigned)ws[slot][j][2 * c + 1] << 16);
        *reinterpret_cast<uint4*>(coef + d.coef_offset + (long)local * 128 + j * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

static inline bool enc_desc_shape_ok(const ssd_jpeg_enc_desc& d) { return image_side_ok(d.H) && image_side_ok(d.W); }

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_jpeg_quality_tables(int quality, unsigned short* out) {
    SSD_CHECK_ARG(out, "ssd_jpeg_quality_tables: NULL pointer");
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (kStdQuant[t][i] * scale + 50) / 100;
            out[t * 64 + i] = (unsigned short)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return SSD_OK;
}

extern "C" int ssd_jpeg_encode_info(int width, int height, int h_samp, int v_samp, const unsigned short* tables,
                                    struct ssd_jpeg_info* out) {
    SSD_CHECK_ARG(tables && out, "ssd_jpeg_encode_info: NULL pointer");
    ssd_jpeg_info o;
    const int rc = enc_fill_info(width, height, h_samp, v_samp, o);
    if (rc != SSD_OK) return rc;
    for (int c = 0; c < 3; ++c) memcpy(o.quant[c], tables + (c ? 64 : 0), 128);
    memcpy(out, &o, sizeof(o));
    return enc_check_info(out);
}

extern "C" size_t ssd_jpeg_encode_bound(const struct ssd_jpeg_info* info) {
    if (enc_check_info(info) != SSD_OK) return 0;
    const size_t blocks = (size_t)info->mcus_x * info->mcus_y * (size_t)(info->h_samp[0] * info->v_samp[0] + 2);
    return jpeg_encode_bound_bytes(blocks);
}

// SOI through SOS into `w`: kEncHeaderBytes bytes, whatever the image (`o` has passed enc_check_info)
static void enc_header(byte_writer& w, const ssd_jpeg_info& o) {
    w.be16(0xFFD8);
    static const unsigned char app0[16] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1};
    for (int i = 0; i < 16; ++i) w.byte(app0[i]);
    w.be16(0);                                                                     // no thumbnail
    for (int t = 0; t < 2; ++t) {
        w.be16(0xFFDB); w.be16(67); w.byte((unsigned)t);
        for (int i = 0; i < 64; ++i) w.byte(o.quant[t][kZigzag[i]]);
    }
    w.be16(0xFFC0); w.be16(17); w.byte(8); w.be16((unsigned)o.height); w.be16((unsigned)o.width); w.byte(3);
    for (int c = 0; c < 3; ++c) { w.byte((unsigned)c + 1); w.byte((unsigned)((o.h_samp[c] << 4) | o.v_samp[c])); w.byte((unsigned)o.quant_index[c]); }
    for (int t = 0; t < 4; ++t) {
        const std_huff& s = kStdHuff[t];
        w.be16(0xFFC4); w.be16((unsigned)(19 + s.count)); w.byte(s.cls_id);
        for (int i = 0; i < 16; ++i) w.byte(s.bits[i]);
        for (int i = 0; i < s.count; ++i) w.byte(s.vals[i]);
    }
    static const unsigned char sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int i = 0; i < 14; ++i) w.byte(sos[i]);
}

extern "C" int ssd_jpeg_encode_header(const struct ssd_jpeg_info* info, unsigned char* out, size_t out_bytes, size_t* written) {
    static_assert(kEncHeaderBytes == SSD_JPEG_HEADER_BYTES, "the header's size is part of the interface");
    SSD_CHECK_ARG(out && written, "ssd_jpeg_encode_header: NULL pointer");
    *written = 0;
    const int rc = enc_check_info(info);
    if (rc != SSD_OK) return rc;
    SSD_CHECK_ARG(out_bytes >= kEncHeaderBytes, "ssd_jpeg_encode_header: out holds %zu bytes, fewer than the header's %zu", out_bytes,
                  kEncHeaderBytes);
    byte_writer w = {out, out_bytes, 0, 0, 0};
    enc_header(w, *info);
    *written = w.at;
    return SSD_OK;
}

extern "C" int ssd_jpeg_entropy_encode(const short* coef, const struct ssd_jpeg_info* info, unsigned char* out, size_t out_bytes,
                                       size_t* written) {
    SSD_CHECK_ARG(coef && out && written, "ssd_jpeg_entropy_encode: NULL pointer");
    *written = 0;
    const int rc = enc_check_info(info);
    if (rc != SSD_OK) return rc;
    const ssd_jpeg_info& o = *info;
    SSD_CHECK_ARG(out_bytes >= kEncHeaderBytes + 2, "ssd_jpeg_entropy_encode: out holds %zu bytes, fewer than the header", out_bytes);
    byte_writer w = {out, out_bytes, 0, 0, 0};
    enc_header(w, o);
    enc_huff huff[4];
    for (int t = 0; t < 4; ++t) enc_build_huff(huff[t], kStdHuff[t]);
    // the real blocks of each component: what the frame header's size gives; the rest of an MCU is synthesised
    int real_w[3], real_h[3];
    for (int c = 0; c < 3; ++c) {
        real_w[c] = ((o.width * o.h_samp[c] + o.h_samp[0] - 1) / o.h_samp[0] + 7) / 8;
        real_h[c] = ((o.height * o.v_samp[c] + o.v_samp[0] - 1) / o.v_samp[0] + 7) / 8;
    }
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < o.mcus_y; ++my)
        for (int mx = 0; mx < o.mcus_x; ++mx) {
            if (w.at > w.n) break;                                                 // already too small: stop early
            for (int c = 0; c < 3; ++c)
                for (int v = 0; v < o.v_samp[c]; ++v)
                    for (int u = 0; u < o.h_samp[c]; ++u) {
                        const int by = my * o.v_samp[c] + v, bx = mx * o.h_samp[c] + u;
                        const bool dummy = by >= real_h[c] || bx >= real_w[c];     // AC zero, the DC of the block before it
                        const short* block = coef + o.coef_offset[c] / 2 + ((long)by * o.blocks_w[c] + bx) * 64;
                        const int r = enc_block(w, huff[c ? 2 : 0], huff[c ? 3 : 1], block, dummy, pred[c]);
                        if (r != SSD_OK) return r;
                    }
        }
    if (w.bits) w.put((1u << (8 - w.bits)) - 1, 8 - w.bits);                       // the last byte padded with 1-bits
    w.be16(0xFFD9);
    SSD_CHECK_ARG(w.at <= w.n, "ssd_jpeg_entropy_encode: out holds %zu bytes, the stream needs more", out_bytes);
    *written = w.at;
    return SSD_OK;
}

extern "C" size_t ssd_jpeg_forward_workspace_bytes(const struct ssd_jpeg_enc_desc* desc_host, int B) {
    if (!desc_host || B <= 0) return 0;
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_enc_desc& d = desc_host[b];
        if (enc_desc_shape_ok(d) && jpeg_sampling_ok(d.h_samp, d.v_samp)) total += align_up((size_t)jpeg_geom(d).nblocks * 64, 16);
    }
    return total;
}

extern "C" int ssd_jpeg_forward(const unsigned char* rgb_dev, size_t rgb_bytes, const unsigned char* tables_dev, size_t tables_bytes,
                                const struct ssd_jpeg_enc_desc* desc_host, const struct ssd_jpeg_enc_desc* desc_dev, int B,
                                short* coef_dev, size_t coef_bytes, void* workspace_dev, size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_jpeg_forward: bad batch");
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_jpeg_forward: B = %d (at most 65535)", B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(rgb_dev && tables_dev && desc_host && desc_dev && coef_dev && workspace_dev, "ssd_jpeg_forward: NULL pointer");
    SSD_CHECK_ARG((((size_t)tables_dev | (size_t)coef_dev | (size_t)workspace_dev) & 15) == 0, "ssd_jpeg_forward: a buffer is not 16-byte aligned");
    long blocks = 0, items = 0;
    size_t plane_end = 0, coef_end = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_enc_desc& d = desc_host[b];
        SSD_UNSUPPORTED_IF(!enc_desc_shape_ok(d), "ssd_jpeg_forward: image %d is %d x %d, outside 1..%d", b, d.H, d.W, kMaxImageSide);
        SSD_UNSUPPORTED_IF(!jpeg_sampling_ok(d.h_samp, d.v_samp), "ssd_jpeg_forward: image %d: luma sampling %dx%d (1x1, 2x1 and 2x2 only)", b, d.h_samp, d.v_samp);
        const jpeg_geometry g = jpeg_geom(d);
        const size_t nb = (size_t)g.nblocks;
        SSD_CHECK_ARG(region_ok(d.src_offset, (size_t)d.H * d.W * 3, rgb_bytes, 1), "ssd_jpeg_forward: image %d lies outside rgb_dev", b);
        SSD_CHECK_ARG(region_ok(d.coef_offset, nb * 128, coef_bytes, 16, &coef_end),
                      "ssd_jpeg_forward: image %d: coefficients outside coef_dev, misaligned or overlapping", b);
        SSD_CHECK_ARG(region_ok(d.quant_offset, 256, tables_bytes, 16),
                      "ssd_jpeg_forward: image %d: quantisation tables outside tables_dev or misaligned", b);
        SSD_CHECK_ARG(region_ok(d.plane_offset, nb * 64, workspace_bytes, 16, &plane_end),
                      "ssd_jpeg_forward: image %d: planes outside the workspace, misaligned or overlapping", b);
        SSD_CHECK_ARG(d.block_start == blocks && d.item_start == items, "ssd_jpeg_forward: image %d: block_start / item_start are not the running sums", b);
        blocks += (long)nb;
        items += g.n1 * 16;                                                   // four chroma samples each: 2 per MCU and row, 8 rows
        SSD_UNSUPPORTED_IF(blocks >= (1L << 31) - 64 || items >= (1L << 31) - 512, "ssd_jpeg_forward: the batch is too large for one call (image %d)", b);
    }
    hipLaunchKernelGGL(jpeg_enc_color_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rgb_dev,
                       desc_dev, B, (int)items, (unsigned char*)workspace_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)workspace_dev, tables_dev, desc_dev, B, (int)blocks, (unsigned char*)coef_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
