// Baseline JPEG decoding, split where the work changes character ("JPEG decoding"):
//   host   ssd_jpeg_parse / ssd_jpeg_entropy_decode: marker walk and Huffman decoding -- serial, bit-granular, branchy.
//          Plain C++: no HIP call, no global state, thread-safe (the data pool's threads call them in parallel).
//   device ssd_jpeg_decode: dequantisation + 8x8 inverse DCT (kernel 1, uint8 component planes in the workspace), then
//          chroma upsampling + YCbCr -> RGB (kernel 2, packed uint8 [H,W,3] images).  Integer arithmetic with one defined
//          answer: [3P] libjpeg-turbo's JDCT_ISLOW inverse DCT, "fancy" triangle upsampling and 16-bit fixed-point colour
//          conversion, restated from the published algorithms (include/ssd_hip.h spells the arithmetic out).
// Compiled with -ffp-contract=off like ssd_data.hip (no float is involved) and -fwrapv: coefficients of a hostile file may
// wrap int32 in the IDCT; wrapping is then the defined behaviour, as on the hardware.
#include <cstring>
#include <vector>

#include "ssd_jpeg_huff.h"

namespace ssd {

// ---------------------------------------------------------------------------------------------------------------------
// host: header

struct huff_table {
    bool defined;
    unsigned short look[256];   // (length << 8) | symbol for codes of at most 8 bits, 0: longer
    int maxcode[17];            // largest code of each length, -1: none
    int valoff[17];             // index of the first symbol of that length minus its first code
    unsigned char vals[256];
};

struct jpeg_header {
    ssd_jpeg_info info;
    bool quant_defined[4];
    unsigned short quant[4][64];
    huff_table dc[4], ac[4];
    int dc_sel[3], ac_sel[3];
    size_t scan_at;             // first byte of the entropy-coded segment
};

static int build_huff(huff_table& t, const unsigned char* counts, const unsigned char* symbols, const int total) {
    memset(t.look, 0, sizeof(t.look));
    memcpy(t.vals, symbols, (size_t)total);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int c = counts[len - 1];
        t.valoff[len] = k - code;
        if (c == 0) {
            t.maxcode[len] = -1;
        } else {
            if (code + c > (1 << len)) return SSD_E_INVALID;                       // the codes do not fit the length
            if (len <= 8)
                for (int i = 0; i < c; ++i) {
                    const int first = (code + i) << (8 - len);
                    for (int f = 0; f < (1 << (8 - len)); ++f) t.look[first + f] = (unsigned short)((len << 8) | symbols[k + i]);
                }
            t.maxcode[len] = code + c - 1;
        }
        code = (code + c) << 1;
        k += c;
    }
    t.defined = true;
    return SSD_OK;
}

static inline int be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

static int parse_header(const unsigned char* data, const size_t n, jpeg_header& h) {
    memset(&h, 0, sizeof(h));
    SSD_CHECK_ARG(data && n >= 4 && data[0] == 0xFF && data[1] == 0xD8, "ssd_jpeg: not a JPEG stream (no SOI)");
    size_t at = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = 0, comp_id[3] = {0, 0, 0};
    ssd_jpeg_info& o = h.info;
    for (;;) {
        SSD_CHECK_ARG(at + 2 <= n && data[at] == 0xFF, "ssd_jpeg: truncated or damaged header at byte %zu", at);
        while (at < n && data[at] == 0xFF) ++at;                                  // fill bytes
        SSD_CHECK_ARG(at < n, "ssd_jpeg: truncated header");
        const int m = data[at++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;                      // no payload
        SSD_CHECK_ARG(m != 0xD9 && m != 0x00, "ssd_jpeg: no scan before the end of the image");
        SSD_CHECK_ARG(at + 2 <= n, "ssd_jpeg: truncated header");
        const int len = be16(data + at);
        SSD_CHECK_ARG(len >= 2 && at + (size_t)len <= n, "ssd_jpeg: segment %02X runs past the end of the data", m);
        const unsigned char* p = data + at + 2;
        const int plen = len - 2;
        if (m == 0xC0) {
            SSD_CHECK_ARG(!have_sof, "ssd_jpeg: two frame headers");
            SSD_CHECK_ARG(plen >= 6, "ssd_jpeg: short frame header");
            SSD_UNSUPPORTED_IF(p[0] != 8, "ssd_jpeg: %d-bit samples (8 only)", p[0]);
            o.height = be16(p + 1); o.width = be16(p + 3); o.components = p[5];
            SSD_CHECK_ARG(o.height >= 1 && o.width >= 1, "ssd_jpeg: empty image");
            SSD_UNSUPPORTED_IF(o.components != 1 && o.components != 3, "ssd_jpeg: %d components (CMYK / YCCK and others: grey and YCbCr only)", o.components);
            SSD_UNSUPPORTED_IF(o.height > kMaxImageSide || o.width > kMaxImageSide, "ssd_jpeg: %d x %d, outside 1..%d", o.height, o.width, kMaxImageSide);
            SSD_CHECK_ARG(plen >= 6 + 3 * o.components, "ssd_jpeg: short frame header");
            for (int c = 0; c < o.components; ++c) {
                comp_id[c] = p[6 + 3 * c];
                o.h_samp[c] = p[7 + 3 * c] >> 4; o.v_samp[c] = p[7 + 3 * c] & 15;
                o.quant_index[c] = p[8 + 3 * c];
                SSD_CHECK_ARG(o.h_samp[c] >= 1 && o.h_samp[c] <= 4 && o.v_samp[c] >= 1 && o.v_samp[c] <= 4, "ssd_jpeg: bad sampling factors");
                SSD_CHECK_ARG(o.quant_index[c] <= 3, "ssd_jpeg: bad quantisation table index");
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            SSD_UNSUPPORTED_IF(true, "ssd_jpeg: SOF%d (%s): baseline SOF0 only", m - 0xC0,
                               m == 0xC2 ? "progressive" : m == 0xC1 ? "extended sequential" : (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) ? "lossless" : m >= 0xC9 ? "arithmetic" : "hierarchical");
        } else if (m == 0xCC) {
            SSD_UNSUPPORTED_IF(true, "ssd_jpeg: arithmetic coding");
        } else if (m == 0xDB) {
            int q = 0;
            while (q < plen) {
                const int pq = p[q] >> 4, tq = p[q] & 15;
                SSD_CHECK_ARG(pq <= 1, "ssd_jpeg: bad quantisation table precision");
                SSD_UNSUPPORTED_IF(tq > 3, "ssd_jpeg: quantisation table %d (more than 4 tables)", tq);
                SSD_CHECK_ARG(q + 1 + 64 * (pq + 1) <= plen, "ssd_jpeg: short quantisation table");
                for (int i = 0; i < 64; ++i)
                    h.quant[tq][kZigzag[i]] = (unsigned short)(pq ? be16(p + q + 1 + 2 * i) : p[q + 1 + i]);
                h.quant_defined[tq] = true;
                q += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xC4) {
            int q = 0;
            while (q < plen) {
                SSD_CHECK_ARG(q + 17 <= plen, "ssd_jpeg: short Huffman table");
                const int tc = p[q] >> 4, th = p[q] & 15;
                SSD_CHECK_ARG(tc <= 1, "ssd_jpeg: bad Huffman table class");
                SSD_UNSUPPORTED_IF(th > 3, "ssd_jpeg: Huffman table %d (more than 4 tables)", th);
                int total = 0;
                for (int i = 0; i < 16; ++i) total += p[q + 1 + i];
                SSD_CHECK_ARG(total <= 256 && q + 17 + total <= plen, "ssd_jpeg: short Huffman table");
                if (tc == 0)
                    for (int i = 0; i < total; ++i) SSD_CHECK_ARG(p[q + 17 + i] <= 15, "ssd_jpeg: bad DC Huffman symbol");
                SSD_CHECK_ARG(build_huff(tc ? h.ac[th] : h.dc[th], p + q + 1, p + q + 17, total) == SSD_OK,
                              "ssd_jpeg: Huffman code lengths do not form a prefix code");
                q += 17 + total;
            }
        } else if (m == 0xDD) {
            SSD_CHECK_ARG(plen >= 2, "ssd_jpeg: short restart interval segment");
            o.restart_interval = be16(p);
        } else if (m == 0xE0) {
            if (plen >= 5 && memcmp(p, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (plen >= 12 && memcmp(p, "Adobe", 5) == 0) { adobe = true; adobe_transform = p[11]; }
        } else if (m == 0xDA) {
            SSD_CHECK_ARG(have_sof, "ssd_jpeg: scan before the frame header");
            SSD_CHECK_ARG(plen >= 1 && p[0] >= 1 && p[0] <= 4 && plen >= 1 + 2 * p[0] + 3, "ssd_jpeg: short scan header");
            SSD_UNSUPPORTED_IF(p[0] != o.components, "ssd_jpeg: a scan of %d of %d components (multi-scan files: one interleaved scan only)", p[0], o.components);
            for (int c = 0; c < o.components; ++c) {
                SSD_UNSUPPORTED_IF(p[1 + 2 * c] != comp_id[c], "ssd_jpeg: scan components out of frame order");
                h.dc_sel[c] = p[2 + 2 * c] >> 4; h.ac_sel[c] = p[2 + 2 * c] & 15;
                SSD_CHECK_ARG(h.dc_sel[c] <= 3 && h.ac_sel[c] <= 3 && h.dc[h.dc_sel[c]].defined && h.ac[h.ac_sel[c]].defined,
                              "ssd_jpeg: component %d uses a Huffman table the file does not define", c);
                SSD_CHECK_ARG(h.quant_defined[o.quant_index[c]], "ssd_jpeg: component %d uses a quantisation table the file does not define", c);
            }
            const unsigned char* s = p + 1 + 2 * o.components;
            SSD_CHECK_ARG(s[0] == 0 && s[1] == 63 && s[2] == 0, "ssd_jpeg: spectral selection / approximation in a baseline scan");
            h.scan_at = at + (size_t)len;
            break;
        }                                                                         // APPn, COM and the rest: skipped
        at += (size_t)len;
    }
    if (o.components == 3) {
        bool ycc = true;                                                          // libjpeg's rules
        if (jfif) ycc = true;
        else if (adobe) ycc = adobe_transform != 0;
        else ycc = !(comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B');
        SSD_UNSUPPORTED_IF(!ycc, "ssd_jpeg: an RGB file (YCbCr and grey only)");
        const int hs = o.h_samp[0], vs = o.v_samp[0];
        SSD_UNSUPPORTED_IF(o.h_samp[1] != 1 || o.v_samp[1] != 1 || o.h_samp[2] != 1 || o.v_samp[2] != 1 || !jpeg_sampling_ok(hs, vs),
                           "ssd_jpeg: sampling %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 only)", hs, vs, o.h_samp[1], o.v_samp[1],
                           o.h_samp[2], o.v_samp[2]);
    } else {
        o.h_samp[0] = o.v_samp[0] = 1;                                            // a one-component scan is not interleaved
    }
    jpeg_complete_info(o);
    for (int c = 0; c < o.components; ++c) memcpy(o.quant[c], h.quant[o.quant_index[c]], 128);
    return SSD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// host: entropy-coded segment

struct bit_reader {
    const unsigned char* data;
    size_t n, at;
    unsigned long long acc;     // the low `bits` bits are data not yet consumed
    int bits;
    bool stopped;               // a marker or the end of the data: nothing more to feed

    inline void fill() {
        while (bits <= 56 && !stopped) {
            if (at >= n) { stopped = true; break; }
            const unsigned b = data[at];
            if (b == 0xFF) {
                if (at + 1 < n && data[at + 1] == 0x00) at += 2;                   // a stuffed data byte
                else { stopped = true; break; }                                    // a marker (or the data ends in FF)
            } else {
                ++at;
            }
            acc = (acc << 8) | b;
            bits += 8;
        }
    }
    // the next k <= 16 bits, zero-padded past the end of the data (consume() refuses to take padding)
    inline unsigned peek(const int k) {
        if (bits < k) fill();
        return bits >= k ? (unsigned)(acc >> (bits - k)) & ((1u << k) - 1) : (unsigned)(acc << (k - bits)) & ((1u << k) - 1);
    }
    inline bool consume(const int k) {
        if (k > bits) return false;
        bits -= k;
        return true;
    }
};

// -1: the code is not in the table, -2: the data ended
static inline int huff_decode(bit_reader& br, const huff_table& t) {
    const unsigned v = br.peek(16);
    const unsigned e = t.look[v >> 8];
    if (e) return br.consume((int)(e >> 8)) ? (int)(e & 255) : -2;
    for (int len = 9; len <= 16; ++len) {
        const int code = (int)(v >> (16 - len));
        if (code <= t.maxcode[len]) return br.consume(len) ? t.vals[t.valoff[len] + code] : -2;
    }
    return -1;
}

static inline int extend(const int v, const int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

static int decode_block(bit_reader& br, const huff_table& dc, const huff_table& ac, int& pred, short* coef) {
    int s = huff_decode(br, dc);
    SSD_CHECK_ARG(s != -1, "ssd_jpeg_entropy_decode: a code that is not in the DC table");
    SSD_CHECK_ARG(s >= 0, "ssd_jpeg_entropy_decode: the data ends before the last MCU");
    if (s) {
        const int v = (int)br.peek(s);
        SSD_CHECK_ARG(br.consume(s), "ssd_jpeg_entropy_decode: the data ends before the last MCU");
        pred = (int)((unsigned)pred + (unsigned)extend(v, s));
    }
    coef[0] = (short)pred;
    for (int k = 1; k < 64;) {
        const int rs = huff_decode(br, ac);
        SSD_CHECK_ARG(rs != -1, "ssd_jpeg_entropy_decode: a code that is not in the AC table");
        SSD_CHECK_ARG(rs >= 0, "ssd_jpeg_entropy_decode: the data ends before the last MCU");
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;                                                    // end of block
            k += 16;
            continue;
        }
        k += r;
        SSD_CHECK_ARG(k <= 63, "ssd_jpeg_entropy_decode: a coefficient index past 63");
        const int v = (int)br.peek(s);
        SSD_CHECK_ARG(br.consume(s), "ssd_jpeg_entropy_decode: the data ends before the last MCU");
        coef[kZigzag[k]] = (short)extend(v, s);
        ++k;
    }
    return SSD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// device

// the post-IDCT range-limit table of libjpeg, indexed with (v & 1023), as a function (it wraps: not a clamp)
__host__ __device__ __forceinline__ int idct_range_limit(const int v) {
    const int i = v & 1023;
    return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

// one 8-point pass of the "islow" inverse DCT: 13-bit constants, int32, descale by `shift` bits with rounding
__host__ __device__ __forceinline__ void idct_islow_1d(const int in[8], int out[8], const int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * kFix0_541196100;
    int tmp2 = z1 + z3 * (-kFix1_847759065);
    int tmp3 = z1 + z2 * kFix0_765366865;
    int tmp0 = (in[0] + in[4]) * 8192;
    int tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * kFix1_175875602;
    tmp0 *= kFix0_298631336; tmp1 *= kFix2_053119869; tmp2 *= kFix3_072711026; tmp3 *= kFix1_501321110;
    z1 *= -kFix0_899976223; z2 *= -kFix2_562915447; z3 *= -kFix1_961570560; z4 *= -kFix0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int half = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + half) >> shift; out[7] = (tmp10 - tmp3 + half) >> shift;
    out[1] = (tmp11 + tmp2 + half) >> shift; out[6] = (tmp11 - tmp2 + half) >> shift;
    out[2] = (tmp12 + tmp1 + half) >> shift; out[5] = (tmp12 - tmp1 + half) >> shift;
    out[3] = (tmp13 + tmp0 + half) >> shift; out[4] = (tmp13 - tmp0 + half) >> shift;
}

__host__ __device__ __forceinline__ jpeg_geometry jpeg_geom(const ssd_jpeg_desc& d) {
    return jpeg_geom(d.H, d.W, d.h_samp, d.v_samp, d.components);
}

// Kernel 1: dequantise + inverse DCT.  One index space of 8x8 blocks over the whole batch (desc[b].block_start is the
// prefix), 8 lanes per block, 32 blocks per workgroup.  Lane j runs column j (pass 1, from the coefficients: for a fixed
// row the 8 lanes read 16 contiguous bytes, a wave covers 1 KiB in 8 loads), the 8x8 int32 intermediate is transposed
// through LDS (rows padded to 9 words: both sides conflict-free), then lane j runs row j (pass 2) and stores its 8 samples
// with one aligned 8-byte store into the component plane.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const unsigned char* __restrict__ packed,
                                                       const ssd_jpeg_desc* __restrict__ desc, const int B,
                                                       const int total_blocks, unsigned char* __restrict__ planes) {
    __shared__ int ws[32][8][9];
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int blk = blockIdx.x * 32 + slot;
    const bool live = blk < total_blocks;
    ssd_jpeg_desc d;
    int local = 0;
    if (live) {
        const int b = find_image(B, blk, [&](const int i) { return desc[i].block_start; });
        d = desc[b];
        local = blk - d.block_start;
        const short* coef = reinterpret_cast<const short*>(packed + d.coef_offset) + (long)local * 64;
        const int comp = jpeg_block(jpeg_geom(d), local).comp;
        const unsigned short* q = reinterpret_cast<const unsigned short*>(packed + d.quant_offset) + comp * 64;
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (int)coef[r * 8 + j] * (int)q[r * 8 + j];
        idct_islow_1d(in, out, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[slot][r][j] = out[r];
    }
    __syncthreads();
    if (live) {
        const jpeg_block_place p = jpeg_block(jpeg_geom(d), local);
        int in[8], out[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = ws[slot][j][c];
        idct_islow_1d(in, out, 18);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= (unsigned)idct_range_limit(out[c]) << (8 * c);
            hi |= (unsigned)idct_range_limit(out[c + 4]) << (8 * c);
        }
        *reinterpret_cast<uint2*>(planes + (d.plane_offset + p.plane_at) + ((long)(p.by * 8 + j) * p.bw + p.bx) * 8) = make_uint2(lo, hi);
    }
}

__device__ __forceinline__ int clamp8(const int v) { return min(max(v, 0), 255); }

// one upsampled chroma sample at output pixel (y, x); p: the component plane, pitch bytes per row, of which only the
// cw x ch real samples are read
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, const int pitch, const int cw, const int ch,
                                         const int hs, const int vs, const int y, const int x) {
    if (hs == 1) return p[(long)y * pitch + x];
    const int i = x >> 1;
    if (vs == 1) {
        const unsigned char* s = p + (long)y * pitch;
        if (cw <= 2) return s[i];                                                  // the library's plain replication
        if (x & 1) return i == cw - 1 ? s[i] : (3 * s[i] + s[i + 1] + 2) >> 2;
        return i == 0 ? s[0] : (3 * s[i] + s[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    if (cw <= 2) return p[(long)r * pitch + i];
    const int far = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);                  // the top / last real row replicated
    const unsigned char* s0 = p + (long)r * pitch;
    const unsigned char* s1 = p + (long)far * pitch;
    const int cur = 3 * s0[i] + s1[i];
    if (x & 1) return i == cw - 1 ? (cur * 4 + 7) >> 4 : (cur * 3 + 3 * s0[i + 1] + s1[i + 1] + 7) >> 4;
    return i == 0 ? (cur * 4 + 8) >> 4 : (cur * 3 + 3 * s0[i - 1] + s1[i - 1] + 8) >> 4;
}

// Kernel 2: upsampling + colour conversion, or the copy of a raw-pixel image.  One index space of items over the batch
// (desc[b].item_start is the prefix); an item is FOUR consecutive pixels of the image's flattened [H*W] pixel order = 12
// output bytes = three aligned dword stores (images start at multiples of 16).
__global__ __launch_bounds__(256) void jpeg_color_kernel(const unsigned char* __restrict__ packed,
                                                        const ssd_jpeg_desc* __restrict__ desc,
                                                        const ssd_image_desc* __restrict__ out_desc, const int B,
                                                        const int total_items, const unsigned char* __restrict__ planes,
                                                        unsigned char* __restrict__ rgb) {
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= total_items) return;
    const int b = find_image(B, item, [&](const int i) { return desc[i].item_start; });
    const ssd_jpeg_desc d = desc[b];
    const int npix = d.H * d.W;
    const int p0 = (item - d.item_start) * 4;
    const int count = min(4, npix - p0);
    unsigned char* o = rgb + out_desc[b].src_offset + (long)p0 * 3;
    unsigned w[3] = {0, 0, 0};
    if (d.kind == SSD_JPEG_RAW) {
        const unsigned char* s = packed + d.coef_offset + (long)p0 * 3;
        if (count == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const unsigned*>(s)[k];
        } else {
            for (int k = 0; k < count * 3; ++k) w[k >> 2] |= (unsigned)s[k] << (8 * (k & 3));
        }
    } else {
        const jpeg_geometry g = jpeg_geom(d);
        const int ypitch = g.bw0 * 8, cpitch = g.mcus_x * 8;
        const unsigned char* py = planes + d.plane_offset;
        const unsigned char* pcb = py + (long)g.bw0 * g.bh0 * 64;
        const unsigned char* pcr = pcb + (long)g.mcus_x * g.mcus_y * 64;
        const int cw = (d.W + d.h_samp - 1) / d.h_samp, ch = (d.H + d.v_samp - 1) / d.v_samp;
        int y = p0 / d.W, x = p0 - y * d.W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < count) {
                const int Y = py[(long)y * ypitch + x];
                int r = Y, gg = Y, bl = Y;
                if (d.components == 3) {
                    const int cb = chroma_at(pcb, cpitch, cw, ch, d.h_samp, d.v_samp, y, x) - 128;
                    const int cr = chroma_at(pcr, cpitch, cw, ch, d.h_samp, d.v_samp, y, x) - 128;
                    r = clamp8(Y + ((91881 * cr + 32768) >> 16));
                    gg = clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                    bl = clamp8(Y + ((116130 * cb + 32768) >> 16));
                }
                const int at = k * 3;
                w[at >> 2] |= (unsigned)r << (8 * (at & 3));
                w[(at + 1) >> 2] |= (unsigned)gg << (8 * ((at + 1) & 3));
                w[(at + 2) >> 2] |= (unsigned)bl << (8 * ((at + 2) & 3));
                if (++x == d.W) { x = 0; ++y; }
            }
        }
    }
    if (count == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<unsigned*>(o)[k] = w[k];
    } else {
        for (int k = 0; k < count * 3; ++k) o[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
    }
}

static inline bool jpeg_desc_shape_ok(const ssd_jpeg_desc& d) { return image_side_ok(d.H) && image_side_ok(d.W); }
static inline bool jpeg_desc_sampling_ok(const ssd_jpeg_desc& d) {
    if (d.components == 1) return d.h_samp == 1 && d.v_samp == 1;
    return d.components == 3 && jpeg_sampling_ok(d.h_samp, d.v_samp);
}

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_jpeg_parse(const unsigned char* data, size_t n, struct ssd_jpeg_info* out) {
    SSD_CHECK_ARG(out, "ssd_jpeg_parse: NULL pointer");
    jpeg_header h;
    const int rc = parse_header(data, n, h);
    if (rc != SSD_OK) return rc;
    memcpy(out, &h.info, sizeof(*out));
    return SSD_OK;
}

extern "C" int ssd_jpeg_entropy_decode(const unsigned char* data, size_t n, const struct ssd_jpeg_info* info, short* coef_out,
                                       size_t coef_bytes) {
    SSD_CHECK_ARG(info && coef_out, "ssd_jpeg_entropy_decode: NULL pointer");
    jpeg_header h;
    const int rc = parse_header(data, n, h);
    if (rc != SSD_OK) return rc;
    SSD_CHECK_ARG(memcmp(&h.info, info, sizeof(*info)) == 0, "ssd_jpeg_entropy_decode: info does not describe this stream");
    SSD_CHECK_ARG((long long)coef_bytes >= h.info.coef_bytes, "ssd_jpeg_entropy_decode: coef_out holds %zu bytes, the image needs %lld",
                  coef_bytes, h.info.coef_bytes);
    const ssd_jpeg_info& o = h.info;
    memset(coef_out, 0, (size_t)o.coef_bytes);
    bit_reader br = {data, n, h.scan_at, 0, 0, false};
    int pred[3] = {0, 0, 0};
    const long mcus = (long)o.mcus_x * o.mcus_y;
    int rst = 0;
    long until_restart = o.restart_interval;
    for (long m = 0; m < mcus; ++m) {
        if (o.restart_interval && until_restart == 0) {
            br.bits = 0; br.acc = 0;                                               // padding bits of the interval
            size_t at = br.at;
            SSD_CHECK_ARG(at < n && data[at] == 0xFF, "ssd_jpeg_entropy_decode: bad restart marker before MCU %ld", m);
            while (at < n && data[at] == 0xFF) ++at;
            SSD_CHECK_ARG(at < n && data[at] == 0xD0 + (rst & 7), "ssd_jpeg_entropy_decode: bad restart marker before MCU %ld", m);
            br.at = at + 1; br.stopped = false;
            ++rst;
            pred[0] = pred[1] = pred[2] = 0;
            until_restart = o.restart_interval;
        }
        --until_restart;
        const int my = (int)(m / o.mcus_x), mx = (int)(m - (long)my * o.mcus_x);
        for (int c = 0; c < o.components; ++c)
            for (int v = 0; v < o.v_samp[c]; ++v)
                for (int u = 0; u < o.h_samp[c]; ++u) {
                    const long blk = (long)(my * o.v_samp[c] + v) * o.blocks_w[c] + mx * o.h_samp[c] + u;
                    short* coef = coef_out + o.coef_offset[c] / 2 + blk * 64;
                    const int r = decode_block(br, h.dc[h.dc_sel[c]], h.ac[h.ac_sel[c]], pred[c], coef);
                    if (r != SSD_OK) return r;
                }
    }
    return SSD_OK;
}

// The marker walk of the scan: a memchr over the bytes, no code is decoded.  Segment ends are where bit_reader::fill stops;
// the markers are the ones ssd_jpeg_entropy_decode looks for.
static int scan_plan(const unsigned char* data, const size_t n, const jpeg_header& h, struct ssd_jpeg_scan_plan* plan, ssd_jpeg_segment* segs,
                     const size_t seg_capacity) {
    const ssd_jpeg_info& o = h.info;
    const long mcus = (long)o.mcus_x * o.mcus_y, ri = o.restart_interval;
    const long nseg = ri ? (mcus + ri - 1) / ri : 1;
    SSD_CHECK_ARG((size_t)nseg <= seg_capacity, "ssd_jpeg_scan_plan: room for %zu segments, the frame has %ld", seg_capacity, nseg);
    memset(plan, 0, sizeof(*plan));
    for (int c = 0; c < o.components; ++c)
        for (int a = 0; a < 2; ++a) {
            const huff_table& t = a ? h.ac[h.ac_sel[c]] : h.dc[h.dc_sel[c]];
            ssd_jpeg_huff& d = plan->huff[2 * c + a];
            memcpy(d.look, t.look, sizeof(d.look));
            memcpy(d.maxcode, t.maxcode, sizeof(d.maxcode));
            memcpy(d.valoff, t.valoff, sizeof(d.valoff));
            memcpy(d.vals, t.vals, sizeof(d.vals));
            d.maxcode[0] = -1; d.valoff[0] = 0;                                   // never indexed: a defined value
        }
    size_t at = h.scan_at;
    for (long k = 0; k < nseg; ++k) {
        const size_t first = at;
        size_t end = first;
        for (;;) {
            const unsigned char* ff = end < n ? (const unsigned char*)memchr(data + end, 0xFF, n - end) : nullptr;
            if (!ff) { end = n; break; }
            end = (size_t)(ff - data);
            if (end + 1 < n && data[end + 1] == 0x00) { end += 2; continue; }      // a stuffed data byte
            break;                                                                 // a marker (or the data ends in FF)
        }
        SSD_UNSUPPORTED_IF((long long)(end - h.scan_at) >= SSD_JPEG_UNPACK_MAX_SCAN_BYTES,
                           "ssd_jpeg_scan_plan: %zu bytes of entropy-coded data (below %lld only)", end - h.scan_at,
                           (long long)SSD_JPEG_UNPACK_MAX_SCAN_BYTES);
        segs[k].first_byte = (unsigned)(first - h.scan_at);
        segs[k].bytes = (unsigned)(end - first);
        segs[k].first_mcu = (int)(k * ri);
        segs[k].reserved = 0;
        at = end;
        if (k + 1 < nseg) {
            SSD_CHECK_ARG(at < n && data[at] == 0xFF, "ssd_jpeg_scan_plan: bad restart marker after segment %ld", k);
            while (at < n && data[at] == 0xFF) ++at;                              // fill bytes
            SSD_CHECK_ARG(at < n && data[at] == 0xD0 + (k & 7), "ssd_jpeg_scan_plan: bad restart marker after segment %ld", k);
            ++at;
        }
    }
    plan->data_begin = (long long)h.scan_at;
    plan->data_end = (long long)at;
    plan->segments = (int)nseg;
    return SSD_OK;
}

extern "C" int ssd_jpeg_scan_plan(const unsigned char* data, size_t n, const struct ssd_jpeg_info* info, struct ssd_jpeg_scan_plan* plan,
                                  struct ssd_jpeg_segment* segments, size_t seg_capacity) {
    SSD_CHECK_ARG(info && plan && segments, "ssd_jpeg_scan_plan: NULL pointer");
    jpeg_header h;
    const int rc = parse_header(data, n, h);
    if (rc != SSD_OK) return rc;
    SSD_CHECK_ARG(memcmp(&h.info, info, sizeof(*info)) == 0, "ssd_jpeg_scan_plan: info does not describe this stream");
    return scan_plan(data, n, h, plan, segments, seg_capacity);
}

// The host model of ssd_jpeg_unpack: the phases of ssd_jpeg_unpack.hip as loops over "threads", on the decode core both
// include.  A sweep is two loops, as the kernel's is two barrier phases: every thread decodes from its entry state, then
// every thread takes its left neighbour's exit state.
extern "C" int ssd_jpeg_entropy_decode_subseq(const unsigned char* data, size_t n, const struct ssd_jpeg_info* info, short* coef_out,
                                              size_t coef_bytes, int subseq_bits) {
    SSD_CHECK_ARG(info && coef_out, "ssd_jpeg_entropy_decode_subseq: NULL pointer");
    const int S = subseq_bits ? subseq_bits : kUnpackDefaultBits;
    SSD_UNSUPPORTED_IF(S % 32 != 0 || S < 128 || S > SSD_JPEG_UNPACK_MAX_SUBSEQ_BITS,
                       "ssd_jpeg_entropy_decode_subseq: subseq_bits = %d (0, or a multiple of 32 in 128..%d)", subseq_bits,
                       SSD_JPEG_UNPACK_MAX_SUBSEQ_BITS);
    jpeg_header h;
    int rc = parse_header(data, n, h);
    if (rc != SSD_OK) return rc;
    SSD_CHECK_ARG(memcmp(&h.info, info, sizeof(*info)) == 0, "ssd_jpeg_entropy_decode_subseq: info does not describe this stream");
    SSD_CHECK_ARG((long long)coef_bytes >= h.info.coef_bytes, "ssd_jpeg_entropy_decode_subseq: coef_out holds %zu bytes, the image needs %lld",
                  coef_bytes, h.info.coef_bytes);
    const ssd_jpeg_info& o = h.info;
    const unpack_frame f = unpack_frame_of(o.height, o.width, o.h_samp[0], o.v_samp[0], o.components);
    const long ri = o.restart_interval;
    std::vector<ssd_jpeg_segment> segs((size_t)(ri ? (f.mcus + ri - 1) / ri : 1));
    struct ssd_jpeg_scan_plan plan;
    rc = scan_plan(data, n, h, &plan, segs.data(), segs.size());
    if (rc != SSD_OK) return rc;
    memset(coef_out, 0, (size_t)o.coef_bytes);
    int flags = 0;
    std::vector<unpack_state> entry;
    std::vector<unsigned> before;
    for (size_t si = 0; si < segs.size(); ++si) {
        const unpack_seg seg = {data + plan.data_begin + segs[si].first_byte, segs[si].bytes};
        const unsigned nsub = unpack_nsub(seg.len, S);
        const long left = f.mcus - segs[si].first_mcu;
        const unsigned seg_blocks = (unsigned)((ri && ri < left ? ri : left) * f.nz);
        auto end_bit = [&](const unsigned j) { const unsigned long long e = (unsigned long long)(j + 1) * S; return e < seg.len * 8ull ? (unsigned)e : seg.len * 8u; };
        entry.assign(nsub, unpack_state{0, 0, 0});
        before.assign(nsub + 1, 0u);
        unpack_state carry = {0, 0, 0}, exits[kUnpackChunk];
        unsigned counts[kUnpackChunk], running = 0;
        bool dirty[kUnpackChunk];
        for (unsigned base = 0; base < nsub; base += kUnpackChunk) {
            const unsigned cnt = nsub - base < (unsigned)kUnpackChunk ? nsub - base : (unsigned)kUnpackChunk;
            // a. synchronise: the segment's first state is known, a chunk's first is the settled exit of the chunk before
            for (unsigned t = 0; t < cnt; ++t) {
                entry[base + t] = base + t == 0 ? unpack_state{0, 0, 0} : (t == 0 ? carry : unpack_guess(seg, base + t, S));
                dirty[t] = true;
            }
            for (int sweep = 0; sweep < kUnpackChunk; ++sweep) {
                for (unsigned t = 0; t < cnt; ++t)
                    if (dirty[t]) { exits[t] = unpack_sweep(seg, plan.huff, f, entry[base + t], end_bit(base + t), counts[t]); dirty[t] = false; }
                bool any = false;
                for (unsigned t = 1; t < cnt; ++t)
                    if (exits[t - 1] != entry[base + t]) { entry[base + t] = exits[t - 1]; dirty[t] = true; any = true; }
                if (!any) break;
            }
            carry = exits[cnt - 1];
            // b. place: the blocks completed before each subsequence of the segment
            for (unsigned t = 0; t < cnt; ++t) { before[base + t] = running; running += counts[t]; }
        }
        // c. write
        for (unsigned j = 0; j < nsub; ++j)
            flags |= unpack_write(seg, plan.huff, f, kZigzag, entry[j], end_bit(j), before[j], seg_blocks, segs[si].first_mcu, j + 1 == nsub,
                                  si + 1 == segs.size(), coef_out);
    }
    // d. DC prediction, per component and segment in scan order.  decode_block computes coef[0] = (short)(unsigned 32-bit
    // running sum), so a sum that wraps at 16 bits gives the same bits.
    for (int c = 0; c < o.components; ++c) {
        const int per = c == 0 ? f.nl : 1;
        const long total = (long)f.mcus * per, seglen = ri ? ri * per : total;
        unsigned short run = 0;
        for (long e = 0; e < total; ++e) {
            if (e % seglen == 0) run = 0;
            short* dcv = coef_out + unpack_dc_at(f, c, per, (int)e);
            run = (unsigned short)(run + (unsigned short)*dcv);
            *dcv = (short)run;
        }
    }
    SSD_CHECK_ARG((flags & kUnpackBadCode) == 0, "ssd_jpeg_entropy_decode_subseq: a code that is not in its table, or a coefficient index past 63");
    SSD_CHECK_ARG((flags & kUnpackShort) == 0, "ssd_jpeg_entropy_decode_subseq: the data ends before the last MCU");
    SSD_CHECK_ARG(flags == 0, "ssd_jpeg_entropy_decode_subseq: a restart interval does not end in its segment's last byte");
    return SSD_OK;
}

extern "C" size_t ssd_jpeg_decode_workspace_bytes(const struct ssd_jpeg_desc* desc_host, int B) {
    if (!desc_host || B <= 0) return 0;
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_desc& d = desc_host[b];
        if (d.kind == SSD_JPEG_COEFFICIENTS && jpeg_desc_shape_ok(d) && jpeg_desc_sampling_ok(d))
            total += align_up((size_t)jpeg_geom(d).nblocks * 64, 16);
    }
    return total;
}

extern "C" int ssd_jpeg_decode(const unsigned char* packed_dev, size_t bytes, const struct ssd_jpeg_desc* desc_host,
                               const struct ssd_jpeg_desc* desc_dev, int B, unsigned char* rgb_dev, size_t rgb_bytes,
                               const struct ssd_image_desc* out_desc_host, const struct ssd_image_desc* out_desc_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_jpeg_decode: bad batch");
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_jpeg_decode: B = %d (at most 65535)", B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(packed_dev && desc_host && desc_dev && rgb_dev && out_desc_host && out_desc_dev, "ssd_jpeg_decode: NULL pointer");
    SSD_CHECK_ARG((((size_t)packed_dev | (size_t)rgb_dev | (size_t)workspace_dev) & 15) == 0, "ssd_jpeg_decode: a buffer is not 16-byte aligned");
    long blocks = 0, items = 0;
    size_t plane_end = 0, rgb_end = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_jpeg_desc& d = desc_host[b];
        const ssd_image_desc& o = out_desc_host[b];
        SSD_CHECK_ARG(d.kind == SSD_JPEG_COEFFICIENTS || d.kind == SSD_JPEG_RAW, "ssd_jpeg_decode: image %d: kind %d", b, d.kind);
        SSD_UNSUPPORTED_IF(!jpeg_desc_shape_ok(d), "ssd_jpeg_decode: image %d is %d x %d, outside 1..%d", b, d.H, d.W, kMaxImageSide);
        SSD_CHECK_ARG(o.H == d.H && o.W == d.W, "ssd_jpeg_decode: image %d: the output descriptor has another size", b);
        const size_t pixels = (size_t)d.H * d.W * 3;
        SSD_CHECK_ARG(region_ok(o.src_offset, pixels, rgb_bytes, 16, &rgb_end),
                      "ssd_jpeg_decode: image %d: output outside rgb_dev, misaligned or overlapping", b);
        SSD_CHECK_ARG(d.coef_offset >= 0 && (d.coef_offset & 15) == 0, "ssd_jpeg_decode: image %d: offset not a multiple of 16", b);
        SSD_CHECK_ARG(d.block_start == blocks && d.item_start == items, "ssd_jpeg_decode: image %d: block_start / item_start are not the running sums", b);
        if (d.kind == SSD_JPEG_RAW) {
            SSD_CHECK_ARG(region_ok(d.coef_offset, pixels, bytes, 16), "ssd_jpeg_decode: image %d lies outside the packed buffer", b);
        } else {
            SSD_UNSUPPORTED_IF(!jpeg_desc_sampling_ok(d), "ssd_jpeg_decode: image %d: %d components sampled %dx%d", b, d.components,
                               d.h_samp, d.v_samp);
            const size_t nb = (size_t)jpeg_geom(d).nblocks;
            SSD_CHECK_ARG(region_ok(d.coef_offset, nb * 128, bytes, 16), "ssd_jpeg_decode: image %d lies outside the packed buffer", b);
            SSD_CHECK_ARG(region_ok(d.quant_offset, 384, bytes, 16),
                          "ssd_jpeg_decode: image %d: quantisation tables outside the packed buffer or misaligned", b);
            SSD_CHECK_ARG(workspace_dev && region_ok(d.plane_offset, nb * 64, workspace_bytes, 16, &plane_end),
                          "ssd_jpeg_decode: image %d: planes outside the workspace, misaligned or overlapping", b);
            blocks += (long)nb;
        }
        items += ((long)d.H * d.W + 3) / 4;
        SSD_UNSUPPORTED_IF(blocks >= (1L << 31) - 64 || items >= (1L << 31) - 512, "ssd_jpeg_decode: the batch is too large for one call (image %d)", b);
    }
    if (blocks > 0) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, (hipStream_t)stream, packed_dev,
                           desc_dev, B, (int)blocks, (unsigned char*)workspace_dev);
        SSD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, packed_dev,
                       desc_dev, out_desc_dev, B, (int)items, (const unsigned char*)workspace_dev, rgb_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
