// PNG decoding behind a host inflate ("PNG decoding"; the format contract: include/ssd_hip.h, "PNG
// DECODER").  The host half -- ssd_png_parse / ssd_png_idat: plain C++, no HIP call -- walks the chunks and hands the zlib
// stream to the caller's inflate; what inflate returns, H rows of (filter byte, filtered bytes), goes to the device as it
// is.  Two kernels per call, whatever the batch:
//   1 unfilter  one wavefront per CHAIN.  A chain begins at row 0 and at every row whose filter is None or Sub: such a row
//               needs nothing of the row above, so chains are independent (one index space over the batch).  Inside a
//               chain a wavefront takes 64 rows at a time as a skewed pipeline: lane l owns row y0 + l and runs one pixel
//               (one filter distance) behind lane l - 1, so "up" arrives from the lane above by __shfl_up, "up-left" is
//               last step's "up", and "left" stays in registers.  Lane 0's "up" is the last row of the band before, read
//               back from the workspace.  The unfiltered rows go to the workspace.
//   2 convert   one workgroup per (image, row) over one index space: unfiltered samples -> packed RGB (png_pixel_rgb), the
//               palette from LDS; the stores of a row are contiguous.
// ssd_png_decode_host runs the same step functions (ssd_png_common.h) as plain loops.  Integer arithmetic only.
#include <climits>
#include <cstring>
#include <vector>

#include "ssd_jpeg_common.h"
#include "ssd_png_common.h"

namespace ssd {

static const int kPngDecWaves = 4;      // chains per workgroup of kernel 1: a wavefront each, they share nothing
static const int kPngDecAhead = 4;      // pipeline steps whose loads are issued together

__device__ __forceinline__ int png_clamp(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Rows r0 .. r1 - 1 of one image, a chain: `in` its filtered rows (1 + rb bytes each), `raw` its unfiltered rows (rb bytes
// each).  FD: the filter distance; rb is a multiple of it (FD > 1 means whole bytes per sample).
template <int FD>
__device__ void png_unfilter_chain(const unsigned char* __restrict__ in, unsigned char* raw, const long long rb, const int r0, const int r1) {
    const int lane = threadIdx.x & 63;
    const int npx = (int)(rb / FD);
    for (int y0 = r0; y0 < r1; y0 += 64) {
        const int rows = r1 - y0 < 64 ? r1 - y0 : 64;
        const bool live = lane < rows;
        const int y = live ? y0 + lane : y0;
        const unsigned char* src = in + (long long)y * (rb + 1);
        unsigned char* dst = raw + (long long)y * rb;
        int type = src[0];
        if (type > 4) type = 0;                                                     // the host refuses such a file; no other path here
        const bool carried = y0 > r0;                                               // a chain's first row reads nothing above it
        const unsigned char* above = raw + (long long)(carried ? y0 - 1 : y0) * rb;
        int a[FD], b[FD], c[FD];
#pragma unroll
        for (int k = 0; k < FD; ++k) a[k] = b[k] = c[k] = 0;
        const int steps = npx + rows - 1;
        for (int s0 = 0; s0 < steps; s0 += kPngDecAhead) {
            int v[kPngDecAhead][FD], top[kPngDecAhead][FD];
#pragma unroll
            for (int u = 0; u < kPngDecAhead; ++u) {
                const int x = s0 + u - lane;
                const bool on = live && x >= 0 && x < npx;
                const bool first = lane == 0 && carried && x < npx;
#pragma unroll
                for (int k = 0; k < FD; ++k) {
                    v[u][k] = on ? src[1 + (long long)x * FD + k] : 0;
                    // written by lane 63 a band ago, behind a fence: read past this CU's vector cache
                    top[u][k] = first ? (int)__hip_atomic_load(above + (long long)x * FD + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < kPngDecAhead; ++u) {
                const int x = s0 + u - lane;
                const bool on = live && x >= 0 && x < npx;
                // the lane above finished this pixel one step ago
                unsigned lo = 0, hi = 0;
#pragma unroll
                for (int k = 0; k < FD; ++k) {
                    if (k < 4) lo |= (unsigned)a[k] << (8 * k); else hi |= (unsigned)a[k] << (8 * (k - 4));
                }
                lo = __shfl_up(lo, 1);
                if (FD > 4) hi = __shfl_up(hi, 1);
#pragma unroll
                for (int k = 0; k < FD; ++k) {
                    c[k] = b[k];
                    const int up = (int)(((k < 4 ? lo : hi) >> (8 * (k & 3))) & 255u);
                    b[k] = lane == 0 ? top[u][k] : up;
                }
                if (on) {
#pragma unroll
                    for (int k = 0; k < FD; ++k) {
                        a[k] = (int)png_unfilter(type, v[u][k], a[k], b[k], c[k]);
                        dst[(long long)x * FD + k] = (unsigned char)a[k];
                    }
                }
            }
        }
        __threadfence();                                                            // the band's last row, before the next band's lane 0 reads it
    }
}

// Kernel 1: wavefront g of the launch takes chain g of the batch.  The chain list is the caller's; whatever it holds, the
// rows are clamped to the image, so nothing outside the image's rows is read or written.
__global__ __launch_bounds__(64 * kPngDecWaves) void png_unfilter_kernel(const unsigned char* __restrict__ packed, const ssd_png_dec_desc* __restrict__ desc,
                                                                        const int B, const int chains, unsigned char* __restrict__ ws) {
    const int g = blockIdx.x * kPngDecWaves + (threadIdx.x >> 6);
    if (g >= chains) return;
    const int b = find_image(B, g, [&](const int i) { return desc[i].chain_start; });
    const ssd_png_dec_desc d = desc[b];
    const int k = g - d.chain_start;
    const int* list = reinterpret_cast<const int*>(packed + d.chain_offset);
    const int r0 = png_clamp(list[k], 0, d.H);
    const int r1 = png_clamp(k + 1 < d.chains ? list[k + 1] : d.H, r0, d.H);
    const long long rb = png_row_bytes(d.W, d.color_type, d.depth);
    const unsigned char* in = packed + d.src_offset;
    unsigned char* raw = ws + d.raw_offset;
    switch (png_filter_distance(d.color_type, d.depth)) {
        case 1: png_unfilter_chain<1>(in, raw, rb, r0, r1); break;
        case 2: png_unfilter_chain<2>(in, raw, rb, r0, r1); break;
        case 3: png_unfilter_chain<3>(in, raw, rb, r0, r1); break;
        case 4: png_unfilter_chain<4>(in, raw, rb, r0, r1); break;
        case 6: png_unfilter_chain<6>(in, raw, rb, r0, r1); break;
        default: png_unfilter_chain<8>(in, raw, rb, r0, r1); break;
    }
}

// Kernel 2: row y of image b, converted.  A workgroup takes the rows blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(256) void png_convert_kernel(const unsigned char* __restrict__ packed, const ssd_png_dec_desc* __restrict__ desc, const int B,
                                                         const int rows, const unsigned char* __restrict__ ws, unsigned char* __restrict__ rgb) {
    __shared__ unsigned char palette[768];
    const int tid = threadIdx.x;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int b = find_image(B, (int)row, [&](const int i) { return desc[i].row_start; });
        const ssd_png_dec_desc d = desc[b];
        const int y = (int)row - d.row_start;
        if (d.color_type == 3) {
            __syncthreads();                                                        // the row before may still read the palette
            for (int i = tid; i < 768; i += 256) palette[i] = packed[d.palette_offset + i];
            __syncthreads();
        }
        const unsigned char* src = ws + d.raw_offset + (long long)y * png_row_bytes(d.W, d.color_type, d.depth);
        unsigned char* dst = rgb + d.dst_offset + (long long)y * d.W * 3;
        for (int x = tid; x < d.W; x += 256) {
            unsigned char px[3];
            png_pixel_rgb(src, x, d.color_type, d.depth, palette, px);
            dst[3 * x] = px[0]; dst[3 * x + 1] = px[1]; dst[3 * x + 2] = px[2];
        }
    }
}

static const char* const kPngDecName = "ssd_png_decode";

// ---- the host half ------------------------------------------------------------------------------------------------------
struct png_crc_table {
    unsigned t[4][256];
    png_crc_table() {
        for (unsigned i = 0; i < 256; ++i) t[0][i] = png_crc_byte(i, 0) ;
        for (unsigned i = 0; i < 256; ++i)
            for (int k = 1; k < 4; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255u];
    }
};
// the CRC-32 register after `n` more bytes, four at a time
static unsigned png_crc_run(unsigned crc, const unsigned char* p, size_t n) {
    static const png_crc_table T;
    while (n >= 4) {
        crc ^= (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        crc = T.t[3][crc & 255u] ^ T.t[2][(crc >> 8) & 255u] ^ T.t[1][(crc >> 16) & 255u] ^ T.t[0][crc >> 24];
        p += 4;
        n -= 4;
    }
    while (n--) crc = (crc >> 8) ^ T.t[0][(crc ^ *p++) & 255u];
    return crc;
}
static unsigned png_be32(const unsigned char* p) {
    return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | (unsigned)p[3];
}
static bool png_is(const unsigned char* type, const char* name) { return memcmp(type, name, 4) == 0; }

// the size of one image's unfiltered rows in the workspace
static size_t png_raw_bytes(const int H, const int W, const int color_type, const int depth) {
    return align_up((size_t)H * (size_t)png_row_bytes(W, color_type, depth), 16);
}

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_png_parse(const unsigned char* data, size_t n, struct ssd_png_info* out) {
    static const char* const name = "ssd_png_parse";
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    SSD_CHECK_ARG(data && out, "%s: NULL pointer", name);
    memset(out, 0, sizeof(*out));
    SSD_CHECK_ARG(n >= 8 && memcmp(data, sig, 8) == 0, "%s: not a PNG signature", name);
    ssd_png_info info;
    memset(&info, 0, sizeof(info));
    const char* unsupported = nullptr;
    bool have_ihdr = false, have_plte = false, have_idat = false, idat_over = false, have_iend = false;
    size_t pos = 8;
    while (!have_iend) {
        SSD_CHECK_ARG(n - pos >= 12, "%s: the file ends inside a chunk (offset %zu)", name, pos);
        const size_t len = png_be32(data + pos);
        SSD_CHECK_ARG(len <= 0x7FFFFFFFu && len <= n - pos - 12, "%s: a chunk of %zu bytes at offset %zu runs past the file", name, len, pos);
        const unsigned char* type = data + pos + 4;
        const unsigned char* body = type + 4;
        SSD_CHECK_ARG((~png_crc_run(0xFFFFFFFFu, type, 4 + len)) == png_be32(body + len), "%s: bad CRC in the chunk at offset %zu", name, pos);
        SSD_CHECK_ARG(have_ihdr == !png_is(type, "IHDR"), "%s: IHDR is not the one first chunk", name);
        if (png_is(type, "IHDR")) {
            SSD_CHECK_ARG(len == 13, "%s: IHDR of %zu bytes", name, len);
            have_ihdr = true;
            const unsigned W = png_be32(body), H = png_be32(body + 4);
            const int depth = body[8], ct = body[9];
            SSD_CHECK_ARG(W >= 1 && H >= 1 && W <= 0x7FFFFFFFu && H <= 0x7FFFFFFFu, "%s: an image of %u x %u", name, W, H);
            SSD_CHECK_ARG(body[10] == 0 && body[11] == 0 && body[12] <= 1, "%s: compression %d, filter method %d, interlace %d", name, body[10],
                          body[11], body[12]);
            SSD_CHECK_ARG(png_format_ok(ct, depth) || (ct == 0 && depth == 16), "%s: colour type %d at depth %d", name, ct, depth);
            if (W > (unsigned)kMaxImageSide || H > (unsigned)kMaxImageSide) unsupported = "a side above 16384";
            else if (body[12] == 1) unsupported = "Adam7 interlace";
            else if (!png_format_ok(ct, depth)) unsupported = "grey at 16 bits";
            if (!unsupported) {
                info.width = (int)W; info.height = (int)H; info.depth = depth; info.color_type = ct;
                info.channels = png_channels(ct);
                info.filter_distance = png_filter_distance(ct, depth);
                info.row_bytes = png_row_bytes((int)W, ct, depth);
                info.stream_bytes = (long long)H * (1 + info.row_bytes);
            }
        } else if (png_is(type, "PLTE")) {
            SSD_CHECK_ARG(!have_plte && !have_idat, "%s: PLTE twice or behind IDAT", name);
            SSD_CHECK_ARG(len >= 3 && len <= 768 && len % 3 == 0, "%s: PLTE of %zu bytes", name, len);
            have_plte = true;
            if (!unsupported && info.color_type != 3 && info.color_type != 2 && info.color_type != 6) unsupported = "PLTE in a grey image";
            if (info.color_type == 3) {
                memcpy(info.palette, body, len);
                info.palette_entries = (int)(len / 3);
            }
        } else if (png_is(type, "IDAT")) {
            SSD_CHECK_ARG(!idat_over, "%s: IDAT chunks that are not consecutive", name);
            SSD_CHECK_ARG(unsupported || info.color_type != 3 || have_plte, "%s: colour type 3 without PLTE", name);
            if (!have_idat) info.first_idat = (long long)pos;
            have_idat = true;
            info.idat_count += 1;
            info.idat_bytes += (long long)len;
        } else if (png_is(type, "IEND")) {
            SSD_CHECK_ARG(len == 0 && have_idat, "%s: IEND of %zu bytes, or no IDAT before it", name, len);
            have_iend = true;
        } else {
            if (have_idat) idat_over = true;
            if (png_is(type, "acTL")) unsupported = "an animated PNG";
            else if (!(type[0] & 0x20) && !unsupported) unsupported = "a critical chunk this decoder does not know";
        }
        pos += 12 + len;
    }
    SSD_UNSUPPORTED_IF(unsupported != nullptr, "%s: %s", name, unsupported);
    *out = info;
    return SSD_OK;
}

extern "C" int ssd_png_idat(const unsigned char* data, size_t n, const struct ssd_png_info* info, unsigned char* out, size_t out_bytes) {
    static const char* const name = "ssd_png_idat";
    SSD_CHECK_ARG(data && info && out, "%s: NULL pointer", name);
    SSD_CHECK_ARG(info->idat_count >= 1 && info->idat_bytes >= 0 && info->first_idat >= 8 && (size_t)info->first_idat <= n, "%s: an info ssd_png_parse did not fill",
                  name);
    SSD_CHECK_ARG(out_bytes >= (size_t)info->idat_bytes, "%s: out holds %zu bytes, the stream has %lld", name, out_bytes, info->idat_bytes);
    size_t pos = (size_t)info->first_idat, at = 0;
    for (int i = 0; i < info->idat_count; ++i) {
        SSD_CHECK_ARG(n - pos >= 12, "%s: not the file that was parsed", name);
        const size_t len = png_be32(data + pos);
        SSD_CHECK_ARG(len <= n - pos - 12 && png_is(data + pos + 4, "IDAT") && len <= (size_t)info->idat_bytes - at, "%s: not the file that was parsed", name);
        memcpy(out + at, data + pos + 8, len);
        at += len;
        pos += 12 + len;
    }
    SSD_CHECK_ARG(at == (size_t)info->idat_bytes, "%s: not the file that was parsed", name);
    return SSD_OK;
}

extern "C" int ssd_png_decode_host(const struct ssd_png_info* info, const unsigned char* filtered, size_t filtered_bytes, unsigned char* rgb,
                                   size_t rgb_bytes) {
    static const char* const name = "ssd_png_decode_host";
    SSD_CHECK_ARG(info && filtered && rgb, "%s: NULL pointer", name);
    const int H = info->height, W = info->width, ct = info->color_type, depth = info->depth;
    SSD_CHECK_ARG(H >= 1 && W >= 1 && png_format_ok(ct, depth), "%s: an image of %d x %d, colour type %d at depth %d", name, H, W, ct, depth);
    SSD_UNSUPPORTED_IF(!image_side_ok(H) || !image_side_ok(W), "%s: an image of %d x %d, outside 1..%d", name, H, W, kMaxImageSide);
    const size_t rb = (size_t)png_row_bytes(W, ct, depth);
    const int fd = png_filter_distance(ct, depth);
    SSD_CHECK_ARG(filtered_bytes == (size_t)H * (rb + 1), "%s: %zu filtered bytes, the image has %zu", name, filtered_bytes, (size_t)H * (rb + 1));
    SSD_CHECK_ARG(rgb_bytes >= (size_t)H * W * 3, "%s: rgb holds %zu bytes, the image needs %zu", name, rgb_bytes, (size_t)H * W * 3);
    for (int y = 0; y < H; ++y)
        SSD_CHECK_ARG(filtered[(size_t)y * (rb + 1)] <= 4, "%s: row %d has filter type %d", name, y, filtered[(size_t)y * (rb + 1)]);
    std::vector<unsigned char> raw((size_t)H * rb);
    for (int y = 0; y < H; ++y) {
        const unsigned char* src = filtered + (size_t)y * (rb + 1);
        unsigned char* row = raw.data() + (size_t)y * rb;
        const unsigned char* up = y ? row - rb : nullptr;
        const int type = src[0];
        for (size_t i = 0; i < rb; ++i) {
            const bool left = i >= (size_t)fd;
            row[i] = (unsigned char)png_unfilter(type, src[1 + i], left ? row[i - fd] : 0, up ? up[i] : 0, (up && left) ? up[i - fd] : 0);
        }
        for (int x = 0; x < W; ++x) png_pixel_rgb(row, x, ct, depth, info->palette, rgb + ((size_t)y * W + x) * 3);
    }
    return SSD_OK;
}

extern "C" size_t ssd_png_decode_workspace_bytes(const struct ssd_png_dec_desc* desc_host, int B) {
    if (!desc_host || B <= 0 || B > 65535) return 0;
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_png_dec_desc& d = desc_host[b];
        if (!image_side_ok(d.H) || !image_side_ok(d.W) || !png_format_ok(d.color_type, d.depth)) return 0;
        total += png_raw_bytes(d.H, d.W, d.color_type, d.depth);
    }
    return total;
}

extern "C" int ssd_png_decode(const unsigned char* packed_dev, size_t packed_bytes, const struct ssd_png_dec_desc* desc_host,
                              const struct ssd_png_dec_desc* desc_dev, int B, unsigned char* rgb_dev, size_t rgb_bytes, void* workspace_dev,
                              size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "%s: bad batch", kPngDecName);
    SSD_UNSUPPORTED_IF(B > 65535, "%s: B = %d (at most 65535)", kPngDecName, B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(packed_dev && desc_host && desc_dev && rgb_dev && workspace_dev, "%s: NULL pointer", kPngDecName);
    SSD_CHECK_ARG((((size_t)packed_dev | (size_t)rgb_dev | (size_t)workspace_dev) & 15) == 0 && ((size_t)desc_dev & 7) == 0,
                  "%s: packed_dev / rgb_dev / workspace_dev are not 16-byte aligned, or desc_dev not 8-byte", kPngDecName);
    long chains = 0, rows = 0;
    size_t raw = 0, src_end = 0, dst_end = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_png_dec_desc& d = desc_host[b];
        SSD_CHECK_ARG(d.H >= 1 && d.W >= 1, "%s: image %d is %d x %d", kPngDecName, b, d.H, d.W);
        SSD_UNSUPPORTED_IF(!image_side_ok(d.H) || !image_side_ok(d.W), "%s: image %d is %d x %d, outside 1..%d", kPngDecName, b, d.H, d.W, kMaxImageSide);
        SSD_CHECK_ARG(png_format_ok(d.color_type, d.depth), "%s: image %d: colour type %d at depth %d", kPngDecName, b, d.color_type, d.depth);
        const size_t rb = (size_t)png_row_bytes(d.W, d.color_type, d.depth);
        SSD_CHECK_ARG(region_ok(d.src_offset, (size_t)d.H * (rb + 1), packed_bytes, 16, &src_end),
                      "%s: image %d: scanlines misaligned, outside packed_dev or overlapping", kPngDecName, b);
        SSD_CHECK_ARG(d.color_type != 3 || region_ok(d.palette_offset, 768, packed_bytes, 16), "%s: image %d: palette misaligned or outside packed_dev",
                      kPngDecName, b);
        SSD_CHECK_ARG(d.chains >= 1 && d.chains <= d.H && region_ok(d.chain_offset, 4 * (size_t)d.chains, packed_bytes, 16),
                      "%s: image %d: %d chains, or the list misaligned or outside packed_dev", kPngDecName, b, d.chains);
        SSD_CHECK_ARG(region_ok(d.dst_offset, (size_t)d.H * d.W * 3, rgb_bytes, 16, &dst_end),
                      "%s: image %d: pixels misaligned, outside rgb_dev or overlapping", kPngDecName, b);
        SSD_CHECK_ARG(d.chain_start == chains && d.row_start == rows && d.raw_offset == (long long)raw,
                      "%s: image %d: chain_start / row_start / raw_offset is not the running sum", kPngDecName, b);
        chains += d.chains;
        rows += d.H;
        raw += png_raw_bytes(d.H, d.W, d.color_type, d.depth);
    }
    SSD_CHECK_ARG(workspace_bytes >= raw, "%s: the workspace holds %zu bytes, the batch needs %zu", kPngDecName, workspace_bytes, raw);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = (unsigned char*)workspace_dev;
    const dim3 per_chain((unsigned)((chains + kPngDecWaves - 1) / kPngDecWaves)), waves(64 * kPngDecWaves);
    const dim3 per_row((unsigned)(rows < (1L << 20) ? rows : (1L << 20))), threads(256);
    hipLaunchKernelGGL(png_unfilter_kernel, per_chain, waves, 0, st, packed_dev, desc_dev, B, (int)chains, ws);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(png_convert_kernel, per_row, threads, 0, st, packed_dev, desc_dev, B, (int)rows, (const unsigned char*)ws, rgb_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
