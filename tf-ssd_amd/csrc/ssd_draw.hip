// Drawing detections on the device (reference utils/drawing_utils.py).  Three entry points:
//   ssd_image_minmax         per-image min / max of a float batch: the two numbers of Keras' array_to_img(scale=True)
//   ssd_draw_detections      array_to_img + the reference's PIL loop (ImageDraw.text, ImageDraw.rectangle per box) as ONE
//                            pass that writes every output byte once
//   ssd_draw_bounding_boxes  tf.image.draw_bounding_boxes (draw_bboxes)
//
// [3P] Keras array_to_img(scale=True), restated from its published source with separately rounded fp32 ops (this file is
// compiled with -ffp-contract=off and correctly rounded division): x = x - min; if (max(x) != 0) x /= max(x); x *= 255;
// astype(uint8) (truncation).  Subtraction is monotonic, so the maximum after the subtraction is fl(max - min).
//
// Pillow's drawing, reproduced to the byte (tests/drawing_cases.py holds it to Pillow itself).  The reference's loop is
// sequential (text, then frame, for each box in index order) and every write is opaque, so a pixel holds its LAST
// writer: each pixel walks the boxes from the last to the first and stops at the first one that inks it.  A box's text
// and frame share one colour, so "the frame wins over the box's own text" needs no separate rule.
//   frame  ImageDraw.rectangle((x0, y0, x1, y1), outline=c, width=w), corners inclusive, is 2w horizontal lines
//          [x0..x1] x {y0 + i, y1 - i} and 2w vertical lines at {x0 + i, x1 - i}, i < w, from y0 + w towards y1 - w + 1:
//          Pillow draws such a line in either direction and leaves its end point out.  For a box whose sides are at
//          least 2w this is the plain frame (the horizontal lines cover the row left out); thinner boxes paint outside
//          their own rectangle, and so does this kernel.
//   text   the legacy bitmap font: every printable ASCII glyph advances 6 and is 11 high; Pillow pastes each glyph's
//          ink box opaquely in string order, and a box may start one column LEFT of the glyph's origin.  A cell's
//          columns 0..4 are therefore its own glyph's, and column 5 is the next glyph's column -1 on the rows of that
//          glyph's box (when it has such a column), else its own.  The atlas (host: utils/drawing_utils.glyph_atlas)
//          holds per glyph 11 row bytes (bit k = column k - 1) and the box rows.
//
// Kernel shape: a workgroup owns a 64 x 16 pixel tile of one image.  Its 256 lanes first test the image's T boxes
// (frame minus its hole, and the text rectangle) against the tile, 64 boxes per wave and ballot, into a T-bit mask in
// LDS; no atomics, and the mask keeps the box order.  Then a lane resolves FOUR adjacent pixels of a row: 48 bytes in
// (three 16-byte loads), 12 bytes out (three dword stores), walking only the set bits from the top.  A wave covers four
// rows of 64 pixels: 768 contiguous bytes per row in, 192 out.  Rows that are not a multiple of four pixels, or
// unaligned bases, take the same path with scalar loads and stores.
#include "common.h"

namespace ssd {

static const int kDrawMaxBoxes = 4096;      // T of ssd_draw_detections (512 bytes of LDS mask)
static const int kDrawMaxText = 64;         // maxlen
static const int kDrawMaxOutline = 64;      // outline width
static const int kBBoxMaxBoxes = 1024;      // T of ssd_draw_bounding_boxes (20 KB of LDS corners)
static const int kDrawGlyphs = 96;          // 95 printable ASCII + one blank
static const int kMinMaxParts = 32;         // partial results per image

#define DRAW_TILE_W 64
#define DRAW_TILE_H 16
#define DRAW_COORD_LIMIT (1 << 24)

// ---------------------------------------------------------------------------------------------------------------------
// min / max: kMinMaxParts workgroups per image write partial results, a second tiny launch combines them in a fixed
// order (no atomics; min and max do not depend on the order anyway).  NaN pixels are ignored (fminf / fmaxf).
__global__ __launch_bounds__(256) void image_minmax_partial_kernel(const float* __restrict__ img, const long n,
                                                                  float* __restrict__ part) {
    __shared__ float smin[256], smax[256];
    const int b = blockIdx.y, p = blockIdx.x, tid = threadIdx.x;
    const float* x = img + (long)b * n;
    const long chunk = ((n + kMinMaxParts - 1) / kMinMaxParts + 3) & ~3L;
    const long lo = min((long)p * chunk, n), hi = min(lo + chunk, n);
    float mn = INFINITY, mx = -INFINITY;
    if ((reinterpret_cast<size_t>(x) & 15) == 0) {          // lo is a multiple of 4: 16-byte loads, then the tail
        const long hi4 = lo + ((hi - lo) & ~3L);
        for (long i = lo + (long)tid * 4; i < hi4; i += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            mn = fminf(fminf(mn, fminf(v.x, v.y)), fminf(v.z, v.w));
            mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
        for (long i = hi4 + tid; i < hi; i += 256) { mn = fminf(mn, x[i]); mx = fmaxf(mx, x[i]); }
    } else {
        for (long i = lo + tid; i < hi; i += 256) { mn = fminf(mn, x[i]); mx = fmaxf(mx, x[i]); }
    }
    smin[tid] = mn;
    smax[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            smin[tid] = fminf(smin[tid], smin[tid + o]);
            smax[tid] = fmaxf(smax[tid], smax[tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[((long)b * kMinMaxParts + p) * 2] = smin[0];
        part[((long)b * kMinMaxParts + p) * 2 + 1] = smax[0];
    }
}

__global__ __launch_bounds__(64) void image_minmax_combine_kernel(const float* __restrict__ part, const int B,
                                                                 float* __restrict__ minmax) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int p = 0; p < kMinMaxParts; ++p) {
        mn = fminf(mn, part[((long)b * kMinMaxParts + p) * 2]);
        mx = fmaxf(mx, part[((long)b * kMinMaxParts + p) * 2 + 1]);
    }
    minmax[b * 2] = mn;
    minmax[b * 2 + 1] = mx;
}

// ---------------------------------------------------------------------------------------------------------------------
struct DrawBox {
    int x0, y0, x1, y1;     // inclusive corners, clamped to +-2^24 (the image sides are at most 2^14)
    bool ok;                // false: the reference skips it
};

__device__ __forceinline__ int draw_clamp(const int v) { return min(max(v, -DRAW_COORD_LIMIT), DRAW_COORD_LIMIT); }

// boxes are (y1, x1, y2, x2); the reference's skip test (drawing_utils.py:63) on the unclamped values; filled squares
// (draw_grid_map) are drawn down to one pixel
__device__ __forceinline__ DrawBox draw_load_box(const int* __restrict__ q, const bool fill) {
    const int4 v = *reinterpret_cast<const int4*>(q);
    const long long w = (long long)v.w - v.y, h = (long long)v.z - v.x;
    DrawBox r;
    r.ok = fill ? (w >= 0 && h >= 0) : (w > 0 && h > 0);
    r.y0 = draw_clamp(v.x); r.x0 = draw_clamp(v.y); r.y1 = draw_clamp(v.z); r.x1 = draw_clamp(v.w);
    return r;
}

__device__ __forceinline__ bool draw_frame_pixel(const DrawBox& q, const int w, const int x, const int y) {
    const bool in_x = x >= q.x0 && x <= q.x1;
    const bool hrow = (y >= q.y0 && y < q.y0 + w) || (y > q.y1 - w && y <= q.y1);
    const bool vcol = (x >= q.x0 && x < q.x0 + w) || (x > q.x1 - w && x <= q.x1);
    const int va = q.y0 + w, vb = q.y1 - w + 1;          // drawn from va towards vb, in either direction, without vb itself
    const int lo = va < vb ? va : vb + 1, hi = va < vb ? vb - 1 : va;
    return (in_x && hrow) || (vcol && y >= lo && y <= hi);
}

__device__ __forceinline__ int draw_glyph(const unsigned char c) { return (c >= 32 && c <= 126) ? c - 32 : kDrawGlyphs - 1; }

// dx, dy inside [0, 6 * len) x [0, 11)
__device__ __forceinline__ bool draw_text_pixel(const unsigned* __restrict__ atlas, const unsigned char* __restrict__ str,
                                                const int len, const int dx, const int dy) {
    const int cell = dx / 6, col = dx - cell * 6;
    const int g = draw_glyph(str[cell]);
    const unsigned rows = (atlas[g * 4 + (dy >> 2)] >> ((dy & 3) * 8)) & 0xffu;
    if (col < 5) return (rows >> (col + 1)) & 1u;
    if (cell + 1 < len) {
        const int n = draw_glyph(str[cell + 1]);
        const unsigned meta = atlas[n * 4 + 3];
        const int r0 = (int)(meta & 0xffu), r1 = (int)((meta >> 8) & 0xffu);
        if (((meta >> 16) & 1u) && dy >= r0 && dy < r1) return (atlas[n * 4 + (dy >> 2)] >> ((dy & 3) * 8)) & 1u;
    }
    return (rows >> 6) & 1u;
}

// array_to_img's element: separately rounded fp32 ops, truncation (saturating: only unscaled input can leave 0..255)
__device__ __forceinline__ unsigned draw_to_u8(const float x, const float mn, const float range, const bool scale) {
    float v = x;
    if (scale) {
        v = x - mn;
        if (range != 0.0f) v = v / range;
        v = v * 255.0f;
    }
    return (unsigned)min(max((int)v, 0), 255);
}

__global__ __launch_bounds__(256) void draw_detections_kernel(
    const float* __restrict__ img, const float* __restrict__ minmax, const int H, const int W,
    const int* __restrict__ boxes, const int* __restrict__ labels, const unsigned char* __restrict__ text,
    const int* __restrict__ text_len, const int T, const int maxlen, const unsigned char* __restrict__ colors, const int L,
    const unsigned* __restrict__ atlas, const int width, const int fill, const int tiles_x, const int wide,
    unsigned char* __restrict__ out) {
    __shared__ unsigned long long hits[kDrawMaxBoxes / 64];
    __shared__ unsigned glyphs[kDrawGlyphs * 4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int X0 = tile_x * DRAW_TILE_W, Y0 = tile_y * DRAW_TILE_H;
    const int X1 = min(X0 + DRAW_TILE_W, W) - 1, Y1 = min(Y0 + DRAW_TILE_H, H) - 1;
    const int* bx = boxes + (long)b * T * 4;
    const int* lab = labels + (long)b * T;
    const int* tlen = text_len ? text_len + (long)b * T : nullptr;
    const unsigned char* txt = text ? text + (long)b * T * maxlen : nullptr;
    const bool with_text = !fill && txt && tlen && maxlen > 0;

    if (with_text)
        for (int i = tid; i < kDrawGlyphs * 4; i += 256) glyphs[i] = atlas[i];
    // cull: 64 boxes per wave and step, one ballot each; every word of the mask below (T + 63) / 64 is written
    for (int base = 0; base < T; base += 256) {
        const int t = base + tid;
        bool hit = false;
        if (t < T) {
            const DrawBox q = draw_load_box(bx + (long)t * 4, fill != 0);
            const int l = lab[t];
            if (q.ok && l >= 0 && l < L) {
                if (fill) {
                    hit = q.x0 <= X1 && q.x1 >= X0 && q.y0 <= Y1 && q.y1 >= Y0;
                } else {
                    const int fx0 = min(q.x0, q.x1 - width + 1), fx1 = max(q.x1, q.x0 + width - 1);
                    const int fy0 = min(q.y0, q.y1 - width + 1), fy1 = max(q.y1, q.y0 + width);
                    hit = fx0 <= X1 && fx1 >= X0 && fy0 <= Y1 && fy1 >= Y0;
                    // a tile that lies inside the frame's hole sees nothing of it
                    if (hit && X0 >= q.x0 + width && X1 <= q.x1 - width && Y0 >= q.y0 + width && Y1 <= q.y1 - width) hit = false;
                    if (!hit && with_text) {
                        const int n = min(max(tlen[t], 0), maxlen);
                        const int tx = q.x0 + 4, ty = q.y0 + 2;
                        hit = n > 0 && tx <= X1 && tx + 6 * n - 1 >= X0 && ty <= Y1 && ty + 10 >= Y0;
                    }
                }
            }
        }
        const unsigned long long m = __ballot(hit);
        if ((tid & 63) == 0) hits[(base >> 6) + (tid >> 6)] = m;
    }
    __syncthreads();

    const int y = Y0 + (tid >> 4), x = X0 + (tid & 15) * 4;
    if (y > Y1 || x > X1) return;
    const int npx = min(4, W - x);
    const long pix = ((long)b * H + y) * W + x;
    const float* src = img + pix * 3;
    float v[12];
    if (wide) {
        const float4 a = *reinterpret_cast<const float4*>(src), c = *reinterpret_cast<const float4*>(src + 4),
                     d = *reinterpret_cast<const float4*>(src + 8);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
        v[8] = d.x; v[9] = d.y; v[10] = d.z; v[11] = d.w;
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) v[j] = j < npx * 3 ? src[j] : 0.0f;
    }

    // last writer: boxes from the top, until every pixel of this lane has its ink
    int ink[4] = {-1, -1, -1, -1};
    unsigned open = (1u << npx) - 1u;
    for (int w64 = (T + 63) / 64 - 1; w64 >= 0 && open; --w64) {
        unsigned long long m = hits[w64];
        while (m && open) {
            const int bit = 63 - __clzll((long long)m);
            m &= ~(1ull << bit);
            const int t = w64 * 64 + bit;
            const DrawBox q = draw_load_box(bx + (long)t * 4, fill != 0);
            const int l = lab[t];
            unsigned got = 0;
            if (fill) {
                if (y >= q.y0 && y <= q.y1) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) got |= (unsigned)(x + j >= q.x0 && x + j <= q.x1) << j;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) got |= (unsigned)draw_frame_pixel(q, width, x + j, y) << j;
                const int dy = y - (q.y0 + 2);
                if (with_text && dy >= 0 && dy < 11 && (got & open) != open) {
                    const int n = min(max(tlen[t], 0), maxlen);
                    const int tx = q.x0 + 4;
                    if (x + 3 >= tx && x < tx + 6 * n) {
                        const unsigned char* s = txt + (long)t * maxlen;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int dx = x + j - tx;
                            if (dx >= 0 && dx < 6 * n) got |= (unsigned)draw_text_pixel(glyphs, s, n, dx, dy) << j;
                        }
                    }
                }
            }
            got &= open;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((got >> j) & 1u) ink[j] = l;
            open &= ~got;
        }
    }

    const bool scale = minmax != nullptr;
    const float mn = scale ? minmax[b * 2] : 0.0f;
    const float range = scale ? minmax[b * 2 + 1] - mn : 0.0f;
    unsigned u[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (ink[j] >= 0) {
            const unsigned char* c = colors + ink[j] * 3;
            u[j * 3] = c[0]; u[j * 3 + 1] = c[1]; u[j * 3 + 2] = c[2];
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) u[j * 3 + k] = draw_to_u8(v[j * 3 + k], mn, range, scale);
        }
    }
    unsigned char* dst = out + pix * 3;
    if (wide) {
        unsigned* d32 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k) d32[k] = u[k * 4] | (u[k * 4 + 1] << 8) | (u[k * 4 + 2] << 16) | (u[k * 4 + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < npx * 3) dst[j] = (unsigned char)u[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// [3P] tf.image.draw_bounding_boxes, restated from the TF 2.0 kernel (DrawBoundingBoxesOp): corners are
// int64(float(coord) * (size - 1)); an inverted box and a box entirely outside are skipped; each of the four 1-pixel
// edges is drawn only when that edge lies inside the image; later boxes overwrite earlier ones; the colour table is
// cycled by box index.  The corners of the image's boxes go to LDS once per workgroup.
__global__ __launch_bounds__(256) void draw_bounding_boxes_kernel(const float* __restrict__ img, const int H, const int W,
                                                                 const float* __restrict__ boxes, const int T,
                                                                 const float* __restrict__ colors, const int L,
                                                                 float* __restrict__ out) {
    __shared__ int corner[kBBoxMaxBoxes][5];       // r0, c0, r1, c1, drawn
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int t = tid; t < T; t += 256) {
        const float* q = boxes + ((long)b * T + t) * 4;
        const long long r0 = (long long)(q[0] * (float)(H - 1)), c0 = (long long)(q[1] * (float)(W - 1));
        const long long r1 = (long long)(q[2] * (float)(H - 1)), c1 = (long long)(q[3] * (float)(W - 1));
        const bool drawn = !(r0 > r1 || c0 > c1) && !(r0 >= H || r1 < 0 || c0 >= W || c1 < 0);
        const long long lim = 1 << 30;
        corner[t][0] = (int)min(max(r0, -lim), lim); corner[t][1] = (int)min(max(c0, -lim), lim);
        corner[t][2] = (int)min(max(r1, -lim), lim); corner[t][3] = (int)min(max(c1, -lim), lim);
        corner[t][4] = drawn;
    }
    __syncthreads();
    const long total = (long)H * W;
    const float* src = img + (long)b * total * 3;
    float* dst = out + (long)b * total * 3;
    for (long e = (long)blockIdx.x * 256 + tid; e < total; e += (long)gridDim.x * 256) {
        const int y = (int)(e / W), x = (int)(e - (long)y * W);
        int who = -1;
        for (int t = T - 1; t >= 0; --t) {
            if (!corner[t][4]) continue;
            const int r0 = corner[t][0], c0 = corner[t][1], r1 = corner[t][2], c1 = corner[t][3];
            const bool in_c = x >= c0 && x <= c1, in_r = y >= r0 && y <= r1;
            if (((y == r0 || y == r1) && in_c) || ((x == c0 || x == c1) && in_r)) { who = t; break; }
        }
        if (who >= 0) {
            const float* c = colors + (who % L) * 3;
            dst[e * 3] = c[0]; dst[e * 3 + 1] = c[1]; dst[e * 3 + 2] = c[2];
        } else {
            dst[e * 3] = src[e * 3]; dst[e * 3 + 1] = src[e * 3 + 1]; dst[e * 3 + 2] = src[e * 3 + 2];
        }
    }
}

}  // namespace ssd

using namespace ssd;

extern "C" size_t ssd_image_minmax_workspace_bytes(int B) {
    return B > 0 ? (size_t)B * kMinMaxParts * 2 * sizeof(float) : 0;
}

extern "C" int ssd_image_minmax(const float* img_dev, int B, int H, int W, int C, float* minmax_out_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_image_minmax: bad batch");
    SSD_UNSUPPORTED_IF(C != 3, "ssd_image_minmax: C = %d (3 only)", C);
    SSD_UNSUPPORTED_IF(!image_side_ok(H) || !image_side_ok(W), "ssd_image_minmax: image %d x %d outside 1..%d", H, W, kMaxImageSide);
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_image_minmax: B = %d (at most 65535)", B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && minmax_out_dev && workspace_dev, "ssd_image_minmax: NULL pointer");
    SSD_CHECK_ARG(workspace_bytes >= ssd_image_minmax_workspace_bytes(B) && (reinterpret_cast<size_t>(workspace_dev) & 3) == 0,
                  "ssd_image_minmax: workspace too small or misaligned");
    hipLaunchKernelGGL(image_minmax_partial_kernel, dim3(kMinMaxParts, B), dim3(256), 0, (hipStream_t)stream, img_dev,
                       (long)H * W * 3, (float*)workspace_dev);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_minmax_combine_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       (const float*)workspace_dev, B, minmax_out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_draw_detections(const float* img_dev, const float* minmax_dev, int B, int H, int W, int C,
                                   const int* boxes_dev, const int* labels_dev, const unsigned char* text_dev,
                                   const int* text_len_dev, int T, int maxlen, const unsigned char* colors_dev, int L,
                                   const unsigned* atlas_dev, int outline_width, int fill, unsigned char* out_dev,
                                   void* stream) {
    SSD_CHECK_ARG(B >= 0 && T >= 0 && maxlen >= 0 && L >= 0, "ssd_draw_detections: negative size");
    SSD_UNSUPPORTED_IF(C != 3, "ssd_draw_detections: C = %d (3 only)", C);
    SSD_UNSUPPORTED_IF(!image_side_ok(H) || !image_side_ok(W), "ssd_draw_detections: image %d x %d outside 1..%d", H, W,
                       kMaxImageSide);
    SSD_UNSUPPORTED_IF(T > kDrawMaxBoxes, "ssd_draw_detections: T = %d (at most %d)", T, kDrawMaxBoxes);
    SSD_UNSUPPORTED_IF(maxlen > kDrawMaxText, "ssd_draw_detections: maxlen = %d (at most %d)", maxlen, kDrawMaxText);
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_draw_detections: B = %d (at most 65535)", B);
    SSD_CHECK_ARG(outline_width >= 1 && outline_width <= kDrawMaxOutline, "ssd_draw_detections: outline width %d outside 1..%d",
                  outline_width, kDrawMaxOutline);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && out_dev && (const void*)img_dev != (const void*)out_dev, "ssd_draw_detections: NULL pointer / in-place call");
    if (T > 0) {
        SSD_CHECK_ARG(boxes_dev && labels_dev && colors_dev && L >= 1, "ssd_draw_detections: boxes without labels or colours");
        SSD_CHECK_ARG((reinterpret_cast<size_t>(boxes_dev) & 15) == 0, "ssd_draw_detections: boxes_dev is not 16-byte aligned");
        if (!fill && maxlen > 0)
            SSD_CHECK_ARG(text_dev && text_len_dev && atlas_dev, "ssd_draw_detections: text without lengths or atlas");
    }
    const int tiles_x = (W + DRAW_TILE_W - 1) / DRAW_TILE_W, tiles_y = (H + DRAW_TILE_H - 1) / DRAW_TILE_H;
    const int wide = (W & 3) == 0 && (reinterpret_cast<size_t>(img_dev) & 15) == 0 && (reinterpret_cast<size_t>(out_dev) & 3) == 0;
    hipLaunchKernelGGL(draw_detections_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, (hipStream_t)stream, img_dev,
                       minmax_dev, H, W, boxes_dev, labels_dev, text_dev, text_len_dev, T, maxlen, colors_dev, L, atlas_dev,
                       outline_width, fill, tiles_x, wide, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_draw_bounding_boxes(const float* img_dev, int B, int H, int W, int C, const float* boxes_dev, int T,
                                       const float* colors_dev, int L, float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && T >= 0 && L >= 0, "ssd_draw_bounding_boxes: negative size");
    SSD_UNSUPPORTED_IF(C != 3, "ssd_draw_bounding_boxes: C = %d (3 only)", C);
    SSD_UNSUPPORTED_IF(!image_side_ok(H) || !image_side_ok(W), "ssd_draw_bounding_boxes: image %d x %d outside 1..%d", H, W,
                       kMaxImageSide);
    SSD_UNSUPPORTED_IF(T > kBBoxMaxBoxes, "ssd_draw_bounding_boxes: T = %d (at most %d)", T, kBBoxMaxBoxes);
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_draw_bounding_boxes: B = %d (at most 65535)", B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && out_dev && img_dev != out_dev, "ssd_draw_bounding_boxes: NULL pointer / in-place call");
    if (T > 0) SSD_CHECK_ARG(boxes_dev && colors_dev && L >= 1, "ssd_draw_bounding_boxes: boxes without colours");
    const long blocks = ((long)H * W + 255) / 256;
    hipLaunchKernelGGL(draw_bounding_boxes_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), B), dim3(256), 0,
                       (hipStream_t)stream, img_dev, H, W, boxes_dev, T, colors_dev, L, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
