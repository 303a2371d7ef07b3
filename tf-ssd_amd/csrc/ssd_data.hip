// GPU input pipeline: reference utils/data_utils.py:22-23
//     img = tf.image.convert_image_dtype(img, tf.float32)      // uint8 -> float32 * (1/255)
//     img = tf.image.resize(img, (final_height, final_width))  // bilinear, half-pixel centres
// as one HBM-bound kernel: a thread produces one output pixel (3 channels) from its 4 source
// pixels; no intermediate float image.  [3P] TF 2.x ResizeBilinear CPU kernel semantics
// (half_pixel_centers = true, antialias = false): scale = in / out (fp32);
// src = (dst + 0.5) * scale - 0.5; lower = max(floor(src), 0); upper = min(ceil(src), in - 1);
// lerp = src - floor(src); out = top + (bottom - top) * y_lerp with top = tl + (tr - tl) * x_lerp.
// Compiled with -ffp-contract=off: every multiply/add rounds separately like the reference's ops.
#include <algorithm>

#include "bilinear_taps.h"
#include "common.h"

namespace ssd {

__global__ __launch_bounds__(256) void preprocess_kernel(const unsigned char* __restrict__ img, const int B,
                                                        const int H, const int W, const int C, const int Ho,
                                                        const int Wo, float* __restrict__ out) {
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const float inv255 = (float)(1.0 / 255.0);
    const long total = (long)B * Ho * Wo;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int ox = (int)(e % Wo);
        const long r = e / Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        const float fy = ((float)oy + 0.5f) * sy - 0.5f, fx = ((float)ox + 0.5f) * sx - 0.5f;
        const float fyf = floorf(fy), fxf = floorf(fx);
        const int y0 = max((int)fyf, 0), y1 = min((int)ceilf(fy), H - 1);
        const int x0 = max((int)fxf, 0), x1 = min((int)ceilf(fx), W - 1);
        const float ly = fy - fyf, lx = fx - fxf;
        const unsigned char* base = img + (long)b * H * W * C;
        const unsigned char *ptl = base + ((long)y0 * W + x0) * C, *ptr_ = base + ((long)y0 * W + x1) * C;
        const unsigned char *pbl = base + ((long)y1 * W + x0) * C, *pbr = base + ((long)y1 * W + x1) * C;
        float* o = out + e * C;
        for (int c = 0; c < C; ++c) {
            const float tl = (float)ptl[c] * inv255, tr = (float)ptr_[c] * inv255;
            const float bl = (float)pbl[c] * inv255, br = (float)pbr[c] * inv255;
            const float top = tl + (tr - tl) * lx;
            const float bot = bl + (br - bl) * lx;
            o[c] = top + (bot - top) * ly;
        }
    }
}

// The ragged form of preprocess_kernel: B images of different sizes, packed in one buffer, in ONE launch (blockIdx.y is the
// image, its size comes from the device descriptor).  Per output value the arithmetic is preprocess_kernel's, expression
// for expression, so image b's result is bitwise what ssd_preprocess(B = 1) writes for it.  A thread owns FOUR consecutive
// floats of the image's output (channel-interleaved, so they belong to at most two neighbouring pixels): one aligned
// 16-byte store per thread, a wave writes 1 KiB contiguous along the output rows.  The taps are byte loads; neighbouring
// lanes read neighbouring source bytes (L1 / L2 hits on lines fetched once).
struct bilinear_taps {
    int tl, tr, bl, br;     // byte offsets of the four source pixels
    float lx, ly;
};

__device__ __forceinline__ bilinear_taps preprocess_taps(const int pix, const int W, const int H, const int Wo, const float sy,
                                                         const float sx) {
    const int oy = pix / Wo, ox = pix - oy * Wo;
    const float fy = ((float)oy + 0.5f) * sy - 0.5f, fx = ((float)ox + 0.5f) * sx - 0.5f;
    const float fyf = floorf(fy), fxf = floorf(fx);
    const int y0 = max((int)fyf, 0), y1 = min((int)ceilf(fy), H - 1);
    const int x0 = max((int)fxf, 0), x1 = min((int)ceilf(fx), W - 1);
    bilinear_taps t;
    t.tl = (y0 * W + x0) * 3; t.tr = (y0 * W + x1) * 3;       // < 16384 * 16384 * 3 < 2^31 (host check)
    t.bl = (y1 * W + x0) * 3; t.br = (y1 * W + x1) * 3;
    t.lx = fx - fxf; t.ly = fy - fyf;
    return t;
}

__global__ __launch_bounds__(256) void preprocess_ragged_kernel(const unsigned char* __restrict__ src,
                                                               const ssd_image_desc* __restrict__ desc, const int Ho,
                                                               const int Wo, float* __restrict__ out) {
    const ssd_image_desc d = desc[blockIdx.y];
    const int H = d.H, W = d.W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const float inv255 = (float)(1.0 / 255.0);
    const int npix = Ho * Wo, n = npix * 3;                     // floats of one output image (< 2^31: host check)
    const int items = (n + 3) >> 2;
    const unsigned char* img = src + d.src_offset;
    float* o = out + (long)blockIdx.y * n;
    const bool wide = (reinterpret_cast<size_t>(o) & 15) == 0;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < items; e += gridDim.x * 256) {
        const int i0 = e * 4;
        const int p0 = i0 / 3, c0 = i0 - p0 * 3;
        const bilinear_taps ta = preprocess_taps(p0, W, H, Wo, sy, sx);
        const bilinear_taps tb = preprocess_taps(min(p0 + 1, npix - 1), W, H, Wo, sy, sx);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool second = c0 + j >= 3;                    // the value belongs to pixel p0 + 1
            const int c = second ? c0 + j - 3 : c0 + j;
            const bilinear_taps& t = second ? tb : ta;
            const float tl = (float)img[t.tl + c] * inv255, tr = (float)img[t.tr + c] * inv255;
            const float bl = (float)img[t.bl + c] * inv255, br = (float)img[t.br + c] * inv255;
            const float top = tl + (tr - tl) * t.lx;
            const float bot = bl + (br - bl) * t.lx;
            v[j] = top + (bot - top) * t.ly;
        }
        if (wide && i0 + 4 <= n) {
            *reinterpret_cast<float4*>(o + i0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) o[i0 + j] = v[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Augmentation (reference augmentation.py, used at trainer.py:42), the deterministic pieces with the random draws as
// inputs: per-channel image mean (expand's fill colour, contrast's pivot), the geometric chain expand -> crop -> bilinear
// resize -> horizontal flip as ONE gather kernel over a virtual canvas, and the photometric chain brightness -> contrast
// -> hue -> saturation -> clip as one elementwise kernel.  Same per-op fp32 rounding as the oracle (oracle/augment_oracle.py;
// this file is compiled with -ffp-contract=off).

// mean[b][c] over H*W of (img + add[b]): one workgroup per image, float64 partial sums in a fixed order (deterministic)
__global__ __launch_bounds__(1024) void image_mean_kernel(const float* __restrict__ img, const int HW, const int C,
                                                         const float* __restrict__ add, float* __restrict__ mean) {
    __shared__ double red[1024];
    const int b = blockIdx.x;
    const float* x = img + (long)b * HW * C;
    const float a = add ? add[b] : 0.0f;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int i = threadIdx.x; i < HW; i += 1024) s += (double)(x[(long)i * C + c] + a);
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) mean[b * C + c] = (float)(red[0] / (double)HW);
        __syncthreads();
    }
}

// params[b] = {canvas_h, canvas_w, pad_top, pad_left, crop_y, crop_x, crop_h, crop_w, flip, use_crop}: the image sits at
// (pad_top, pad_left) of a canvas_h x canvas_w canvas filled with fill[b][c]; the window (crop_y, crop_x, crop_h, crop_w)
// of that canvas is resized (bilinear, half-pixel centres) to H x W, then flipped left-right.  use_crop 0: flip only.
__global__ __launch_bounds__(256) void augment_geometry_kernel(const float* __restrict__ img, const int B, const int H,
                                                              const int W, const int C, const int Ho, const int Wo,
                                                              const int* __restrict__ params, const float* __restrict__ fill,
                                                              float* __restrict__ out) {
    const long total = (long)B * Ho * Wo;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int ox = (int)(e % Wo);
        const long r = e / Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        const int* q = params + b * 10;
        const int pad_top = q[2], pad_left = q[3], cy = q[4], cx = q[5], ch = q[6], cw = q[7];
        const int sx = q[8] ? Wo - 1 - ox : ox;
        const float* xb = img + (long)b * H * W * C;
        float* o = out + e * C;
        if (!q[9]) {        // flip only: Ho == H, Wo == W is the caller's contract (include/ssd_hip.h) -- the params are on
                            // the device, the C entry cannot check it
            for (int c = 0; c < C; ++c) o[c] = xb[((long)oy * W + sx) * C + c];
            continue;
        }
        int y0, y1, x0, x1;
        float ly, lx;
        bilinear_axis(oy, ch, Ho, y0, y1, ly);      // bilinear_taps.h: shared with the mosaic pixels
        bilinear_axis(sx, cw, Wo, x0, x1, lx);
        // canvas -> image coordinates; outside the image the canvas holds the fill colour
        const int iy0 = cy + y0 - pad_top, iy1 = cy + y1 - pad_top, ix0 = cx + x0 - pad_left, ix1 = cx + x1 - pad_left;
        const bool vy0 = (unsigned)iy0 < (unsigned)H, vy1 = (unsigned)iy1 < (unsigned)H;
        const bool vx0 = (unsigned)ix0 < (unsigned)W, vx1 = (unsigned)ix1 < (unsigned)W;
        for (int c = 0; c < C; ++c) {
            const float f = fill[b * C + c];
            const float tl = (vy0 && vx0) ? xb[((long)iy0 * W + ix0) * C + c] : f;
            const float tr = (vy0 && vx1) ? xb[((long)iy0 * W + ix1) * C + c] : f;
            const float bl = (vy1 && vx0) ? xb[((long)iy1 * W + ix0) * C + c] : f;
            const float br = (vy1 && vx1) ? xb[((long)iy1 * W + ix1) * C + c] : f;
            o[c] = bilinear_blend(tl, tr, bl, br, lx, ly);
        }
    }
}

__device__ __forceinline__ void rgb_to_hsv(const float r, const float g, const float b, float& h, float& s, float& v) {
    v = fmaxf(fmaxf(r, g), b);
    const float mn = fminf(fminf(r, g), b);
    const float range = v - mn;
    s = v > 0.0f ? range / v : 0.0f;
    const float norm = range > 0.0f ? 1.0f / (6.0f * range) : 0.0f;
    const float two6 = (float)(2.0 / 6.0), four6 = (float)(4.0 / 6.0);
    h = r == v ? norm * (g - b) : (g == v ? norm * (b - r) + two6 : norm * (r - g) + four6);
    h = range > 0.0f ? h : 0.0f;
    h = h < 0.0f ? h + 1.0f : h;
}
__device__ __forceinline__ void hsv_to_rgb(const float h, const float s, const float v, float& r, float& g, float& b) {
    const float c = s * v;
    const float m = v - c;
    const float dh = h * 6.0f;
    float f = dh;
    while (f >= 2.0f) f -= 2.0f;
    const float x = c * (1.0f - fabsf(f - 1.0f));
    const int hc = (int)floorf(dh);
    float rr = c, gg = 0.0f, bb = x;             // category 5 (and beyond)
    if (hc == 0) { rr = c; gg = x; bb = 0.0f; }
    else if (hc == 1) { rr = x; gg = c; bb = 0.0f; }
    else if (hc == 2) { rr = 0.0f; gg = c; bb = x; }
    else if (hc == 3) { rr = 0.0f; gg = x; bb = c; }
    else if (hc == 4) { rr = x; gg = 0.0f; bb = c; }
    r = rr + m; g = gg + m; b = bb + m;
}

// in place on RGB float images; params[b] = {brightness delta, contrast factor, hue delta, saturation factor}, flags[b] bits
// 0..3 say which of the four run (reference order), mean[b][3] = per-channel mean of the image contrast pivots on (the
// brightness-adjusted image: image_mean_kernel with add = delta); always ends with clip to [0,1]
__global__ __launch_bounds__(256) void augment_color_kernel(float* __restrict__ img, const int B, const long HW,
                                                           const float* __restrict__ params, const int* __restrict__ flags,
                                                           const float* __restrict__ mean) {
    const long total = (long)B * HW;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int b = (int)(e / HW);
        const float* q = params + b * 4;
        const int fl = flags[b];
        float* p = img + e * 3;
        float r = p[0], g = p[1], bl = p[2];
        if (fl & 1) { r = r + q[0]; g = g + q[0]; bl = bl + q[0]; }
        if (fl & 2) {
            const float* m = mean + b * 3;
            r = (r - m[0]) * q[1] + m[0];
            g = (g - m[1]) * q[1] + m[1];
            bl = (bl - m[2]) * q[1] + m[2];
        }
        if (fl & 4) {
            float h, s, v;
            rgb_to_hsv(r, g, bl, h, s, v);
            h = h + q[2];
            h = h < 0.0f ? h + 1.0f : h;
            h = h >= 1.0f ? h - 1.0f : h;
            hsv_to_rgb(h, s, v, r, g, bl);
        }
        if (fl & 8) {
            float h, s, v;
            rgb_to_hsv(r, g, bl, h, s, v);
            s = fminf(fmaxf(s * q[3], 0.0f), 1.0f);
            hsv_to_rgb(h, s, v, r, g, bl);
        }
        p[0] = fminf(fmaxf(r, 0.0f), 1.0f);
        p[1] = fminf(fmaxf(g, 0.0f), 1.0f);
        p[2] = fminf(fmaxf(bl, 0.0f), 1.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Custom images (reference utils/data_utils.py:93-108: PIL Image.resize(..., Image.LANCZOS), then convert_image_dtype).
// [3P] Pillow's 8-bit resampler, bit for bit: two separable passes in 22-bit fixed point, int32 accumulators, a uint8
// image between the passes; coefficient tables from the host (float64 there, like Pillow's).  One launch per pass covers
// a ragged batch: blockIdx.y is the image, blockIdx.x strides over its (row, 4 output bytes) items.  A thread owns FOUR
// consecutive bytes of an output row (channel-interleaved, so 1 1/3 pixels): the intermediate rows are padded to a
// multiple of 4 bytes, every store of the horizontal pass and every load of the vertical pass is one aligned dword, and a
// wave reads / writes 256 contiguous bytes per instruction.  The horizontal pass gathers its taps with byte loads at
// stride 3: neighbouring lanes' windows overlap almost entirely, so these are L1 hits on lines fetched once.

__device__ __forceinline__ int lanczos_clip8(const int acc) { return min(max(acc >> 22, 0), 255); }

__global__ __launch_bounds__(256) void lanczos_horizontal_kernel(const unsigned char* __restrict__ src,
                                                                const int* __restrict__ tables,
                                                                const ssd_resize_desc* __restrict__ desc, const int out_w,
                                                                const int pitch, unsigned char* __restrict__ tmp) {
    const ssd_resize_desc d = desc[blockIdx.y];
    if (d.W == out_w) return;                                   // pass skipped: the vertical pass reads the source
    const int W = d.W, rowb = out_w * 3, qpr = pitch >> 2;
    const long total = (long)d.H * qpr;
    const unsigned char* img = src + d.src_offset;
    unsigned char* dst = tmp + d.tmp_offset;
    const int* bounds = tables + d.h_bounds;
    const int* kk = tables + d.h_k;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int y = (int)(e / qpr), q = (int)(e - (long)y * qpr);
        const unsigned char* row = img + (long)y * W * 3;
        unsigned packed = 0;                                    // bytes past the row's end (padding) are written as 0
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = q * 4 + j;
            if (i < rowb) {
                const int ox = i / 3, c = i - ox * 3;
                const int xmin = min(max(bounds[ox * 2], 0), W);
                const int xmax = min(min(max(bounds[ox * 2 + 1], 0), W - xmin), d.h_ksize);   // clipped to the image
                const int* k = kk + (long)ox * d.h_ksize;
                const unsigned char* p = row + xmin * 3 + c;
                int acc = 1 << 21;
                for (int x = 0; x < xmax; ++x) acc += (int)p[x * 3] * k[x];
                packed |= (unsigned)lanczos_clip8(acc) << (8 * j);
            }
        }
        *reinterpret_cast<unsigned*>(dst + (long)y * pitch + q * 4) = packed;
    }
}

// vertical pass + epilogue.  Input: the intermediate (pitch bytes per row) or, when the horizontal pass was skipped, the
// source itself (W == out_w; dword loads only when its rows happen to be 4-byte aligned).  H == out_h: the pass is skipped,
// i.e. the one tap (row oy, weight 2^22) that leaves the byte as it is.
__global__ __launch_bounds__(256) void lanczos_vertical_kernel(const unsigned char* __restrict__ src,
                                                              const int* __restrict__ tables,
                                                              const ssd_resize_desc* __restrict__ desc, const int out_h,
                                                              const int out_w, const int pitch,
                                                              const unsigned char* __restrict__ tmp, float* __restrict__ out,
                                                              unsigned char* __restrict__ out_u8) {
    const int b = blockIdx.y;
    const ssd_resize_desc d = desc[b];
    const bool hpass = d.W != out_w, vpass = d.H != out_h;
    const unsigned char* in = hpass ? tmp + d.tmp_offset : src + d.src_offset;
    const int rowb = out_w * 3, qpr = pitch >> 2;
    const int in_pitch = hpass ? pitch : rowb;
    const bool wide_in = (in_pitch & 3) == 0 && (reinterpret_cast<size_t>(in) & 3) == 0;
    const long total = (long)out_h * qpr;
    float* o = out + (long)b * out_h * rowb;
    unsigned char* o8 = out_u8 ? out_u8 + (long)b * out_h * rowb : nullptr;
    const bool wide_out = (rowb & 3) == 0 && (reinterpret_cast<size_t>(o) & 15) == 0;
    const int* bounds = tables + d.v_bounds;
    const int* kk = tables + d.v_k;
    const float inv255 = (float)(1.0 / 255.0);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int oy = (int)(e / qpr), q = (int)(e - (long)oy * qpr);
        const int i0 = q * 4, n = min(4, rowb - i0);            // n: bytes of this item inside the row
        int ymin = oy, ymax = 1;
        const int* k = nullptr;
        if (vpass) {
            ymin = min(max(bounds[oy * 2], 0), d.H);
            ymax = min(min(max(bounds[oy * 2 + 1], 0), d.H - ymin), d.v_ksize);               // clipped to the image
            k = kk + (long)oy * d.v_ksize;
        }
        const unsigned char* p = in + (long)ymin * in_pitch + i0;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
        for (int y = 0; y < ymax; ++y, p += in_pitch) {
            unsigned v;
            if (wide_in) {
                v = *reinterpret_cast<const unsigned*>(p);
            } else {
                v = p[0];
                if (n > 1) v |= (unsigned)p[1] << 8;
                if (n > 2) v |= (unsigned)p[2] << 16;
                if (n > 3) v |= (unsigned)p[3] << 24;
            }
            const int kv = vpass ? k[y] : (1 << 22);
            a0 += (int)(v & 255u) * kv;
            a1 += (int)((v >> 8) & 255u) * kv;
            a2 += (int)((v >> 16) & 255u) * kv;
            a3 += (int)(v >> 24) * kv;
        }
        const int u[4] = {lanczos_clip8(a0), lanczos_clip8(a1), lanczos_clip8(a2), lanczos_clip8(a3)};
        float* po = o + (long)oy * rowb + i0;
        if (wide_out) {
            *reinterpret_cast<float4*>(po) = make_float4((float)u[0] * inv255, (float)u[1] * inv255, (float)u[2] * inv255,
                                                         (float)u[3] * inv255);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) po[j] = (float)u[j] * inv255;
        }
        if (o8) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) o8[(long)oy * rowb + i0 + j] = (unsigned char)u[j];
        }
    }
}

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_image_mean(const float* img_dev, int B, int H, int W, int C, const float* add_dev, float* mean_out_dev,
                              void* stream) {
    SSD_CHECK_ARG(B >= 0 && H >= 1 && W >= 1 && C >= 1 && C <= 16, "ssd_image_mean: bad sizes");
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && mean_out_dev, "ssd_image_mean: NULL pointer");
    hipLaunchKernelGGL(image_mean_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, img_dev, H * W, C, add_dev, mean_out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_augment_geometry(const float* img_dev, int B, int H, int W, int C, int out_h, int out_w,
                                    const int* params_dev, const float* fill_dev, float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && H >= 1 && W >= 1 && C >= 1 && out_h >= 1 && out_w >= 1, "ssd_augment_geometry: bad sizes");
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && params_dev && fill_dev && out_dev && img_dev != out_dev, "ssd_augment_geometry: NULL pointer / in-place call");
    const long total = (long)B * out_h * out_w;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(augment_geometry_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0,
                       (hipStream_t)stream, img_dev, B, H, W, C, out_h, out_w, params_dev, fill_dev, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_augment_color(float* img_dev, int B, int H, int W, const float* params_dev, const int* flags_dev,
                                 const float* mean_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && H >= 1 && W >= 1, "ssd_augment_color: bad sizes");
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && params_dev && flags_dev && mean_dev, "ssd_augment_color: NULL pointer");
    const long total = (long)B * H * W;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(augment_color_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0,
                       (hipStream_t)stream, img_dev, B, (long)H * W, params_dev, flags_dev, mean_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_preprocess(const unsigned char* image_u8_dev, int B, int H, int W, int C, int out_h, int out_w,
                              float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && H >= 1 && W >= 1 && C >= 1 && out_h >= 1 && out_w >= 1, "ssd_preprocess: bad sizes");
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(image_u8_dev && out_dev, "ssd_preprocess: NULL pointer");
    const long total = (long)B * out_h * out_w;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0,
                       (hipStream_t)stream, image_u8_dev, B, H, W, C, out_h, out_w, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_preprocess_ragged(const unsigned char* src_dev, size_t src_bytes, const struct ssd_image_desc* desc_host,
                                     const struct ssd_image_desc* desc_dev, int B, int C, int out_h, int out_w,
                                     float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_preprocess_ragged: bad batch");
    SSD_UNSUPPORTED_IF(C != 3, "ssd_preprocess_ragged: C = %d (3 only)", C);
    SSD_UNSUPPORTED_IF(!image_side_ok(out_h) || !image_side_ok(out_w), "ssd_preprocess_ragged: output %d x %d outside 1..%d",
                       out_h, out_w, kMaxImageSide);
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_preprocess_ragged: B = %d (at most 65535)", B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(src_dev && desc_host && desc_dev && out_dev, "ssd_preprocess_ragged: NULL pointer");
    for (int b = 0; b < B; ++b) {
        const ssd_image_desc& d = desc_host[b];
        SSD_UNSUPPORTED_IF(!image_side_ok(d.H) || !image_side_ok(d.W), "ssd_preprocess_ragged: image %d is %d x %d, outside 1..%d",
                           b, d.H, d.W, kMaxImageSide);
        SSD_CHECK_ARG(d.src_offset >= 0 && (d.src_offset & 15) == 0, "ssd_preprocess_ragged: image %d: offset not a multiple of 16", b);
        SSD_CHECK_ARG(region_ok(d.src_offset, (size_t)d.H * d.W * 3, src_bytes, 16),
                      "ssd_preprocess_ragged: image %d lies outside the source buffer", b);
    }
    const long items = ((long)out_h * out_w * 3 + 3) / 4;
    const long blocks = (items + 255) / 256;
    hipLaunchKernelGGL(preprocess_ragged_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192), B), dim3(256), 0,
                       (hipStream_t)stream, src_dev, desc_dev, out_h, out_w, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_resize_lanczos_pitch(int out_w) { return image_side_ok(out_w) ? (out_w * 3 + 3) & ~3 : 0; }

extern "C" size_t ssd_resize_lanczos_workspace_bytes(const struct ssd_resize_desc* desc_host, int B, int out_h, int out_w) {
    if (!desc_host || B <= 0 || !image_side_ok(out_h) || !image_side_ok(out_w)) return 0;
    const size_t pitch = (size_t)ssd_resize_lanczos_pitch(out_w);
    size_t total = 0;
    for (int b = 0; b < B; ++b)
        if (desc_host[b].W != out_w && image_side_ok(desc_host[b].H)) total += align_up((size_t)desc_host[b].H * pitch, 16);
    return total;
}

extern "C" int ssd_resize_lanczos(const unsigned char* src_dev, size_t src_bytes, const int* tables_dev, size_t tables_ints,
                                  const struct ssd_resize_desc* desc_host, const struct ssd_resize_desc* desc_dev, int B,
                                  int C, int out_h, int out_w, float* out_dev, unsigned char* out_u8_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_resize_lanczos: bad batch");
    SSD_UNSUPPORTED_IF(C != 3, "ssd_resize_lanczos: C = %d (3 only)", C);
    SSD_UNSUPPORTED_IF(!image_side_ok(out_h) || !image_side_ok(out_w), "ssd_resize_lanczos: output %d x %d outside 1..%d",
                       out_h, out_w, kMaxImageSide);
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_resize_lanczos: B = %d (at most 65535)", B);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(src_dev && tables_dev && desc_host && desc_dev && out_dev, "ssd_resize_lanczos: NULL pointer");
    const int pitch = ssd_resize_lanczos_pitch(out_w);
    const long qpr = pitch >> 2;
    long h_items = 0;
    size_t tmp_end = 0;
    for (int b = 0; b < B; ++b) {
        const ssd_resize_desc& d = desc_host[b];
        SSD_UNSUPPORTED_IF(!image_side_ok(d.H) || !image_side_ok(d.W), "ssd_resize_lanczos: image %d is %d x %d, outside 1..%d",
                           b, d.H, d.W, kMaxImageSide);
        SSD_CHECK_ARG(region_ok(d.src_offset, (size_t)d.H * d.W * 3, src_bytes, 1),
                      "ssd_resize_lanczos: image %d lies outside the source buffer", b);
        if (d.W != out_w) {
            SSD_CHECK_ARG(d.h_ksize >= 1 && d.h_bounds >= 0 && (size_t)d.h_bounds + (size_t)out_w * 2 <= tables_ints &&
                              d.h_k >= 0 && (size_t)d.h_k + (size_t)out_w * d.h_ksize <= tables_ints,
                          "ssd_resize_lanczos: image %d: horizontal tables lie outside tables_dev", b);
            SSD_CHECK_ARG(workspace_dev && region_ok(d.tmp_offset, (size_t)d.H * pitch, workspace_bytes, 16, &tmp_end),
                          "ssd_resize_lanczos: image %d: intermediate outside the workspace, misaligned or overlapping", b);
            h_items = std::max(h_items, (long)d.H * qpr);
        }
        if (d.H != out_h)
            SSD_CHECK_ARG(d.v_ksize >= 1 && d.v_bounds >= 0 && (size_t)d.v_bounds + (size_t)out_h * 2 <= tables_ints &&
                              d.v_k >= 0 && (size_t)d.v_k + (size_t)out_h * d.v_ksize <= tables_ints,
                          "ssd_resize_lanczos: image %d: vertical tables lie outside tables_dev", b);
    }
    if (h_items > 0) {
        const long blocks = (h_items + 255) / 256;
        hipLaunchKernelGGL(lanczos_horizontal_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192), B), dim3(256), 0,
                           (hipStream_t)stream, src_dev, tables_dev, desc_dev, out_w, pitch, (unsigned char*)workspace_dev);
        SSD_LAUNCH_CHECK();
    }
    const long blocks = ((long)out_h * qpr + 255) / 256;
    hipLaunchKernelGGL(lanczos_vertical_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192), B), dim3(256), 0,
                       (hipStream_t)stream, src_dev, tables_dev, desc_dev, out_h, out_w, pitch,
                       (const unsigned char*)workspace_dev, out_dev, out_u8_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
