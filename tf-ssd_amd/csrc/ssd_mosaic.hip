// Mosaic augmentation (include/ssd_hip.h, "augmentation, mosaic"): four images of the batch, each resized as a whole by its
// own scale, tiled around a random centre; their ground truth moved to the tile, clipped to it, filtered by the usual
// candidate rule (2 px, 10 % of the area, aspect below 100) and merged into G_out rows with the sources' labels.
// Two kernels: the PLAN (one wavefront per output image: the draws, the tile table, the merged ground truth -- lanes take
// the source rows 64 at a time, a ballot and a prefix popcount give every kept row its output index, so the order is the
// sequential one; no atomics, no LDS, no workspace) and the PIXELS (one thread per output pixel, the four taps of
// bilinear_taps.h on the tile's source image).  The generator is ssd_augplan.hip's (philox.h) on slots of its own.
// Compiled with -ffp-contract=off and correctly rounded division: every fp32 operation rounds on its own, as in the NumPy
// restatement the tests compare with (tests/mosaic_cases.py).
#include "bilinear_taps.h"
#include "common.h"
#include "philox.h"

namespace ssd {

static const int kMosaicMaxSide = 4096, kMosaicMaxBoxes = 512, kMosaicMaxOut = 2048, kMosaicMaxBatch = 65535;
static const unsigned int kMosaicSlot = 128u;       // 128 decisions, 129 centre, 130 scales

// clip to [lo, hi]: a NaN stays a NaN (and then fails every test of the candidate rule)
__device__ __forceinline__ float clip_to(const float v, const float lo, const float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// blockIdx.x = the output image, 64 threads = one wavefront
__global__ __launch_bounds__(64) void augment_mosaic_plan_kernel(const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                                const long long* __restrict__ sample_ids, const int B, const int G,
                                                                const int H, const int W, const unsigned int key0,
                                                                const unsigned int key1, const float p, const float s_min,
                                                                const float s_max, const int G_out, const int pad_label,
                                                                int* __restrict__ plan_out, float* __restrict__ boxes_out,
                                                                int* __restrict__ labels_out, int* __restrict__ info_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const unsigned long long id = (unsigned long long)sample_ids[b];
    const unsigned int id0 = (unsigned int)id, id1 = (unsigned int)(id >> 32);
    const philox4 d0 = philox4x32_10(id0, id1, kMosaicSlot, 0u, key0, key1);
    const philox4 d1 = philox4x32_10(id0, id1, kMosaicSlot + 1u, 0u, key0, key1);
    const philox4 d2 = philox4x32_10(id0, id1, kMosaicSlot + 2u, 0u, key0, key1);

    const bool mosaic = draw_unit(d0.w[0]) < p;
    const float fh = (float)H, fw = (float)W;
    const int yc = min(max((int)(fh * (0.25f + 0.5f * draw_unit(d1.w[0]))), 1), H - 1);
    const int xc = min(max((int)(fw * (0.25f + 0.5f * draw_unit(d1.w[1]))), 1), W - 1);
    int src[4], hs[4], ws[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        src[t] = t == 0 ? b : draw_below(d0.w[t], B);
        const float s = draw_uniform(d2.w[t], s_min, s_max);
        hs[t] = max(1, (int)rintf(fh * s));
        ws[t] = max(1, (int)rintf(fw * s));
    }

    float* ob = boxes_out + (long)b * G_out * 4;
    int* ol = labels_out + (long)b * G_out;
    int kept = 0, seen = 0, written = G;
    if (mosaic) {
        const unsigned long long below_me = (1ull << lane) - 1ull;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool lower = t >= 2, right = (t & 1) != 0;
            const float top = (float)(lower ? yc : yc - hs[t]), left = (float)(right ? xc : xc - ws[t]);
            const float y_lo = lower ? (float)yc : 0.0f, y_hi = lower ? fh : (float)yc;
            const float x_lo = right ? (float)xc : 0.0f, x_hi = right ? fw : (float)xc;
            const float fhs = (float)hs[t], fws = (float)ws[t];
            const float* sb = gt_boxes + (long)src[t] * G * 4;
            const int* sl = gt_labels + (long)src[t] * G;
            for (int g0 = 0; g0 < G; g0 += 64) {
                const int g = g0 + lane;
                bool valid = false, keep = false;
                int label = 0;
                float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (g < G) {
                    label = sl[g];
                    valid = label > 0;
                }
                if (valid) {
                    const float4 v = *reinterpret_cast<const float4*>(sb + (long)g * 4);
                    const float Y1 = top + v.x * fhs, X1 = left + v.y * fws, Y2 = top + v.z * fhs, X2 = left + v.w * fws;
                    const float cy1 = clip_to(Y1, y_lo, y_hi), cx1 = clip_to(X1, x_lo, x_hi);
                    const float cy2 = clip_to(Y2, y_lo, y_hi), cx2 = clip_to(X2, x_lo, x_hi);
                    const float h = cy2 - cy1, w = cx2 - cx1, h0 = Y2 - Y1, w0 = X2 - X1;
                    keep = h >= 2.0f && w >= 2.0f && w * h >= 0.1f * (w0 * h0) && w < 100.0f * h && h < 100.0f * w;
                    o = make_float4(cy1 / fh, cx1 / fw, cy2 / fh, cx2 / fw);
                }
                const unsigned long long votes = __ballot(keep), valids = __ballot(valid);
                const int row = kept + __popcll(votes & below_me);
                if (keep && row < G_out) {
                    *reinterpret_cast<float4*>(ob + (long)row * 4) = o;
                    ol[row] = label;
                }
                kept += __popcll(votes);
                seen += __popcll(valids);
            }
        }
        written = min(kept, G_out);
    } else {        // not a mosaic: the image's own rows as they are, valid or not
        const float* sb = gt_boxes + (long)b * G * 4;
        const int* sl = gt_labels + (long)b * G;
        for (int g = lane; g < G; g += 64) {
            *reinterpret_cast<float4*>(ob + (long)g * 4) = *reinterpret_cast<const float4*>(sb + (long)g * 4);
            ol[g] = sl[g];
        }
    }
    for (int g = written + lane; g < G_out; g += 64) {      // padding: all-zero box, the padding label
        *reinterpret_cast<float4*>(ob + (long)g * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        ol[g] = pad_label;
    }
    if (lane == 0) {
        int* q = plan_out + (long)b * 16;
        q[0] = mosaic ? 1 : 0; q[1] = yc; q[2] = xc; q[3] = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) { q[4 + 3 * t] = src[t]; q[5 + 3 * t] = hs[t]; q[6 + 3 * t] = ws[t]; }
        int* o = info_out + (long)b * 4;
        o[0] = mosaic ? 1 : 0; o[1] = kept; o[2] = written; o[3] = seen;
    }
}

// one thread per output pixel (3 channels), grid-stride.  A tile whose plan row does not name an image of the batch, a
// centre on the image and a size the plan kernel can write (1 .. 2 * kMosaicMaxSide) shows the fill colour: the plan is
// device data the C entry cannot check, and nothing is read outside `img` whatever it holds.
__global__ __launch_bounds__(256) void augment_mosaic_pixels_kernel(const float* __restrict__ img, const int B, const int H,
                                                                   const int W, const int* __restrict__ plan, const float fill0,
                                                                   const float fill1, const float fill2, float* __restrict__ out) {
    const long total = (long)B * H * W;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int ox = (int)(e % W);
        const long r = e / W;
        const int oy = (int)(r % H), b = (int)(r / H);
        const int* q = plan + (long)b * 16;
        float* o = out + e * 3;
        if (!q[0]) {        // not a mosaic: copied through
            const float* x = img + e * 3;
            o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
            continue;
        }
        const int yc = q[1], xc = q[2];
        const bool lower = oy >= yc, right = ox >= xc;
        const int* tile = q + 4 + 3 * ((lower ? 2 : 0) + (right ? 1 : 0));
        const int src = tile[0], hs = tile[1], ws = tile[2];
        // the row is held to the ranges the plan kernel writes BEFORE any arithmetic on it: no difference below can wrap
        const bool sane = (unsigned)src < (unsigned)B && (unsigned)yc <= (unsigned)H && (unsigned)xc <= (unsigned)W && hs >= 1 &&
                          hs <= 2 * kMosaicMaxSide && ws >= 1 && ws <= 2 * kMosaicMaxSide;
        const int ry = sane ? oy - (lower ? yc : yc - hs) : -1, rx = sane ? ox - (right ? xc : xc - ws) : -1;
        if (sane && (unsigned)ry < (unsigned)hs && (unsigned)rx < (unsigned)ws) {
            int y0, y1, x0, x1;
            float ly, lx;
            bilinear_axis(ry, H, hs, y0, y1, ly);       // the whole source image resized to hs x ws
            bilinear_axis(rx, W, ws, x0, x1, lx);
            const float* xb = img + (long)src * H * W * 3;
            const float* tl = xb + ((long)y0 * W + x0) * 3;
            const float* tr = xb + ((long)y0 * W + x1) * 3;
            const float* bl = xb + ((long)y1 * W + x0) * 3;
            const float* br = xb + ((long)y1 * W + x1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = bilinear_blend(tl[c], tr[c], bl[c], br[c], lx, ly);
        } else {
            o[0] = fill0; o[1] = fill1; o[2] = fill2;
        }
    }
}

// [a, a + an) and [b, b + bn) share a byte
static bool ranges_overlap(const void* a, const size_t an, const void* b, const size_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bn && b0 < a0 + an;
}

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_augment_mosaic_plan(const float* gt_boxes_dev, const int* gt_labels_dev, const long long* sample_ids_dev, int B,
                                       int G, int H, int W, unsigned long long seed, float p, float s_min, float s_max, int G_out,
                                       int pad_label, int* plan_out_dev, float* boxes_out_dev, int* labels_out_dev,
                                       int* info_out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_augment_mosaic_plan: B = %d", B);
    SSD_UNSUPPORTED_IF(H < 2 || W < 2 || H > kMosaicMaxSide || W > kMosaicMaxSide,
                       "ssd_augment_mosaic_plan: %d x %d images (sides 2..%d)", H, W, kMosaicMaxSide);
    SSD_UNSUPPORTED_IF(G < 1 || G > kMosaicMaxBoxes, "ssd_augment_mosaic_plan: G = %d ground-truth rows (1..%d)", G, kMosaicMaxBoxes);
    SSD_UNSUPPORTED_IF(G_out < G || G_out > kMosaicMaxOut, "ssd_augment_mosaic_plan: G_out = %d output rows (G = %d .. %d)", G_out, G,
                       kMosaicMaxOut);
    SSD_UNSUPPORTED_IF(B > kMosaicMaxBatch, "ssd_augment_mosaic_plan: B = %d images (at most %d)", B, kMosaicMaxBatch);
    SSD_CHECK_ARG(p >= 0.0f && p <= 1.0f, "ssd_augment_mosaic_plan: p = %g outside [0, 1]", (double)p);
    SSD_CHECK_ARG(s_min >= 0.1f && s_min <= s_max && s_max <= 2.0f, "ssd_augment_mosaic_plan: scale range [%g, %g] outside 0.1 <= lo <= hi <= 2",
                  (double)s_min, (double)s_max);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(gt_boxes_dev && gt_labels_dev && sample_ids_dev && plan_out_dev && boxes_out_dev && labels_out_dev && info_out_dev,
                  "ssd_augment_mosaic_plan: NULL pointer");
    SSD_CHECK_ARG((((uintptr_t)gt_boxes_dev | (uintptr_t)boxes_out_dev) & 15) == 0, "ssd_augment_mosaic_plan: boxes are not 16-byte aligned");
    // every wave reads other images' rows: nothing is in place
    const void* ins[3] = {gt_boxes_dev, gt_labels_dev, sample_ids_dev};
    const size_t in_bytes[3] = {(size_t)B * G * 16, (size_t)B * G * 4, (size_t)B * 8};
    const void* outs[4] = {plan_out_dev, boxes_out_dev, labels_out_dev, info_out_dev};
    const size_t out_bytes[4] = {(size_t)B * 64, (size_t)B * G_out * 16, (size_t)B * G_out * 4, (size_t)B * 16};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 3; ++i)
            SSD_CHECK_ARG(!ranges_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]), "ssd_augment_mosaic_plan: an output aliases an input");
        for (int k = 0; k < o; ++k)
            SSD_CHECK_ARG(!ranges_overlap(outs[o], out_bytes[o], outs[k], out_bytes[k]), "ssd_augment_mosaic_plan: two outputs overlap");
    }
    hipLaunchKernelGGL(augment_mosaic_plan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, gt_boxes_dev, gt_labels_dev,
                       sample_ids_dev, B, G, H, W, (unsigned int)(seed & 0xffffffffull), (unsigned int)(seed >> 32), p, s_min, s_max,
                       G_out, pad_label, plan_out_dev, boxes_out_dev, labels_out_dev, info_out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

extern "C" int ssd_augment_mosaic_pixels(const float* img_dev, int B, int H, int W, const int* plan_dev, const float* fill,
                                         float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0, "ssd_augment_mosaic_pixels: B = %d", B);
    SSD_UNSUPPORTED_IF(H < 2 || W < 2 || H > kMosaicMaxSide || W > kMosaicMaxSide,
                       "ssd_augment_mosaic_pixels: %d x %d images (sides 2..%d)", H, W, kMosaicMaxSide);
    SSD_UNSUPPORTED_IF(B > kMosaicMaxBatch, "ssd_augment_mosaic_pixels: B = %d images (at most %d)", B, kMosaicMaxBatch);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(img_dev && plan_dev && fill && out_dev, "ssd_augment_mosaic_pixels: NULL pointer");
    const size_t bytes = (size_t)B * H * W * 12;
    SSD_CHECK_ARG(!ranges_overlap(out_dev, bytes, img_dev, bytes) && !ranges_overlap(out_dev, bytes, plan_dev, (size_t)B * 64),
                  "ssd_augment_mosaic_pixels: the output aliases an input");
    const long total = (long)B * H * W;
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(augment_mosaic_pixels_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0,
                       (hipStream_t)stream, img_dev, B, H, W, plan_dev, fill[0], fill[1], fill[2], out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
