// Pair IoU and box encoding shared by ssd_bbox.hip and ssd_match.hip: one definition, so "the IoU bits are ssd_iou_map's"
// holds by construction; box decode, the NMS IoU and the score sort keys shared by ssd_bbox.hip and ssd_decode.hip.
// All three files are built with -ffp-contract=off and correctly rounded fp32 division.
#pragma once
#include <hip/hip_runtime.h>

namespace ssd {

// utils/bbox_utils.py:44-59 for one (box, gt) pair.
__device__ __forceinline__ float pair_iou(const float4 p, const float4 g) {
    const float garea = (g.z - g.x) * (g.w - g.y);
    const float parea = (p.z - p.x) * (p.w - p.y);
    const float x_top = fmaxf(p.y, g.y), y_top = fmaxf(p.x, g.x);
    const float x_bot = fminf(p.w, g.w), y_bot = fminf(p.z, g.z);
    const float inter = fmaxf(x_bot - x_top, 0.0f) * fmaxf(y_bot - y_top, 0.0f);
    const float uni = parea + garea - inter;
    return ((inter) / (uni));
}

// utils/bbox_utils.py:96-113 (M3)
__device__ __forceinline__ float4 encode_box(const float4 p, const float4 g) {
    float bw = p.w - p.y, bh = p.z - p.x;
    const float bcx = p.y + 0.5f * bw, bcy = p.x + 0.5f * bh;
    const float gw = g.w - g.y, gh = g.z - g.x;
    const float gcx = g.y + 0.5f * gw, gcy = g.x + 0.5f * gh;
    if (bw == 0.0f) bw = 1e-3f;
    if (bh == 0.0f) bh = 1e-3f;
    const float dx = gw == 0.0f ? 0.0f : ((gcx - bcx) / (bw));
    const float dy = gh == 0.0f ? 0.0f : ((gcy - bcy) / (bh));
    const float dw = gw == 0.0f ? 0.0f : logf(((gw) / (bw)));
    const float dh = gh == 0.0f ? 0.0f : logf(((gh) / (bh)));
    return make_float4(dy, dx, dh, dw);
}

// utils/bbox_utils.py:61-85 (+ models/decoder.py:41 variance scaling when USE_VAR).
__device__ __forceinline__ float4 decode_box(const float4 p, float4 d, const float4 var,
                                             const bool use_var) {
    if (use_var) { d.x = d.x * var.x; d.y = d.y * var.y; d.z = d.z * var.z; d.w = d.w * var.w; }
    const float pw = p.w - p.y;
    const float ph = p.z - p.x;
    const float pcx = p.y + 0.5f * pw;
    const float pcy = p.x + 0.5f * ph;
    const float w = expf(d.w) * pw;
    const float h = expf(d.z) * ph;
    const float cx = (d.y * pw) + pcx;
    const float cy = (d.x * ph) + pcy;
    const float y1 = cy - (0.5f * h);
    const float x1 = cx - (0.5f * w);
    return make_float4(y1, x1, h + y1, w + x1);
}

// [3P] TF CombinedNonMaxSuppression IOU helper, boxes unclipped.
__device__ __forceinline__ float nms_iou(const float4 a, const float4 b) {
    const float ymin_i = fminf(a.x, a.z), ymax_i = fmaxf(a.x, a.z);
    const float xmin_i = fminf(a.y, a.w), xmax_i = fmaxf(a.y, a.w);
    const float ymin_j = fminf(b.x, b.z), ymax_j = fmaxf(b.x, b.z);
    const float xmin_j = fminf(b.y, b.w), xmax_j = fmaxf(b.y, b.w);
    const float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
    const float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
    if (area_i <= 0.0f || area_j <= 0.0f) return 0.0f;
    const float iy = fmaxf(fminf(ymax_i, ymax_j) - fmaxf(ymin_i, ymin_j), 0.0f);
    const float ix = fmaxf(fminf(xmax_i, xmax_j) - fmaxf(xmin_i, xmin_j), 0.0f);
    const float inter = iy * ix;
    return ((inter) / (area_i + area_j - inter));
}

// Sort keys: ascending u64 order == (score desc, anchor asc[, class asc]).
__device__ __forceinline__ unsigned score_desc_key(float s) {
    const unsigned u = __float_as_uint(s);
    const unsigned asc = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    return ~asc;
}
__device__ __forceinline__ float score_from_key(unsigned k) {
    const unsigned asc = ~k;
    const unsigned u = (asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc;
    return __uint_as_float(u);
}

constexpr int kIdxBits = 22;    // N <= 4,194,304 anchors
constexpr int kClsBits = 10;    // L <= 1,024 classes

}  // namespace ssd
