// Pair IoU and box encoding shared by ssd_bbox.hip and ssd_match.hip: one definition, so "the IoU bits are ssd_iou_map's"
// holds by construction.  Both files are built with -ffp-contract=off and correctly rounded fp32 division.
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

}  // namespace ssd
