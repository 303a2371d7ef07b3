// IoU-family localisation losses (IoU / GIoU / DIoU / CIoU) on the boxes decoded from the deltas, in place of the Huber
// term of ssd_loss.hip / ssd_focal.hip: ssd_iou_loc_loss in include/ssd_hip.h states the arithmetic.
//
// Parallel over anchors on a grid of (256-anchor tile, image), one anchor per lane.  A lane reads its two delta rows and
// its prior row as one 16-byte load each and writes its gradient row as one 16-byte store; nothing is staged in LDS (a
// row is used by one lane only, and the whole call moves a few megabytes).  Two launches, because an anchor's gradient
// is divided by the image's positive count:
//   iou_partial_kernel   per (image, tile): loss sum and positive count -> workspace; per_anchor_out
//   iou_finish_kernel    every workgroup adds its image's partials in tile order (the fixed tree of loss_reduce.h, so the
//                        same bits in every workgroup and at every grid size), tile 0 writes loc_loss[b], every lane
//                        evaluates its anchor again, now with the derivatives, and writes its scaled gradient row
// No floating-point atomics; an anchor's values depend on its own rows and on the image's positive count alone.
#include "common.h"
#include "loss_reduce.h"

namespace ssd {

constexpr int kIouThreads = 256;          // anchors per workgroup (ssd_iou_loc_loss_tile)
constexpr int kIouWaves = kIouThreads / 64;
constexpr float kIouEps = 1e-7f;
constexpr float kFourOverPiSq = 0.40528473456935108578f;        // 4 / pi^2

struct IouPartial {
    float sum;      // the tile's positives' per-anchor losses
    int pos;
};

struct IouParams {
    const float4* priors;   // [N]
    float4 var;
    const float4* yd;       // actual_deltas [B,N]
    const float4* pd;       // pred_deltas   [B,N]
    int B, N, mode, tiles;
    float loc_alpha;
    float* loc_loss;        // [B] (nullable)
    float* per_anchor;      // [B,N] (nullable)
    float4* grad;           // [B,N] (nullable)
    float grad_scale;
    IouPartial* part;       // workspace [B][tiles]
};

struct Box {
    float y1, x1, y2, x2;
    float h, w;             // the decoded sizes exp(d * var) * prior size (y2 = h + y1, x2 = w + x1)
};

// utils/bbox_utils.py:61-85 on deltas * variances (models/decoder.py:41): box_math.h's decode_box, the sizes kept
__device__ __forceinline__ Box decode(const float4 p, const float4 d, const float4 var, float& ph, float& pw) {
#pragma clang fp contract(off)
    const float dy = d.x * var.x, dx = d.y * var.y, dh = d.z * var.z, dw = d.w * var.w;
    pw = p.w - p.y;
    ph = p.z - p.x;
    const float pcx = p.y + 0.5f * pw;
    const float pcy = p.x + 0.5f * ph;
    Box b;
    b.w = expf(dw) * pw;
    b.h = expf(dh) * ph;
    const float cx = (dx * pw) + pcx;
    const float cy = (dy * ph) + pcy;
    b.y1 = cy - (0.5f * b.h);
    b.x1 = cx - (0.5f * b.w);
    b.y2 = b.h + b.y1;
    b.x2 = b.w + b.x1;
    return b;
}

// One positive anchor: its loss, and with GRAD the derivative of that loss w.r.t. the anchor's four predicted deltas
// (not yet scaled).  min / max pass the derivative to the PREDICTION's coordinate at a tie, max(x, 0) passes it where
// x > 0, CIoU's weight a is a constant.
template <bool GRAD>
__device__ __forceinline__ float iou_anchor(const float4 prior, const float4 var, const float4 td, const float4 od,
                                            const int mode, float4& grad) {
#pragma clang fp contract(off)
    float ph, pw;
    const Box t = decode(prior, td, var, ph, pw);
    const Box b = decode(prior, od, var, ph, pw);
    const float ihr = fminf(b.y2, t.y2) - fmaxf(b.y1, t.y1);
    const float iwr = fminf(b.x2, t.x2) - fmaxf(b.x1, t.x1);
    const float ih = fmaxf(ihr, 0.f), iw = fmaxf(iwr, 0.f);
    const float inter = ih * iw;
    const float hb = b.y2 - b.y1, wb = b.x2 - b.x1;
    const float ht = t.y2 - t.y1, wt = t.x2 - t.x1;
    const float uni = (hb * wb + ht * wt) - inter;
    const float U = uni + kIouEps;
    const float iou = inter / U;
    const float ch = fmaxf(b.y2, t.y2) - fminf(b.y1, t.y1);
    const float cw = fmaxf(b.x2, t.x2) - fminf(b.x1, t.x1);
    float l = 1.0f - iou;
    // derivatives of l w.r.t. inter, the prediction's area, ch, cw, the prediction's centre (y, x), hb, wb
    float g_inter = 0.f, g_area = 0.f, g_ch = 0.f, g_cw = 0.f, g_cy = 0.f, g_cx = 0.f, g_hb = 0.f, g_wb = 0.f;
    if (GRAD) {
        g_inter = -((1.0f + iou) / U);      // iou = inter / (area_b + area_t - inter + eps)
        g_area = iou / U;
    }
    if (mode == SSD_LOC_GIOU) {
        const float ac = ch * cw;
        const float A = ac + kIouEps;
        l = 1.0f - (iou - (ac - uni) / A);
        if (GRAD) {
            const float rA = 1.0f / A;
            g_inter = g_inter + rA;          // (ac - union) / A: d/d union = -1 / A, d union / d inter = -1
            g_area = g_area - rA;
            const float g_ac = U / (A * A);
            g_ch = g_ac * cw;
            g_cw = g_ac * ch;
        }
    } else if (mode == SSD_LOC_DIOU || mode == SSD_LOC_CIOU) {
        const float dyc = (b.y1 + b.y2) * 0.5f - (t.y1 + t.y2) * 0.5f;
        const float dxc = (b.x1 + b.x2) * 0.5f - (t.x1 + t.x2) * 0.5f;
        const float rho2 = dyc * dyc + dxc * dxc;
        const float c2 = (ch * ch + cw * cw) + kIouEps;
        const float pen = rho2 / c2;
        l = l + pen;
        if (GRAD) {
            const float g_c2 = -(pen / c2);
            g_ch = g_c2 * (2.0f * ch);
            g_cw = g_c2 * (2.0f * cw);
            g_cy = (2.0f * dyc) / c2;
            g_cx = (2.0f * dxc) / c2;
        }
        if (mode == SSD_LOC_CIOU) {
            const float d = atanf(wt / ht) - atanf(wb / hb);
            const float v = kFourOverPiSq * (d * d);
            const float a = v / (((1.0f - iou) + v) + kIouEps);
            l = l + a * v;
            if (GRAD) {
                const float g_ap = a * (-(2.0f * kFourOverPiSq) * d);      // d v / d atan(wb / hb)
                const float den = hb * hb + wb * wb;
                g_wb = g_ap * (hb / den);
                g_hb = g_ap * (-(wb / den));
            }
        }
    }
    if (GRAD) {
        float g_y1 = 0.f, g_y2 = 0.f, g_x1 = 0.f, g_x2 = 0.f;
        if (ihr > 0.f) {
            const float gi = g_inter * iw;
            if (b.y2 <= t.y2) g_y2 += gi;
            if (b.y1 >= t.y1) g_y1 -= gi;
        }
        if (iwr > 0.f) {
            const float gi = g_inter * ih;
            if (b.x2 <= t.x2) g_x2 += gi;
            if (b.x1 >= t.x1) g_x1 -= gi;
        }
        g_hb = g_hb + g_area * wb;
        g_wb = g_wb + g_area * hb;
        g_y2 += g_hb; g_y1 -= g_hb;
        g_x2 += g_wb; g_x1 -= g_wb;
        if (b.y2 >= t.y2) g_y2 += g_ch;
        if (b.y1 <= t.y1) g_y1 -= g_ch;
        if (b.x2 >= t.x2) g_x2 += g_cw;
        if (b.x1 <= t.x1) g_x1 -= g_cw;
        g_y1 += 0.5f * g_cy; g_y2 += 0.5f * g_cy;
        g_x1 += 0.5f * g_cx; g_x2 += 0.5f * g_cx;
        // the decode: y1 = cy - 0.5 h, y2 = h + y1, cy = dy * vy * ph + pcy, h = exp(dh * vh) * ph
        grad.x = (g_y1 + g_y2) * (var.x * ph);
        grad.y = (g_x1 + g_x2) * (var.y * pw);
        grad.z = (0.5f * (g_y2 - g_y1)) * (b.h * var.z);
        grad.w = (0.5f * (g_x2 - g_x1)) * (b.w * var.w);
    }
    return l;
}

__device__ __forceinline__ bool is_positive(const float4 t) { return t.x != 0.f || t.y != 0.f || t.z != 0.f || t.w != 0.f; }

__global__ __launch_bounds__(kIouThreads) void iou_partial_kernel(const IouParams p) {
    __shared__ float shf[kIouWaves];
    __shared__ int shi[kIouWaves];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int n = tile * kIouThreads + tid;
    float l = 0.f;
    int pos = 0;
    if (n < p.N) {
        const long row = (long)b * p.N + n;
        const float4 t = p.yd[row];
        if (is_positive(t)) {
            float4 unused;
            l = iou_anchor<false>(p.priors[n], p.var, t, p.pd[row], p.mode, unused);
            pos = 1;
        }
        if (p.per_anchor) p.per_anchor[row] = l;
    }
    IouPartial out;
    out.sum = block_sum<kIouWaves>(l, shf);
    out.pos = block_sum_i<kIouWaves>(pos, shi);
    if (tid == 0) p.part[blockIdx.x] = out;
}

__global__ __launch_bounds__(kIouThreads) void iou_finish_kernel(const IouParams p) {
    __shared__ float shf[kIouWaves];
    __shared__ int shi[kIouWaves];
    const int tid = threadIdx.x;
    const bool grads = p.grad != nullptr;                     // without them the grid is one workgroup per image
    const int b = grads ? blockIdx.x / p.tiles : blockIdx.x, tile = grads ? blockIdx.x % p.tiles : 0;
    // the image's totals: thread i adds the partials i, i + 256, ... in tile order, then the fixed tree
    float sum = 0.f;
    int pos = 0;
    for (int i = tid; i < p.tiles; i += kIouThreads) {
        const IouPartial v = p.part[(long)b * p.tiles + i];
        sum += v.sum;
        pos += v.pos;
    }
    sum = block_sum<kIouWaves>(sum, shf);
    pos = block_sum_i<kIouWaves>(pos, shi);
    const float den = pos == 0 ? 1.0f : (float)pos;
    if (tile == 0 && tid == 0 && p.loc_loss) p.loc_loss[b] = sum / den * p.loc_alpha;
    if (!grads) return;

    // gradient of grad_scale * loc_loss[b]
    const int n = tile * kIouThreads + tid;
    if (n >= p.N) return;
    const long row = (long)b * p.N + n;
    const float g = p.grad_scale * p.loc_alpha / den;
    const float4 t = p.yd[row];
    float4 r = {0.f, 0.f, 0.f, 0.f};
    if (is_positive(t)) {
        float4 d;
        iou_anchor<true>(p.priors[n], p.var, t, p.pd[row], p.mode, d);
        r.x = g * d.x; r.y = g * d.y; r.z = g * d.z; r.w = g * d.w;
    }
    p.grad[row] = r;
}

static size_t iou_workspace(int B, int N) {
    return align_up((size_t)B * (size_t)cdiv(N, kIouThreads) * sizeof(IouPartial), 256);
}

}  // namespace ssd

using namespace ssd;

extern "C" {

int ssd_iou_loc_loss_tile(void) { return kIouThreads; }

size_t ssd_iou_loc_loss_workspace_bytes(int B, int N) {
    if (B < 0 || N < 0) return 0;
    return iou_workspace(B, N);
}

int ssd_iou_loc_loss(const float* priors_dev, const float* variances, const float* actual_deltas_dev,
                     const float* pred_deltas_dev, int B, int N, int mode, float loc_loss_alpha, float* loc_loss_dev,
                     float* per_anchor_out_dev, float* grad_deltas_dev, float grad_scale, void* workspace_dev,
                     size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 1, "ssd_iou_loc_loss: bad sizes B=%d N=%d", B, N);
    SSD_CHECK_ARG(mode >= SSD_LOC_IOU && mode <= SSD_LOC_CIOU, "ssd_iou_loc_loss: unknown mode %d", mode);
    SSD_CHECK_ARG(variances, "ssd_iou_loc_loss: variances is NULL");
    for (int k = 0; k < 4; ++k)
        SSD_CHECK_ARG(variances[k] > 0.f && variances[k] < INFINITY,
                      "ssd_iou_loc_loss: variances must be > 0 and finite, got variances[%d]=%g", k, (double)variances[k]);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(priors_dev, "ssd_iou_loc_loss: priors is NULL");
    SSD_CHECK_ARG(!grad_deltas_dev || actual_deltas_dev, "ssd_iou_loc_loss: grad_deltas needs the localisation target");
    SSD_CHECK_ARG(actual_deltas_dev && pred_deltas_dev, "ssd_iou_loc_loss: actual_deltas / pred_deltas is NULL");
    SSD_CHECK_ARG(workspace_dev && workspace_bytes >= iou_workspace(B, N),
                  "ssd_iou_loc_loss: workspace too small (%zu < %zu bytes)", workspace_bytes, iou_workspace(B, N));
    SSD_CHECK_ARG((((uintptr_t)priors_dev | (uintptr_t)actual_deltas_dev | (uintptr_t)pred_deltas_dev |
                    (uintptr_t)grad_deltas_dev) & 15) == 0,
                  "ssd_iou_loc_loss: priors and delta tensors must be 16-byte aligned");
    SSD_CHECK_ARG((((uintptr_t)loc_loss_dev | (uintptr_t)per_anchor_out_dev | (uintptr_t)workspace_dev) & 3) == 0,
                  "ssd_iou_loc_loss: loss outputs and the workspace must be 4-byte aligned");
    IouParams p{};
    p.priors = reinterpret_cast<const float4*>(priors_dev);
    p.var = make_float4(variances[0], variances[1], variances[2], variances[3]);
    p.yd = reinterpret_cast<const float4*>(actual_deltas_dev);
    p.pd = reinterpret_cast<const float4*>(pred_deltas_dev);
    p.B = B; p.N = N; p.mode = mode;
    p.tiles = cdiv(N, kIouThreads);
    SSD_UNSUPPORTED_IF((long)B * p.tiles > 0x7fffffffL, "ssd_iou_loc_loss: B * tiles = %ld workgroups exceed the grid limit",
                       (long)B * p.tiles);
    p.loc_alpha = loc_loss_alpha;
    p.loc_loss = loc_loss_dev; p.per_anchor = per_anchor_out_dev;
    p.grad = reinterpret_cast<float4*>(grad_deltas_dev); p.grad_scale = grad_scale;
    p.part = (IouPartial*)workspace_dev;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned all = (unsigned)((long)B * p.tiles);
    hipLaunchKernelGGL(iou_partial_kernel, dim3(all), dim3(kIouThreads), 0, st, p);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(iou_finish_kernel, dim3(grad_deltas_dev ? all : (unsigned)B), dim3(kIouThreads), 0, st, p);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

}  // extern "C"
