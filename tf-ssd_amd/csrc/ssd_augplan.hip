// The random PLAN of the training augmentation on the device (reference augmentation.py:19-25; the host form is
// tf-ssd_amd/augmentation.py draw_plan): which of patch / expand / flip / brightness / contrast / hue / saturation run, the
// expand canvas, the sampled window and the transformed ground-truth boxes -- one wavefront per image, in the layouts
// ssd_augment_geometry / ssd_augment_color / ssd_image_mean read, so a training step uploads no plan arrays.
// The generator is counter based (Philox4x32-10): every draw is a pure function of (seed, sample id, slot); the slot
// table is in include/ssd_hip.h.  The 100 attempts of sample_distorted_bounding_box are independent, so lane l evaluates
// attempts l and l + 64 and a ballot picks the lowest accepted one.  Compiled with -ffp-contract=off and correctly
// rounded division / sqrt: every fp32 operation rounds on its own, as in the NumPy restatement the tests compare with
// (tests/augment_plan_cases.py).
#include "common.h"
#include "philox.h"

namespace ssd {

static const int kPlanMaxBoxes = 512;
static const int kPlanAttempts = 100;

// np.clip(v, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clip01(const float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// bbox_utils.renormalize_bboxes_with_min_max (utils/bbox_utils.py:178-188) on one box, in LDS
__device__ __forceinline__ void renormalize(float* box, const float y_min, const float x_min, const float y_max, const float x_max) {
    const float dy = y_max - y_min, dx = x_max - x_min;
    box[0] = clip01((box[0] - y_min) / dy);
    box[1] = clip01((box[1] - x_min) / dx);
    box[2] = clip01((box[2] - y_min) / dy);
    box[3] = clip01((box[3] - x_min) / dx);
}

// blockIdx.x = the image, 64 threads = one wavefront
__global__ __launch_bounds__(64) void augment_plan_kernel(const float* gt_boxes /* may be boxes_out */, const int* __restrict__ gt_labels,
                                                         const long long* __restrict__ sample_ids, const int G, const int H,
                                                         const int W, const unsigned int key0, const unsigned int key1,
                                                         int* __restrict__ geom_out, float* __restrict__ color_out,
                                                         int* __restrict__ flags_out, float* __restrict__ add_out,
                                                         int* __restrict__ info_out, float* boxes_out) {
    __shared__ float s_box[kPlanMaxBoxes][4];       // the ground truth, transformed in place (valid rows only)
    __shared__ int s_rect[kPlanMaxBoxes][4];        // pixel rectangles on the canvas
    __shared__ unsigned char s_valid[kPlanMaxBoxes];
    const int b = blockIdx.x, lane = threadIdx.x;
    const unsigned long long id = (unsigned long long)sample_ids[b];
    const unsigned int id0 = (unsigned int)id, id1 = (unsigned int)(id >> 32);

    // the ground truth into LDS (also what makes boxes_out == gt_boxes safe: a wave reads its image before it writes it)
    const float* gb = gt_boxes + (long)b * G * 4;
    bool mine_valid = false;
    for (int g = lane; g < G; g += 64) {
        const float4 v = *reinterpret_cast<const float4*>(gb + g * 4);
        s_box[g][0] = v.x; s_box[g][1] = v.y; s_box[g][2] = v.z; s_box[g][3] = v.w;
        const bool ok = gt_labels ? gt_labels[(long)b * G + g] > 0 : (fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w)) > 0.0f;
        s_valid[g] = ok ? 1 : 0;
        mine_valid |= ok;
    }
    const bool any_valid = __ballot(mine_valid) != 0ull;

    const philox4 d0 = philox4x32_10(id0, id1, 0u, 0u, key0, key1), d1 = philox4x32_10(id0, id1, 1u, 0u, key0, key1);
    const philox4 d2 = philox4x32_10(id0, id1, 2u, 0u, key0, key1), d3 = philox4x32_10(id0, id1, 3u, 0u, key0, key1);
    const bool patch = draw_bool(d0.w[0]) && any_valid, expand = patch && draw_bool(d0.w[1]), flip = draw_bool(d0.w[2]);
    const bool brightness = draw_bool(d0.w[3]), contrast = draw_bool(d1.w[0]), hue = draw_bool(d1.w[1]), saturation = draw_bool(d1.w[2]);
    const int overlap_index = draw_below(d1.w[3], 5);

    int ch = H, cw = W, pt = 0, pl = 0;             // the canvas and the image's place on it
    int cy = 0, cx = 0, chh = H, cww = W;           // the window
    int accepted = -1;
    if (patch) {
        if (expand) {
            // expand_geometry: tf.round of the fp32 products (augmentation.py:135-140)
            const float ratio = draw_uniform(d2.w[0], 1.0f, 4.0f), fh = (float)H, fw = (float)W;
            const float final_h = rintf(fh * ratio), final_w = rintf(fw * ratio);
            const float pad_left = rintf(draw_unit(d2.w[1]) * (final_w - fw)), pad_top = rintf(draw_unit(d2.w[2]) * (final_h - fh));
            ch = (int)final_h; cw = (int)final_w; pt = (int)pad_top; pl = (int)pad_left;
            // expand_boxes: the image's corners in canvas units, then renormalize to them
            const float pad_bottom = (float)ch - (fh + (float)pt), pad_right = (float)cw - (fw + (float)pl);
            const float y_min = -(float)pt / fh, x_min = -(float)pl / fw;
            const float y_max = (pad_bottom + fh) / fh, x_max = (pad_right + fw) / fw;
            for (int g = lane; g < G; g += 64)
                if (s_valid[g]) renormalize(s_box[g], y_min, x_min, y_max, x_max);
        }
        chh = ch; cww = cw;
        const float fch = (float)ch, fcw = (float)cw;
        for (int g = lane; g < G; g += 64) {        // pixel_rectangles: truncation of the fp32 product
            s_rect[g][0] = (int)(s_box[g][0] * fch); s_rect[g][1] = (int)(s_box[g][1] * fcw);
            s_rect[g][2] = (int)(s_box[g][2] * fch); s_rect[g][3] = (int)(s_box[g][3] * fcw);
        }
        __syncthreads();
        const float overlaps[5] = {0.1f, 0.3f, 0.5f, 0.7f, 0.9f};
        const float min_overlap = overlaps[overlap_index];
        const float area = fch * fcw, min_area = 0.05f * area, max_area = 1.0f * area;
        accepted = kPlanAttempts;                   // every attempt failed: the whole canvas
        for (int round = 0; round < 2; ++round) {
            const int a = lane + 64 * round;
            bool ok = false;
            int y = 0, x = 0, h = 0, w = 0;
            if (a < kPlanAttempts) {
                const philox4 d = philox4x32_10(id0, id1, 16u + (unsigned int)a, 0u, key0, key1);
                const float aspect = draw_uniform(d.w[0], 0.5f, 2.0f);
                int min_h = (int)rintf(sqrtf(min_area / aspect)), max_h = (int)rintf(sqrtf(max_area / aspect));
                if ((int)rintf((float)max_h * aspect) > cw) {
                    max_h = (int)(((fcw + 0.5f) - 1e-7f) / aspect);
                    if ((int)rintf((float)max_h * aspect) > cw) max_h -= 1;
                }
                max_h = min(max_h, ch);
                min_h = min(min_h, max_h);
                h = min_h;
                if (min_h < max_h) h += draw_below(d.w[1], max_h - min_h + 1);
                w = (int)rintf((float)h * aspect);
                if ((float)((long long)w * h) < min_area) { h += 1; w = (int)rintf((float)h * aspect); }
                if ((float)((long long)w * h) > max_area) { h -= 1; w = (int)rintf((float)h * aspect); }
                const float wh = (float)((long long)w * h);
                if (!(wh < min_area || wh > max_area || w > cw || h > ch || w <= 0 || h <= 0)) {
                    y = h < ch ? draw_below(d.w[2], ch - h) : 0;
                    x = w < cw ? draw_below(d.w[3], cw - w) : 0;
                    // window_satisfies: some valid box of at least one pixel has >= min_overlap of its area inside
                    for (int g = 0; g < G && !ok; ++g) {
                        if (!s_valid[g]) continue;
                        const int r0 = s_rect[g][0], r1 = s_rect[g][1], r2 = s_rect[g][2], r3 = s_rect[g][3];
                        const long long box_area = (long long)(r2 - r0) * (long long)(r3 - r1);
                        if (box_area < 1) continue;
                        const long long iy = max(min(r2, y + h) - max(r0, y), 0), ix = max(min(r3, x + w) - max(r1, x), 0);
                        ok = (float)(iy * ix) / (float)box_area >= min_overlap;
                    }
                }
            }
            const unsigned long long votes = __ballot(ok);
            if (votes != 0ull) {
                const int winner = __ffsll(votes) - 1;
                accepted = winner + 64 * round;
                cy = __shfl(y, winner); cx = __shfl(x, winner); chh = __shfl(h, winner); cww = __shfl(w, winner);
                break;
            }
        }
        // the boxes in window units (augmentation.py:178-179)
        const float y_min = (float)cy / fch, x_min = (float)cx / fcw;
        const float y_max = (float)(cy + chh) / fch, x_max = (float)(cx + cww) / fcw;
        for (int g = lane; g < G; g += 64)
            if (s_valid[g]) renormalize(s_box[g], y_min, x_min, y_max, x_max);
    }
    float* ob = boxes_out + (long)b * G * 4;
    for (int g = lane; g < G; g += 64) {            // a lane reads back only the rows it wrote
        float4 v = make_float4(s_box[g][0], s_box[g][1], s_box[g][2], s_box[g][3]);
        if (flip && s_valid[g]) v = make_float4(v.x, 1.0f - v.w, v.z, 1.0f - v.y);
        *reinterpret_cast<float4*>(ob + g * 4) = v;
    }
    if (lane == 0) {
        int* q = geom_out + b * 10;
        q[0] = ch; q[1] = cw; q[2] = pt; q[3] = pl; q[4] = cy; q[5] = cx; q[6] = chh; q[7] = cww; q[8] = flip ? 1 : 0; q[9] = patch ? 1 : 0;
        const float delta = brightness ? draw_uniform(d3.w[0], -0.12f, 0.12f) : 0.0f;
        float* c = color_out + b * 4;
        c[0] = delta;
        c[1] = contrast ? draw_uniform(d3.w[1], 0.5f, 1.5f) : 1.0f;
        c[2] = hue ? draw_uniform(d3.w[2], -0.08f, 0.08f) : 0.0f;
        c[3] = saturation ? draw_uniform(d3.w[3], 0.5f, 1.5f) : 1.0f;
        flags_out[b] = (brightness ? 1 : 0) | (contrast ? 2 : 0) | (hue ? 4 : 0) | (saturation ? 8 : 0);
        add_out[b] = delta;
        int* o = info_out + b * 4;
        o[0] = accepted; o[1] = overlap_index; o[2] = expand ? 1 : 0; o[3] = 0;
    }
}

}  // namespace ssd

using namespace ssd;

extern "C" int ssd_augment_plan(const float* gt_boxes_dev, const int* gt_labels_dev, const long long* sample_ids_dev, int B,
                                int G, int H, int W, unsigned long long seed, int* geom_out_dev, float* color_out_dev,
                                int* flags_out_dev, float* add_out_dev, int* info_out_dev, float* boxes_out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && G >= 0 && H >= 1 && W >= 1, "ssd_augment_plan: bad sizes B=%d G=%d H=%d W=%d", B, G, H, W);
    SSD_UNSUPPORTED_IF(G > kPlanMaxBoxes, "ssd_augment_plan: G = %d ground-truth rows (at most %d)", G, kPlanMaxBoxes);
    SSD_UNSUPPORTED_IF(H > kMaxImageSide / 4 || W > kMaxImageSide / 4,
                       "ssd_augment_plan: %d x %d: the 4x expand canvas would exceed %d a side", H, W, kMaxImageSide);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(sample_ids_dev && geom_out_dev && color_out_dev && flags_out_dev && add_out_dev && info_out_dev,
                  "ssd_augment_plan: NULL pointer");
    SSD_CHECK_ARG(G == 0 || (gt_boxes_dev && boxes_out_dev), "ssd_augment_plan: NULL boxes");
    SSD_CHECK_ARG((((uintptr_t)gt_boxes_dev | (uintptr_t)boxes_out_dev) & 15) == 0, "ssd_augment_plan: boxes are not 16-byte aligned");
    hipLaunchKernelGGL(augment_plan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, gt_boxes_dev, gt_labels_dev, sample_ids_dev,
                       G, H, W, (unsigned int)(seed & 0xffffffffull), (unsigned int)(seed >> 32), geom_out_dev, color_out_dev,
                       flags_out_dev, add_out_dev, info_out_dev, boxes_out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
