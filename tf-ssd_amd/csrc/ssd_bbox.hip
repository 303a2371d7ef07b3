// Box-math kernels for gfx950: prior boxes, box decode, pairwise IoU map, delta encode, max-IoU target matching
// (match_encode) and the two evaluation matchers (eval_match, eval_match_protocol).  The detection post-processor
// (compaction, NMS, top-K merge) is ssd_decode.hip; the device math both share is box_math.h.
//
// Built with -ffp-contract=off: every product and sum is rounded separately, exactly as
// the reference's chain of elementwise TF ops does (utils/bbox_utils.py), so that the
// match indices are bit-exact against the oracle.
#include "box_math.h"
#include "common.h"

#include <algorithm>
#include <cmath>

namespace ssd {

// ------------------------------------------------------------------ prior boxes (A1-A3)
constexpr int kMaxLevels = 16;
constexpr int kMaxArs = 15;
struct PriorCfg {
    int levels;
    int f[kMaxLevels];
    int a[kMaxLevels];          // anchors per cell = n_ars + 1
    int offset[kMaxLevels + 1];
    double cur[kMaxLevels];     // A1 scale s_k   (host float64, utils/bbox_utils.py:124)
    double nxt[kMaxLevels];     // A1 scale s_k+1
    float ar[kMaxLevels][kMaxArs];
};

__global__ void priors_kernel(const PriorCfg cfg, float4* __restrict__ out, int total) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    int l = 0;
    while (l + 1 < cfg.levels && gid >= cfg.offset[l + 1]) ++l;
    const int local = gid - cfg.offset[l];
    const int A = cfg.a[l], f = cfg.f[l];
    const int a = local % A;
    const int cell = local / A;
    const int y = cell / f, x = cell % f;
    // utils/bbox_utils.py:139-146
    float h, w;
    if (a < A - 1) {
        const float s = sqrtf(cfg.ar[l][a]);
        h = (((float)cfg.cur[l]) / (s));
        w = (float)cfg.cur[l] * s;
    } else {
        h = w = sqrtf((float)(cfg.cur[l] * cfg.nxt[l]));
    }
    // utils/bbox_utils.py:164-165: int32 / int -> float64, + stride/2 in float64, cast.
    const double stride = 1.0 / (double)f;
    const float gy = (float)((double)y / (double)f + stride / 2.0);
    const float gx = (float)((double)x / (double)f + stride / 2.0);
    float4 r;
    r.x = (-h / 2.0f) + gy;
    r.y = (-w / 2.0f) + gx;
    r.z = (h / 2.0f) + gy;
    r.w = (w / 2.0f) + gx;
    // :176 clip_by_value(0, 1)
    r.x = fminf(fmaxf(r.x, 0.0f), 1.0f);
    r.y = fminf(fmaxf(r.y, 0.0f), 1.0f);
    r.z = fminf(fmaxf(r.z, 0.0f), 1.0f);
    r.w = fminf(fmaxf(r.w, 0.0f), 1.0f);
    out[gid] = r;
}

// ------------------------------------------------------------------ decode (D1)
__global__ void decode_kernel(const float4* __restrict__ priors, const float4* __restrict__ deltas,
                              const float4 var, const int use_var, const int N, const long total,
                              float4* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x)
        out[i] = decode_box(priors[i % N], deltas[i], var, use_var != 0);
}

// ------------------------------------------------------------------ IoU map (M1)
__global__ void iou_map_kernel(const float4* __restrict__ boxes, const int boxes_batched,
                               const float4* __restrict__ gt, const int N, const int G,
                               const long total, float* __restrict__ out) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long)gridDim.x * blockDim.x) {
        const int g = (int)(e % G);
        const long bi = e / G;
        const int i = (int)(bi % N);
        const long b = bi / N;
        const float4 p = boxes_batched ? boxes[b * N + i] : boxes[i];
        out[e] = pair_iou(p, gt[b * G + g]);
    }
}

// ------------------------------------------------------------------ encode (M3): encode_box, box_math.h
__global__ void encode_kernel(const float4* __restrict__ bboxes, const float4* __restrict__ gt,
                              const int N, const long total, float4* __restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x)
        out[i] = encode_box(bboxes[i % N], gt[i]);
}

// ------------------------------------------------------------------ match + encode (M2)
// One thread per (image, prior): loop over the (small) padded GT list staged in LDS.
__global__ __launch_bounds__(256) void match_encode_kernel(
    const float4* __restrict__ priors, const float4* __restrict__ gt, const int* __restrict__ gt_labels,
    const float4 var, const float iou_thr, const int N, const int G, const int L,
    float4* __restrict__ deltas, int* __restrict__ label_idx, int* __restrict__ match_idx,
    float* __restrict__ onehot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* s_gt = reinterpret_cast<float4*>(smem);
    int* s_lab = reinterpret_cast<int*>(s_gt + G);
    const int b = blockIdx.y;
    for (int g = threadIdx.x; g < G; g += 256) {
        s_gt[g] = gt[(size_t)b * G + g];
        s_lab[g] = gt_labels[(size_t)b * G + g];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float4 p = priors[i];
    // [3P] tf.argmax / reduce_max (Eigen reducers: accumulator starts at lowest(), replaced only
    // by a strictly greater value): first max wins and a NaN IoU (0/0: degenerate prior against a
    // padded ground-truth box) is never selected
    int am = 0;
    float best = G > 0 ? -3.402823466e38f : 0.0f;
    for (int g = 0; g < G; ++g) {
        const float v = pair_iou(p, s_gt[g]);
        if (v > best) { best = v; am = g; }
    }
    const bool pos = best > iou_thr;              // strict (utils/train_utils.py:117)
    float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
    int lab = 0;
    if (pos) { gb = s_gt[am]; lab = s_lab[am]; }
    float4 d = encode_box(p, gb);
    d.x = ((d.x) / (var.x));
    d.y = ((d.y) / (var.y));
    d.z = ((d.z) / (var.z));
    d.w = ((d.w) / (var.w));
    const size_t o = (size_t)b * N + i;
    deltas[o] = d;
    label_idx[o] = lab;
    match_idx[o] = am;
    if (onehot) {
        float* oh = onehot + o * L;
        for (int c = 0; c < L; ++c) oh[c] = (c == lab) ? 1.0f : 0.0f;
    }
}

// ------------------------------------------------------------------ detection scoring (N2)
// utils/eval_utils.py:20-50 for one image per 256-thread block.  The reference walks the detections serially in
// descending best-IoU order and remembers the ground-truth boxes already taken; here every detection finds its own
// place in that walk by counting (its record index = the number of non-padding detections visited before it) and the
// "already taken" test becomes "am I the first ELIGIBLE record on my box" (eligible: IoU >= thr and labels agree),
// resolved by an integer atomicMin on the record index in LDS -- order-independent, so the result is deterministic.
// LDS: G * 24 B (boxes, labels, first record) + T * 16 B (key, label, arg-max, record index).
constexpr int kEvalMaxT = 1024;
constexpr int kEvalMaxG = 256;

__global__ __launch_bounds__(256) void eval_match_kernel(
    const float4* __restrict__ det, const float* __restrict__ det_labels, const float* __restrict__ det_scores,
    const float4* __restrict__ gt, const int* __restrict__ gt_labels, const int T, const int G, const float iou_thr,
    int* __restrict__ rec_class, float* __restrict__ rec_score, int* __restrict__ rec_tp, int* __restrict__ rec_det,
    int* __restrict__ rec_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* s_gt = reinterpret_cast<float4*>(smem);          // [G]
    int* s_glab = reinterpret_cast<int*>(s_gt + G);          // [G]
    int* s_first = s_glab + G;                               // [G] record index of the first eligible detection
    float* s_key = reinterpret_cast<float*>(s_first + G);    // [T] best IoU
    float* s_lab = s_key + T;                                // [T] detection label
    int* s_arg = reinterpret_cast<int*>(s_lab + T);          // [T] arg-max ground-truth box
    int* s_pos = s_arg + T;                                  // [T] record index
    __shared__ int s_count;
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int g = tid; g < G; g += 256) {
        s_gt[g] = gt[(size_t)b * G + g];
        s_glab[g] = gt_labels[(size_t)b * G + g];
        s_first[g] = T;
    }
    if (tid == 0) s_count = 0;
    __syncthreads();
    // :20-22 [3P] tf.reduce_max / tf.argmax (Eigen reducers): start at -inf, strict >: first max, NaN never selected
    for (int t = tid; t < T; t += 256) {
        const float4 p = det[(size_t)b * T + t];
        int am = 0;
        float best = -__builtin_inff();
        for (int g = 0; g < G; ++g) {
            const float v = pair_iou(p, s_gt[g]);
            if (v > best) { best = v; am = g; }
        }
        s_key[t] = best;
        s_arg[t] = am;
        s_lab[t] = det_labels[(size_t)b * T + t];
    }
    __syncthreads();
    // :23 argsort DESCENDING (equal keys by ascending index), :35-36 label 0 skipped
    for (int t = tid; t < T; t += 256) {
        const float lab = s_lab[t];
        if (lab == 0.0f) continue;
        const float kt = s_key[t];
        int pos = 0;
        for (int u = 0; u < T; ++u) {
            const float ku = s_key[u];
            const bool before = ku > kt || (ku == kt && u < t);
            pos += (before && s_lab[u] != 0.0f) ? 1 : 0;
        }
        s_pos[t] = pos;
        const int am = s_arg[t];
        if (kt >= iou_thr && (int)lab == s_glab[am]) atomicMin(&s_first[am], pos);
        atomicAdd(&s_count, 1);
    }
    __syncthreads();
    const int count = s_count;
    if (tid == 0) rec_count[b] = count;
    // :37-50
    for (int t = tid; t < T; t += 256) {
        const float lab = s_lab[t];
        if (lab == 0.0f) continue;
        const int pos = s_pos[t], am = s_arg[t];
        const bool hit = s_key[t] >= iou_thr && (int)lab == s_glab[am] && s_first[am] == pos;
        const size_t o = (size_t)b * T + pos;
        rec_class[o] = (int)lab;
        rec_score[o] = det_scores[(size_t)b * T + t];
        rec_tp[o] = hit ? 1 : 0;
        if (rec_det) rec_det[o] = t;
    }
    for (int r = count + tid; r < T; r += 256) {
        const size_t o = (size_t)b * T + r;
        rec_class[o] = 0;
        rec_score[o] = 0.0f;
        rec_tp[o] = 0;
        if (rec_det) rec_det[o] = 0;
    }
}

// ------------------------------------------------------------------ detection scoring, devkit / COCO matching rules
// One image per 256-thread block.  Records (label != 0 rows) are ranked by counting on a total-order score key (score
// descending, equal scores by ascending index; -0 == +0, NaN last), the ground truth is sorted by counting too (by class,
// under the COCO rule non-ignored boxes first, index order within) so that the boxes of one class are one contiguous
// segment.  The walk is serial only within one (class with ground truth in the image, threshold) chain: every chain gets
// a lane, chain = class segment * NT + threshold so that neighbouring lanes share their loop bounds.  The records are
// kept in LDS sorted by (class, rank) -- a second count in the ranking loop -- so that a chain walks its own contiguous
// run of records and the lanes of a wavefront stay convergent (lane k on ITS i-th record; walking all records and
// skipping the other classes' serialises the wavefront over every record: measured at B=64, T=200, G=16 that way 98 us
// (VOC, NT=1) / 121 us (COCO, NT=10), 52 / 65 us on the sorted records, 34 / 63 us with the VOC maxima found by one
// thread per record in front of the walk).  Chains of different
// classes touch disjoint boxes and disjoint records, chains of different thresholds own a row of `taken` and of the
// states each: byte stores to distinct LDS bytes, no atomics, the same bits on every run.  Records whose class has no
// box in the image keep the initial state 0 (FP).
// IoU: recomputed (pair_iou, ~20 VALU ops) instead of an LDS tile -- the tile is T * G * 4 B = 1 MiB at the limits against
// 160 KiB of LDS per CU, and a chain only ever asks for (record of class c) x (box of class c) pairs.
// LDS: T * (32 + NT) B (box, key, label, class, rank and NT states per record) + G * (33 + NT) B + NT * 4 + 4 B, see
// eval_protocol_lds_bytes: 52.8 KiB at T = 1024, G = 256, NT = 10, under the 64 KiB a workgroup gets.
constexpr int kEvalMaxNT = 10;
constexpr int kEvalRuleVoc = 0;     // SSD_EVAL_RULE_VOC
constexpr int kEvalRuleCoco = 1;    // SSD_EVAL_RULE_COCO
struct EvalThresholds { float v[kEvalMaxNT]; };

static size_t eval_protocol_lds_bytes(int T, int G, int NT) {
    // float4 s_gt[G], s_rbox[T]; 4-byte s_thr[NT], s_gkey[G], s_glab[G], s_cstart[G + 1], s_ccls[G], s_key[T], s_lab[T],
    // s_rcls[T], s_rrank[T]; bytes s_gign[G], s_taken[NT * G], s_state[NT * T]
    return (size_t)(G + T) * 16 + (size_t)(NT + 4 * G + 1 + 4 * T) * 4 + (size_t)G + (size_t)NT * G + (size_t)NT * T;
}

// ascending unsigned order == score descending; -0 counts as +0, every NaN goes last
__device__ __forceinline__ unsigned eval_score_key(float s) {
    if (s != s) return 0xffffffffu;
    return score_desc_key(s == 0.0f ? 0.0f : s);
}

__global__ __launch_bounds__(256) void eval_match_protocol_kernel(
    const float4* __restrict__ det, const float* __restrict__ det_labels, const float* __restrict__ det_scores,
    const float4* __restrict__ gt, const int* __restrict__ gt_labels, const unsigned char* __restrict__ gt_ignore,
    const int T, const int G, const int rule, const EvalThresholds thrs, const int NT, int* __restrict__ rec_class,
    float* __restrict__ rec_score, int* __restrict__ rec_det, signed char* __restrict__ rec_state,
    int* __restrict__ rec_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* s_gt = reinterpret_cast<float4*>(smem);                 // [G] boxes, sorted by (class, [ignored,] index)
    float4* s_rbox = s_gt + G;                                      // [T] boxes of the records, sorted by (class, rank)
    float* s_thr = reinterpret_cast<float*>(s_rbox + T);            // [NT]
    int* s_gkey = reinterpret_cast<int*>(s_thr + NT);               // [G] sort key of box g (input order)
    int* s_glab = s_gkey + G;                                       // [G] label, sorted
    int* s_cstart = s_glab + G;                                     // [G + 1] first sorted box of class segment k
    int* s_ccls = s_cstart + G + 1;                                 // [G] class of segment k
    unsigned* s_key = reinterpret_cast<unsigned*>(s_ccls + G);      // [T] score key (input order)
    float* s_lab = reinterpret_cast<float*>(s_key + T);             // [T] detection label (input order)
    int* s_rcls = reinterpret_cast<int*>(s_lab + T);                // [T] class, sorted like s_rbox
    int* s_rrank = s_rcls + T;                                      // [T] record index (rank by score), sorted like s_rbox
    unsigned char* s_gign = reinterpret_cast<unsigned char*>(s_rrank + T);  // [G] ignore flag, sorted
    unsigned char* s_taken = s_gign + G;                            // [NT, G]
    signed char* s_state = reinterpret_cast<signed char*>(s_taken + (size_t)NT * G);    // [NT, T]
    __shared__ int s_count, s_classes;
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool coco = rule == kEvalRuleCoco;
    constexpr int kPadKey = 0x7fffffff;
    for (int g = tid; g < G; g += 256) {
        const int lab = gt_labels[(size_t)b * G + g];
        const int ign = (gt_ignore && gt_ignore[(size_t)b * G + g]) ? 1 : 0;
        s_gkey[g] = lab <= 0 ? kPadKey : (int)(((unsigned)lab << 1) | (unsigned)(coco ? ign : 0));
    }
    for (int t = tid; t < T; t += 256) {
        s_key[t] = eval_score_key(det_scores[(size_t)b * T + t]);
        s_lab[t] = det_labels[(size_t)b * T + t];
    }
    for (int i = tid; i < NT * G; i += 256) s_taken[i] = 0;
    for (int i = tid; i < NT * T; i += 256) s_state[i] = 0;
    if (tid < NT) s_thr[tid] = thrs.v[tid];
    if (tid == 0) s_count = 0;
    __syncthreads();
    // ground truth to its sorted place (keys are unique with the index as the last digit: every place is written once)
    for (int g = tid; g < G; g += 256) {
        const int kg = s_gkey[g];
        int pos = 0;
        for (int u = 0; u < G; ++u) {
            const int ku = s_gkey[u];
            pos += (ku < kg || (ku == kg && u < g)) ? 1 : 0;
        }
        s_gt[pos] = gt[(size_t)b * G + g];
        s_glab[pos] = kg == kPadKey ? -1 : (kg >> 1);
        s_gign[pos] = (gt_ignore && gt_ignore[(size_t)b * G + g]) ? 1 : 0;
    }
    // records to their place: descending score, equal scores by ascending index, label-0 rows skipped (pos); and to
    // their place in the walk: by class, within a class in that order (cpos)
    for (int t = tid; t < T; t += 256) {
        const float lab = s_lab[t];
        if (lab == 0.0f) continue;
        const unsigned kt = s_key[t];
        const int c = (int)lab;
        int pos = 0, cpos = 0;
        for (int u = 0; u < T; ++u) {
            const float lu = s_lab[u];
            const unsigned ku = s_key[u];
            const bool before = (ku < kt || (ku == kt && u < t)) && lu != 0.0f;
            const int cu = (int)lu;
            pos += before ? 1 : 0;
            cpos += (lu != 0.0f && (cu < c || (cu == c && before))) ? 1 : 0;
        }
        s_rbox[cpos] = det[(size_t)b * T + t];
        s_rcls[cpos] = c;
        s_rrank[cpos] = pos;
        const size_t o = (size_t)b * T + pos;
        rec_class[o] = (int)lab;
        rec_score[o] = det_scores[(size_t)b * T + t];
        if (rec_det) rec_det[o] = t;
        atomicAdd(&s_count, 1);
    }
    __syncthreads();
    const int count = s_count;
    if (tid == 0) {
        rec_count[b] = count;
        int k = 0, g = 0;
        for (; g < G && s_glab[g] > 0; ++g)
            if (g == 0 || s_glab[g] != s_glab[g - 1]) { s_cstart[k] = g; s_ccls[k] = s_glab[g]; ++k; }
        s_cstart[k] = g;
        s_classes = k;
    }
    for (int r = count + tid; r < T; r += 256) {
        const size_t o = (size_t)b * T + r;
        rec_class[o] = 0;
        rec_score[o] = 0.0f;
        if (rec_det) rec_det[o] = 0;
    }
    __syncthreads();
    if (!coco) {
        // VOCevaldet.m looks at ALL class-c boxes, ignored and taken ones included, so ovmax / jmax depend on neither the
        // threshold nor the walk: one thread per record finds them (first maximum; a NaN never wins) and leaves them in
        // the record's box slot (.x = ovmax, .y = jmax, -1: no class-c box or every IoU NaN); the chains only decide
        for (int i = tid; i < count; i += 256) {
            const int c = s_rcls[i];
            int k = 0;
            for (int hi = s_classes; k < hi;) { const int mid = (k + hi) >> 1; if (s_ccls[mid] < c) k = mid + 1; else hi = mid; }
            float ovmax = -__builtin_inff();
            int jmax = -1;
            if (k < s_classes && s_ccls[k] == c) {
                const float4 p = s_rbox[i];
                for (int g = s_cstart[k]; g < s_cstart[k + 1]; ++g) {
                    const float v = pair_iou(p, s_gt[g]);
                    if (v > ovmax) { ovmax = v; jmax = g; }
                }
            }
            s_rbox[i].x = ovmax;
            s_rbox[i].y = __int_as_float(jmax);
        }
        __syncthreads();
    }
    const int chains = s_classes * NT;
    for (int chain = tid; chain < chains; chain += 256) {
        const int k = chain / NT, ti = chain - k * NT;
        const int c = s_ccls[k], g0 = s_cstart[k], g1 = s_cstart[k + 1];
        const float thr = s_thr[ti];
        unsigned char* taken = s_taken + (size_t)ti * G;
        signed char* state = s_state + (size_t)ti * T;
        // the chain's records: the run of class c in s_rcls[0, count)
        int d0 = 0, d1 = count;
        for (int hi = count; d0 < hi;) { const int mid = (d0 + hi) >> 1; if (s_rcls[mid] < c) d0 = mid + 1; else hi = mid; }
        for (int lo = d0; lo < d1;) { const int mid = (lo + d1) >> 1; if (s_rcls[mid] <= c) lo = mid + 1; else d1 = mid; }
        for (int i = d0; i < d1; ++i) {
            const int r = s_rrank[i];
            const float4 p = s_rbox[i];
            if (!coco) {
                const float ovmax = p.x;
                const int jmax = __float_as_int(p.y);
                if (jmax < 0 || ovmax < thr) continue;              // FP
                if (s_gign[jmax]) state[r] = -1;
                else if (!taken[jmax]) { taken[jmax] = 1; state[r] = 1; }
            } else {
                // cocoeval.evaluateImg: free boxes only, non-ignored ones first, a later tie wins
                float best = thr;
                int m = -1;
                for (int g = g0; g < g1; ++g) {
                    if (taken[g]) continue;
                    if (m >= 0 && !s_gign[m] && s_gign[g]) break;
                    const float v = pair_iou(p, s_gt[g]);
                    if (!(v >= best)) continue;
                    best = v;
                    m = g;
                }
                if (m < 0) continue;                                // FP
                taken[m] = 1;
                state[r] = s_gign[m] ? -1 : 1;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < NT * T; i += 256) rec_state[(size_t)b * NT * T + i] = s_state[i];
}

}  // namespace ssd

using namespace ssd;

extern "C" {

int ssd_priors_count(const int* fmaps, const int* n_ars, int levels) {
    if (!fmaps || !n_ars || levels < 0) return SSD_E_INVALID;
    long n = 0;
    for (int l = 0; l < levels; ++l) n += (long)fmaps[l] * fmaps[l] * (n_ars[l] + 1);
    return (int)n;
}

int ssd_priors(const int* fmaps, const float* const* ars, const int* n_ars, int levels,
               float* out_dev, void* stream) {
    SSD_CHECK_ARG(fmaps && ars && n_ars && out_dev, "ssd_priors: NULL argument");
    SSD_CHECK_ARG(levels >= 1 && levels <= kMaxLevels, "ssd_priors: levels=%d (1..%d)", levels, kMaxLevels);
    PriorCfg cfg;
    cfg.levels = levels;
    int off = 0;
    for (int l = 0; l < levels; ++l) {
        SSD_CHECK_ARG(fmaps[l] >= 1, "ssd_priors: feature map %d has size %d", l, fmaps[l]);
        SSD_CHECK_ARG(n_ars[l] >= 0 && n_ars[l] <= kMaxArs, "ssd_priors: level %d has %d ratios", l, n_ars[l]);
        cfg.f[l] = fmaps[l];
        cfg.a[l] = n_ars[l] + 1;
        cfg.offset[l] = off;
        off += fmaps[l] * fmaps[l] * cfg.a[l];
        // A1 (utils/bbox_utils.py:124), Python float64: 0.2 + (0.7/(m-1))*(k-1), k = l+1
        const double step = (0.9 - 0.2) / (double)(levels - 1);
        cfg.cur[l] = 0.2 + step * (double)((l + 1) - 1);
        cfg.nxt[l] = 0.2 + step * (double)((l + 2) - 1);
        for (int a = 0; a < n_ars[l]; ++a) cfg.ar[l][a] = ars[l][a];
    }
    cfg.offset[levels] = off;
    if (off == 0) return SSD_OK;
    hipLaunchKernelGGL(priors_kernel, dim3(cdiv(off, 256)), dim3(256), 0, (hipStream_t)stream, cfg,
                       (float4*)out_dev, off);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int ssd_decode_boxes(const float* priors_dev, const float* deltas_dev, const float* var, int B, int N,
                     float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 0, "ssd_decode_boxes: B=%d N=%d", B, N);
    const long total = (long)B * N;
    if (total == 0) return SSD_OK;
    SSD_CHECK_ARG(priors_dev && deltas_dev && out_dev, "ssd_decode_boxes: NULL pointer");
    const float4 v4 = var ? make_float4(var[0], var[1], var[2], var[3]) : make_float4(1, 1, 1, 1);
    const int blocks = (int)(cdiv(total, 256) < 2048 ? cdiv(total, 256) : 2048);
    hipLaunchKernelGGL(decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)priors_dev, (const float4*)deltas_dev, v4, var ? 1 : 0, N, total,
                       (float4*)out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int ssd_iou_map(const float* boxes_dev, int boxes_batched, const float* gt_dev, int B, int N, int G,
                float* out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 0 && G >= 0, "ssd_iou_map: B=%d N=%d G=%d", B, N, G);
    const long total = (long)B * N * G;
    if (total == 0) return SSD_OK;
    SSD_CHECK_ARG(boxes_dev && gt_dev && out_dev, "ssd_iou_map: NULL pointer");
    const int blocks = (int)(cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096);
    hipLaunchKernelGGL(iou_map_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)boxes_dev, boxes_batched, (const float4*)gt_dev, N, G, total, out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int ssd_encode_deltas(const float* bboxes_dev, const float* gt_dev, int B, int N, float* out_dev,
                      void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 0, "ssd_encode_deltas: B=%d N=%d", B, N);
    const long total = (long)B * N;
    if (total == 0) return SSD_OK;
    SSD_CHECK_ARG(bboxes_dev && gt_dev && out_dev, "ssd_encode_deltas: NULL pointer");
    const int blocks = (int)(cdiv(total, 256) < 2048 ? cdiv(total, 256) : 2048);
    hipLaunchKernelGGL(encode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const float4*)bboxes_dev, (const float4*)gt_dev, N, total, (float4*)out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int ssd_match_encode(const float* priors_dev, const float* gt_boxes_dev, const int* gt_labels_dev,
                     const float* var, float iou_thr, int B, int N, int G, int L,
                     float* deltas_out_dev, int* label_idx_out_dev, int* match_idx_out_dev,
                     float* onehot_out_dev, void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 0 && G >= 0 && L >= 1, "ssd_match_encode: B=%d N=%d G=%d L=%d", B, N, G, L);
    SSD_CHECK_ARG(var != nullptr, "ssd_match_encode: variances pointer is NULL");
    if ((long)B * N == 0) return SSD_OK;
    SSD_CHECK_ARG(priors_dev && deltas_out_dev && label_idx_out_dev && match_idx_out_dev,
                  "ssd_match_encode: NULL pointer");
    SSD_CHECK_ARG(G == 0 || (gt_boxes_dev && gt_labels_dev), "ssd_match_encode: NULL gt pointer");
    SSD_UNSUPPORTED_IF((size_t)G * 20 > 60 * 1024, "ssd_match_encode: G=%d exceeds the LDS-staged limit", G);
    const float4 v4 = make_float4(var[0], var[1], var[2], var[3]);
    hipLaunchKernelGGL(match_encode_kernel, dim3(cdiv(N, 256), B), dim3(256), (size_t)G * 20 + 16,
                       (hipStream_t)stream, (const float4*)priors_dev, (const float4*)gt_boxes_dev,
                       gt_labels_dev, v4, iou_thr, N, G, L, (float4*)deltas_out_dev, label_idx_out_dev,
                       match_idx_out_dev, onehot_out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int ssd_eval_match(const float* det_boxes_dev, const float* det_labels_dev, const float* det_scores_dev,
                   const float* gt_boxes_dev, const int* gt_labels_dev, int B, int T, int G, float iou_thr,
                   int* rec_class_out, float* rec_score_out, int* rec_tp_out, int* rec_det_out, int* rec_count_out,
                   void* stream) {
    SSD_CHECK_ARG(B >= 0 && T >= 0 && G >= 0, "ssd_eval_match: B=%d T=%d G=%d", B, T, G);
    SSD_UNSUPPORTED_IF(T > kEvalMaxT, "ssd_eval_match: T=%d exceeds %d detections per image", T, kEvalMaxT);
    SSD_UNSUPPORTED_IF(G < 1 || G > kEvalMaxG, "ssd_eval_match: G=%d outside 1..%d ground-truth boxes per image", G,
                       kEvalMaxG);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(gt_boxes_dev && gt_labels_dev && rec_count_out, "ssd_eval_match: NULL pointer");
    SSD_CHECK_ARG(T == 0 || (det_boxes_dev && det_labels_dev && det_scores_dev && rec_class_out && rec_score_out &&
                             rec_tp_out), "ssd_eval_match: NULL pointer");
    hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(256), (size_t)G * 24 + (size_t)T * 16, (hipStream_t)stream,
                       (const float4*)det_boxes_dev, det_labels_dev, det_scores_dev, (const float4*)gt_boxes_dev,
                       gt_labels_dev, T, G, iou_thr, rec_class_out, rec_score_out, rec_tp_out, rec_det_out,
                       rec_count_out);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int ssd_eval_match_protocol(const float* det_boxes_dev, const float* det_labels_dev, const float* det_scores_dev,
                            const float* gt_boxes_dev, const int* gt_labels_dev, const unsigned char* gt_ignore_dev,
                            int B, int T, int G, int rule, const float* iou_thrs_host, int NT, int* rec_class_out,
                            float* rec_score_out, int* rec_det_out, signed char* rec_state_out, int* rec_count_out,
                            void* stream) {
    SSD_CHECK_ARG(B >= 0 && T >= 0 && G >= 0 && NT >= 0, "ssd_eval_match_protocol: B=%d T=%d G=%d NT=%d", B, T, G, NT);
    SSD_CHECK_ARG(rule == kEvalRuleVoc || rule == kEvalRuleCoco, "ssd_eval_match_protocol: rule=%d", rule);
    SSD_UNSUPPORTED_IF(T > kEvalMaxT, "ssd_eval_match_protocol: T=%d exceeds %d detections per image", T, kEvalMaxT);
    SSD_UNSUPPORTED_IF(G < 1 || G > kEvalMaxG, "ssd_eval_match_protocol: G=%d outside 1..%d ground-truth boxes per image",
                       G, kEvalMaxG);
    SSD_UNSUPPORTED_IF(NT < 1 || NT > kEvalMaxNT, "ssd_eval_match_protocol: NT=%d outside 1..%d IoU thresholds", NT,
                       kEvalMaxNT);
    const size_t lds = eval_protocol_lds_bytes(T, G, NT);
    SSD_UNSUPPORTED_IF(lds > 64 * 1024, "ssd_eval_match_protocol: T=%d G=%d NT=%d need %zu bytes of LDS", T, G, NT, lds);
    if (B == 0) return SSD_OK;
    SSD_CHECK_ARG(iou_thrs_host && gt_boxes_dev && gt_labels_dev && rec_count_out, "ssd_eval_match_protocol: NULL pointer");
    SSD_CHECK_ARG(T == 0 || (det_boxes_dev && det_labels_dev && det_scores_dev && rec_class_out && rec_score_out &&
                             rec_state_out), "ssd_eval_match_protocol: NULL pointer");
    EvalThresholds thrs = {};
    for (int i = 0; i < NT; ++i) thrs.v[i] = iou_thrs_host[i];
    hipLaunchKernelGGL(eval_match_protocol_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream,
                       (const float4*)det_boxes_dev, det_labels_dev, det_scores_dev, (const float4*)gt_boxes_dev,
                       gt_labels_dev, gt_ignore_dev, T, G, rule, thrs, NT, rec_class_out, rec_score_out, rec_det_out,
                       rec_state_out, rec_count_out);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

}  // extern "C"
