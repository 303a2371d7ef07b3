// The detection post-processor's call record and its plan (ssd_decode.hip holds the kernels and the driver).  NmsCall is
// what an entry point asks for; nms_plan() turns it into everything that follows from it -- the sizes, which kernels run
// with how much LDS, the workspace carve, every argument check -- as one pure host function: no HIP call, no function
// pointer, no allocation, so "what would this call launch" can be asked without launching it (and by a host-only program).
#pragma once
#include <algorithm>
#include <cmath>

#include "box_math.h"
#include "common.h"

namespace ssd {

constexpr int kSortLds = 4096;   // nms_class_kernel: candidates sorted in LDS (32 KB); above: in place in HBM
constexpr int kSoftLds = 4096;   // soft_nms_kernel: the longest list whose keys and boxes are held in LDS
enum { kNmsHard = 0, kNmsGaussian = 1, kNmsLinear = 2 };     // SSD_NMS_*

struct NmsCall {
    const float *deltas, *scores, *priors_or_boxes;   // decode: deltas, probabilities, priors; raw: NULL, scores, boxes
    const float* var;       // HOST[4]; NULL: deltas taken as they are
    int B, N, L;
    bool decode;            // the SSDDecoder path (class mask, decoded boxes, clipped) / raw combined NMS
    bool logits;            // the net's own predict path: `scores` holds LOGITS, the softmax runs inside the compaction
    // the workspace's candidate counters are known to be zero (zeroed at allocation, re-zeroed by the selection kernel of
    // the previous call): no memset launch
    bool counts_clean;
    ssd_nms_config cfg;     // {SSD_NMS_HARD, per class} for the entry points without one; clip_boxes counts in raw form only
    float *boxes_out, *labels_out, *scores_out;
    int *valid_out, *kept_idx;
    void* ws;
    size_t ws_bytes;
    // the workspace is carved for ws_batch images when given (>= B): with counts_clean the counters have to sit at the same
    // place whatever batch a call runs (a layout for a smaller B would put its kept counts on a larger batch's counters)
    int ws_batch;
};

// a config into the record: SSD_E_INVALID for the arguments include/ssd_hip.h rejects
inline int nms_set_config(NmsCall* c, const ssd_nms_config* cfg) {
    SSD_CHECK_ARG(cfg != nullptr, "nms config is NULL");
    SSD_CHECK_ARG(cfg->method == SSD_NMS_HARD || cfg->method == SSD_NMS_GAUSSIAN || cfg->method == SSD_NMS_LINEAR,
                  "nms config: unknown method %d", cfg->method);
    SSD_CHECK_ARG(cfg->method != SSD_NMS_GAUSSIAN || (std::isfinite(cfg->sigma) && cfg->sigma > 0.0f),
                  "nms config: sigma=%g (SSD_NMS_GAUSSIAN needs a finite sigma > 0)", (double)cfg->sigma);
    SSD_CHECK_ARG(cfg->iou_threshold >= 0.0f && cfg->iou_threshold <= 1.0f, "nms config: iou_threshold=%g outside [0, 1]",
                  (double)cfg->iou_threshold);
    c->cfg = *cfg;
    return SSD_OK;
}

struct NmsWs {
    int *cand_count, *kept_count;
    unsigned long long *cand_keys, *kept_keys, *merge_ws;
    float4* boxes;
    size_t bytes;
};
inline NmsWs nms_carve(void* base, int B, int N, int L, int maxk) {
    NmsWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? (void*)((char*)base + off) : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    w.cand_count = (int*)take((size_t)B * L * 4);
    w.kept_count = (int*)take((size_t)B * L * 4);
    w.cand_keys = (unsigned long long*)take((size_t)B * L * N * 8);
    w.kept_keys = (unsigned long long*)take((size_t)B * L * maxk * 8);
    w.merge_ws = (unsigned long long*)take((size_t)B * L * maxk * 8);
    w.boxes = (float4*)take((size_t)B * N * 16);
    w.bytes = off;
    return w;
}

// compact_kernel<DECODE, LOGITS, AGN>: kCompactAgn + one of the first three for the class-agnostic form
enum { kCompactDecode, kCompactLogits, kCompactRaw, kCompactAgn };
// nms_class_kernel (hard, per class: the reference's post-processor), or kSelectSoft + SSD_NMS_*: soft_nms_kernel<METHOD>
enum { kSelectClass, kSelectSoft };
// one launch of 256-thread blocks; raise: `lds` is past the 64 KiB a kernel gets without its attribute raised
struct NmsLaunch { int kernel; dim3 grid; size_t lds; bool raise; };

struct NmsPlan {
    enum { kNothing, kZeroFill, kRun } what;    // B == 0: no output rows; N == 0: nothing to select, all-zero outputs
    int agn, maxk, use_lds, clip;
    // a list is an (image, class), or an image when agn: `cap` keys of the cand_keys carve and `kept_stride` of the
    // kept_keys carve each, at most `limit` selections; the merge reads merge_L lists an image
    int cap, kept_stride, limit, lds_cap, merge_L, merge_in_lds;
    float scale;                                // SSD_NMS_GAUSSIAN: -0.5f / sigma, one float division
    NmsLaunch compact, select, merge;
    NmsWs ws;
};

// the fused softmax needs the [256, L] score slab staged in LDS; above 96 KiB the compaction's lanes read their rows from HBM
inline bool decode_nms_fused_ok(int L) { return (size_t)256 * L * 4 <= 96 * 1024; }

inline int nms_plan(const NmsCall& c, NmsPlan* p) {
    const int B = c.B, N = c.N, L = c.L, max_per_class = c.cfg.max_per_class, max_total = c.cfg.max_total;
    SSD_CHECK_ARG(B >= 0 && N >= 0 && L >= 1, "decode_nms: bad sizes B=%d N=%d L=%d", B, N, L);
    SSD_CHECK_ARG(max_per_class >= 1 && max_total >= 1, "decode_nms: max_per_class=%d max_total=%d", max_per_class, max_total);
    SSD_UNSUPPORTED_IF(N >= (1 << kIdxBits), "decode_nms: N=%d exceeds %d anchors", N, 1 << kIdxBits);
    SSD_UNSUPPORTED_IF(L > (1 << kClsBits), "decode_nms: L=%d exceeds %d classes", L, 1 << kClsBits);
    *p = NmsPlan{};
    const bool agn = c.cfg.class_agnostic != 0;
    SSD_UNSUPPORTED_IF(agn && (long)N * L > 0x7fffffffL, "decode_nms: N=%d x L=%d candidates in one class-agnostic list", N, L);
    p->what = B == 0 ? NmsPlan::kNothing : N == 0 ? NmsPlan::kZeroFill : NmsPlan::kRun;
    if (p->what != NmsPlan::kRun) return SSD_OK;
    const int maxk = max_per_class < N ? max_per_class : N;
    const size_t nms_lds = (size_t)maxk * 16 + 256 * 16 + 256 * 8 + (size_t)kSortLds * 8 + 64;
    SSD_UNSUPPORTED_IF(nms_lds > 160 * 1024, "decode_nms: max_per_class=%d needs %zu B of LDS", max_per_class, nms_lds);
    SSD_CHECK_ARG(c.ws != nullptr, "decode_nms: workspace is NULL");
    SSD_CHECK_ARG(c.ws_batch == 0 || c.ws_batch >= B, "decode_nms: workspace carved for %d images, batch %d", c.ws_batch, B);
    p->ws = nms_carve(c.ws, c.ws_batch ? c.ws_batch : B, N, L, maxk);
    SSD_CHECK_ARG(c.ws_bytes >= p->ws.bytes, "decode_nms: workspace %zu < required %zu", c.ws_bytes, p->ws.bytes);
    SSD_CHECK_ARG(((uintptr_t)c.ws & 15) == 0, "decode_nms: workspace must be 16-byte aligned");
    const size_t tile_bytes = (size_t)256 * L * 4;
    p->use_lds = decode_nms_fused_ok(L);
    SSD_CHECK_ARG(!c.logits || (c.decode && p->use_lds), "decode_nms: fused softmax needs the LDS-staged decoder path");
    p->agn = agn; p->maxk = maxk;
    p->clip = c.decode ? 1 : c.cfg.clip_boxes;          // SSDDecoder always clips
    p->cap = agn ? N * L : N;
    p->kept_stride = agn ? L * maxk : maxk;
    p->limit = agn ? std::min(std::min(max_per_class, max_total), p->kept_stride) : maxk;
    p->lds_cap = std::min(p->cap, kSoftLds);
    p->scale = c.cfg.method == SSD_NMS_GAUSSIAN ? -0.5f / c.cfg.sigma : 0.0f;
    p->compact = {(agn ? kCompactAgn : 0) + (!c.decode ? kCompactRaw : c.logits ? kCompactLogits : kCompactDecode),
                  dim3(cdiv(N, 256), B), p->use_lds ? tile_bytes : 0, p->use_lds && tile_bytes > 64 * 1024};
    // everything but the reference's post-processor runs the selection kernel: 24 B of LDS a candidate it holds
    const bool soft = agn || c.cfg.method != SSD_NMS_HARD;
    const size_t select_lds = soft ? (size_t)p->lds_cap * 24 : nms_lds;
    p->select = {soft ? kSelectSoft + c.cfg.method : kSelectClass, dim3(agn ? B : B * L), select_lds, select_lds > 64 * 1024};
    // the merge of an agnostic image: ONE list of up to kept_stride rows, already in order
    p->merge_L = agn ? 1 : L;
    const size_t merge_keys = (size_t)p->merge_L * p->kept_stride * 8;
    const size_t merge_hdr = align_up((size_t)(p->merge_L + 1) * 4, 16);
    p->merge_in_lds = merge_hdr + merge_keys <= 64 * 1024;
    p->merge = {0, dim3(B), merge_hdr + (p->merge_in_lds ? merge_keys : 0), false};
    return SSD_OK;
}

}  // namespace ssd
