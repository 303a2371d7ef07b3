// Target assignment behind a strategy (include/ssd_hip.h, ssd_match_encode_cfg): the SSD paper's bipartite stage in
// front of the reference's threshold rule, and ATSS.  Integer + fp32 work, wave64 shuffles and 64-bit integer maxima in LDS
// and global memory; no float atomics, so the results do not depend on the order in which waves arrive.
//
// Built with -ffp-contract=off and correctly rounded fp32 division like ssd_bbox.hip: the IoU (box_math.h) has
// ssd_iou_map's bits, and ATSS's distances and statistics are rounded once per operation as the header states.
#include "box_math.h"
#include "common.h"

#pragma clang fp contract(off)

namespace ssd {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;

__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_min(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

// ------------------------------------------------------------------ bipartite stage
// One workgroup per image.  s_best[g]: box g's best still-free prior as (IoU bits << 32 | ~i) -- IoU > 0, so the bits order
// as the floats do, and the larger key is the larger IoU, then the smaller prior; 0: no free prior overlaps the box.
// Every cached value is a maximum over the FREE priors, so picking the box with the largest cached value (ties: smaller g)
// is the global greedy step; only the boxes whose cached prior was just taken are rescanned.
// owner[i] (workspace, int32 per prior): the box prior i is forced to, -1 otherwise.  Inside bipartite_kernel prior i is
// read and written by thread i % kBipThreads alone, so no ordering between threads is needed on it.
constexpr int kBipThreads = 1024;

__device__ __forceinline__ u64 pair_key(const float v, const int i) {
    return ((u64)__float_as_uint(v) << 32) | (u64)(0xffffffffu - (unsigned)i);
}

// Box `box`'s best free prior over all N, into *slot (LDS, 0 before the call).  Both loads are unconditional so that the
// unrolled loop keeps several of them in flight: the scan is bound by their latency, not by the IoU.
__device__ __forceinline__ void column_best(const float4* __restrict__ priors, const float4 box, const int* owner,
                                            const int N, u64* slot) {
    u64 loc = 0;
#pragma unroll 4
    for (int i = threadIdx.x; i < N; i += kBipThreads) {
        const int ow = owner[i];
        const float v = pair_iou(priors[i], box);
        if (ow < 0 && v > 0.0f) {                         // a NaN IoU is no pair
            const u64 key = pair_key(v, i);
            loc = key > loc ? key : loc;
        }
    }
    loc = wave_max(loc);
    if ((threadIdx.x & 63) == 0 && loc) atomicMax(slot, loc);
}

// The first column maxima, while every prior is free: a thread per (image, prior) over the whole device, the boxes in LDS as
// in match_encode_kernel; one wave reduction and one 64-bit integer atomicMax per (wave, box) the wave overlaps.
// best_all [B][G] is zero before the launch; owner_all [B][N] is set to -1 here.
__global__ __launch_bounds__(256) void bipartite_best_kernel(
    const float4* __restrict__ priors, const float4* __restrict__ gt, const int* __restrict__ gt_labels, const int N,
    const int G, u64* __restrict__ best_all, int* __restrict__ owner_all) {
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
    const bool in = i < N;                                   // threads past N stay: the shuffles below need whole waves
    const float4 p = in ? priors[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) owner_all[(size_t)b * N + i] = -1;
    for (int g = 0; g < G; ++g) {
        if (s_lab[g] <= 0) continue;                         // uniform
        const float v = in ? pair_iou(p, s_gt[g]) : 0.0f;
        u64 key = v > 0.0f ? pair_key(v, i) : 0;
        if (__ballot(key != 0) == 0) continue;               // uniform over the wave
        key = wave_max(key);
        if ((threadIdx.x & 63) == 0) atomicMax(&best_all[(size_t)b * G + g], key);
    }
}

__global__ __launch_bounds__(kBipThreads) void bipartite_kernel(
    const float4* __restrict__ priors, const float4* __restrict__ gt, const int* __restrict__ gt_labels, const int N,
    const int G, const u64* __restrict__ best_all, int* owner_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* s_best = reinterpret_cast<u64*>(smem);              // [G]
    int* s_open = reinterpret_cast<int*>(s_best + G);        // [G] 1: valid and not yet forced
    int* s_conf = s_open + G;                                // [G] boxes to rescan this round
    __shared__ int s_nconf;
    const int b = blockIdx.x, tid = threadIdx.x;
    int* owner = owner_all + (size_t)b * N;
    const float4* bgt = gt + (size_t)b * G;
    for (int g = tid; g < G; g += kBipThreads) {
        s_best[g] = best_all[(size_t)b * G + g];            // bipartite_best_kernel's: every prior was free
        s_open[g] = gt_labels[(size_t)b * G + g] > 0 ? 1 : 0;
    }
    __syncthreads();
    for (int round = 0; round < G; ++round) {
        // every wave picks for itself (the same data, the same answer): no barrier between the reads
        u64 pick = 0;
        for (int g = tid & 63; g < G; g += 64) {
            const u64 k = s_best[g];
            if (s_open[g] && k) {
                const u64 key = (k & 0xffffffff00000000ull) | (u64)(0xffffffffu - (unsigned)g);
                pick = key > pick ? key : pick;
            }
        }
        pick = wave_max(pick);
        if (!pick) break;                                    // uniform over the workgroup
        const int gs = (int)(0xffffffffu - (unsigned)(pick & 0xffffffffull));
        const unsigned enc = (unsigned)(s_best[gs] & 0xffffffffull);
        const int is = (int)(0xffffffffu - enc);
        if (tid == 0) s_nconf = 0;
        __syncthreads();                                     // all picks are made: s_best / s_open may change
        if (tid == 0) s_open[gs] = 0;
        if (tid == (is % kBipThreads)) owner[is] = gs;
        for (int g = tid; g < G; g += kBipThreads) {
            if (g == gs || !s_open[g]) continue;
            const u64 k = s_best[g];
            if (k && (unsigned)(k & 0xffffffffull) == enc) {
                s_best[g] = 0;
                s_conf[atomicAdd(&s_nconf, 1)] = g;         // the order of the list does not matter
            }
        }
        __syncthreads();
        const int nconf = s_nconf;
        for (int c = 0; c < nconf; ++c) {
            const int g = s_conf[c];
            column_best(priors, bgt[g], owner, N, &s_best[g]);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ ATSS candidates
// One workgroup per (image, box).  Per level, min(topk, level size) rounds of a block arg-min on the key
// (d2 bits << 32 | i): d2 >= +0, so its bits order as the floats do; a NaN d2 becomes 0xffffffff and orders last.  A round
// takes the smallest key above the previous round's, so nothing is marked and the keys are recomputed (five fp32 ops).
// keys[b * N + i] (workspace, zeroed before the launch) takes, by a 64-bit integer maximum, the largest
// (ordered IoU bits << 32 | ~g) over the boxes prior i is positive for: the largest IoU, then the smaller g.
constexpr int kAtssThreads = 256;
constexpr int kAtssMaxCand = SSD_MATCH_MAX_LEVELS * SSD_MATCH_MAX_TOPK;

struct AtssLevels {
    int n;
    int topk;
    int start[SSD_MATCH_MAX_LEVELS + 1];
};

__device__ __forceinline__ float centre(const float a, const float b) { return (a + b) * 0.5f; }

__device__ __forceinline__ u64 dist_key(const float4 p, const float gcy, const float gcx, const int i) {
    const float dy = centre(p.x, p.z) - gcy;
    const float dx = centre(p.y, p.w) - gcx;
    const float dy2 = dy * dy;
    const float dx2 = dx * dx;
    const float d2 = dy2 + dx2;
    const unsigned hi = d2 != d2 ? 0xffffffffu : __float_as_uint(d2);
    return ((u64)hi << 32) | (u64)(unsigned)i;
}

// ascending unsigned order == ascending float order (-0 folded into +0 first: equal IoUs must tie)
__device__ __forceinline__ unsigned ordered_bits(const float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ __launch_bounds__(kAtssThreads) void atss_candidates_kernel(
    const float4* __restrict__ priors, const float4* __restrict__ gt, const int* __restrict__ gt_labels, const int N,
    const int G, const AtssLevels lv, u64* __restrict__ keys) {
    __shared__ u64 s_cand[kAtssMaxCand];
    __shared__ float s_iou[kAtssMaxCand];
    __shared__ double s_thr;
    const int b = blockIdx.x / G, g = blockIdx.x % G, tid = threadIdx.x;
    if (gt_labels[(size_t)b * G + g] <= 0) return;           // uniform: padding rows select nothing
    const float4 box = gt[(size_t)b * G + g];
    const float gcy = centre(box.x, box.z), gcx = centre(box.y, box.w);
    for (int k = tid; k < kAtssMaxCand; k += kAtssThreads) s_cand[k] = kNone;
    __syncthreads();
    int n = 0;
    for (int l = 0; l < lv.n; ++l) {
        const int s = lv.start[l], e = lv.start[l + 1];
        const int cnt = min(lv.topk, e - s);
        u64 last = 0;
        for (int r = 0; r < cnt; ++r) {
            u64 loc = kNone;
            for (int i = s + tid; i < e; i += kAtssThreads) {
                const u64 key = dist_key(priors[i], gcy, gcx, i);
                if ((r == 0 || key > last) && key < loc) loc = key;
            }
            loc = wave_min(loc);
            if ((tid & 63) == 0 && loc != kNone) atomicMin(&s_cand[n + r], loc);
            __syncthreads();
            last = s_cand[n + r];                            // cnt <= level size and the keys are distinct: a real key
        }
        n += cnt;
    }
    for (int k = tid; k < n; k += kAtssThreads)
        s_iou[k] = pair_iou(priors[(int)(s_cand[k] & 0xffffffffull)], box);
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int k = 0; k < n; ++k) sum = sum + (double)s_iou[k];
        const double mean = sum / (double)n;
        double sq = 0.0;
        for (int k = 0; k < n; ++k) {
            const double d = (double)s_iou[k] - mean;
            const double dd = d * d;
            sq = sq + dd;
        }
        const double var = n > 1 ? sq / (double)(n - 1) : 0.0;
        s_thr = mean + sqrt(var);
    }
    __syncthreads();
    const double thr = s_thr;
    for (int k = tid; k < n; k += kAtssThreads) {
        const float v = s_iou[k];
        if (!((double)v >= thr)) continue;
        const int i = (int)(s_cand[k] & 0xffffffffull);
        const float4 p = priors[i];
        const float cy = centre(p.x, p.z), cx = centre(p.y, p.w);
        if (box.x < cy && cy < box.z && box.y < cx && cx < box.w)
            atomicMax(&keys[(size_t)b * N + i], ((u64)ordered_bits(v) << 32) | (u64)(0xffffffffu - (unsigned)g));
    }
}

// ------------------------------------------------------------------ per-prior targets
// match_encode_kernel's thread per (image, prior) behind the two strategies' ownership tables.
// BIPARTITE: the reference rule over the G columns (boxes in LDS), overridden where owner[i] >= 0.
// ATSS: the box out of keys[i], background (match_idx -1) where the key is 0.
template <int STRATEGY>
__global__ __launch_bounds__(256) void assign_kernel(
    const float4* __restrict__ priors, const float4* __restrict__ gt, const int* __restrict__ gt_labels, const float4 var,
    const float iou_thr, const int N, const int G, const int L, const void* __restrict__ table,
    float4* __restrict__ deltas, int* __restrict__ label_idx, int* __restrict__ match_idx, float* __restrict__ onehot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* s_gt = reinterpret_cast<float4*>(smem);
    int* s_lab = reinterpret_cast<int*>(s_gt + G);
    const int b = blockIdx.y;
    if (STRATEGY == SSD_MATCH_BIPARTITE) {
        for (int g = threadIdx.x; g < G; g += 256) {
            s_gt[g] = gt[(size_t)b * G + g];
            s_lab[g] = gt_labels[(size_t)b * G + g];
        }
        __syncthreads();
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float4 p = priors[i];
    const size_t o = (size_t)b * N + i;
    int am;
    bool pos;
    float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
    int lab = 0;
    if (STRATEGY == SSD_MATCH_BIPARTITE) {
        am = 0;
        float best = -3.402823466e38f;                       // G > 0 here
        for (int g = 0; g < G; ++g) {
            const float v = pair_iou(p, s_gt[g]);
            if (v > best) { best = v; am = g; }
        }
        pos = best > iou_thr;
        const int forced = static_cast<const int*>(table)[o];
        if (forced >= 0) { am = forced; pos = true; }
        if (pos) { gb = s_gt[am]; lab = s_lab[am]; }
    } else {
        const u64 key = static_cast<const u64*>(table)[o];
        pos = key != 0;
        am = pos ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) : -1;
        if (pos) { gb = gt[(size_t)b * G + am]; lab = gt_labels[(size_t)b * G + am]; }
    }
    float4 d = encode_box(p, gb);
    d.x = ((d.x) / (var.x));
    d.y = ((d.y) / (var.y));
    d.z = ((d.z) / (var.z));
    d.w = ((d.w) / (var.w));
    deltas[o] = d;
    label_idx[o] = lab;
    match_idx[o] = am;
    if (onehot) {
        float* oh = onehot + o * L;
        for (int c = 0; c < L; ++c) oh[c] = (c == lab) ? 1.0f : 0.0f;
    }
}

static int match_config_check(const ssd_match_config* cfg, const int N) {
    SSD_CHECK_ARG(cfg != nullptr, "match config is NULL");
    SSD_CHECK_ARG(cfg->strategy == SSD_MATCH_MAX_IOU || cfg->strategy == SSD_MATCH_BIPARTITE || cfg->strategy == SSD_MATCH_ATSS,
                  "match config: unknown strategy %d", cfg->strategy);
    if (cfg->strategy != SSD_MATCH_ATSS) return SSD_OK;
    SSD_CHECK_ARG(cfg->topk >= 1 && cfg->topk <= SSD_MATCH_MAX_TOPK, "match config: topk=%d outside 1..%d", cfg->topk,
                  SSD_MATCH_MAX_TOPK);
    SSD_CHECK_ARG(cfg->n_levels >= 1 && cfg->n_levels <= SSD_MATCH_MAX_LEVELS, "match config: n_levels=%d outside 1..%d",
                  cfg->n_levels, SSD_MATCH_MAX_LEVELS);
    SSD_CHECK_ARG(cfg->level_start[0] == 0, "match config: level_start[0]=%d, not 0", cfg->level_start[0]);
    for (int l = 0; l < cfg->n_levels; ++l)
        SSD_CHECK_ARG(cfg->level_start[l + 1] >= cfg->level_start[l], "match config: level_start decreases at level %d", l);
    SSD_CHECK_ARG(cfg->level_start[cfg->n_levels] == N, "match config: level_start ends at %d, N=%d",
                  cfg->level_start[cfg->n_levels], N);
    return SSD_OK;
}

}  // namespace ssd

using namespace ssd;

extern "C" {

size_t ssd_match_encode_cfg_workspace_bytes(int B, int N, int G, const ssd_match_config* cfg) {
    if (!cfg || B <= 0 || N <= 0 || G < 0) return 0;
    if (cfg->strategy == SSD_MATCH_BIPARTITE) return G > 0 ? align_up((size_t)B * N * sizeof(int), 16) + (size_t)B * G * sizeof(u64) : 0;
    if (cfg->strategy == SSD_MATCH_ATSS) return (size_t)B * N * sizeof(u64);
    return 0;
}

int ssd_match_encode_cfg(const float* priors_dev, const float* gt_boxes_dev, const int* gt_labels_dev, const float* var,
                         const ssd_match_config* cfg, int B, int N, int G, int L, float* deltas_out_dev,
                         int* label_idx_out_dev, int* match_idx_out_dev, float* onehot_out_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 0 && G >= 0 && L >= 1, "ssd_match_encode_cfg: B=%d N=%d G=%d L=%d", B, N, G, L);
    if (const int rc = match_config_check(cfg, N)) return rc;
    // MAX_IOU, and BIPARTITE without a box to force: the reference rule, ssd_match_encode's own launch
    if (cfg->strategy == SSD_MATCH_MAX_IOU || (cfg->strategy == SSD_MATCH_BIPARTITE && G == 0))
        return ssd_match_encode(priors_dev, gt_boxes_dev, gt_labels_dev, var, cfg->iou_threshold, B, N, G, L, deltas_out_dev,
                                label_idx_out_dev, match_idx_out_dev, onehot_out_dev, stream);
    SSD_CHECK_ARG(var != nullptr, "ssd_match_encode_cfg: variances pointer is NULL");
    if ((long)B * N == 0) return SSD_OK;
    SSD_CHECK_ARG(priors_dev && deltas_out_dev && label_idx_out_dev && match_idx_out_dev, "ssd_match_encode_cfg: NULL pointer");
    SSD_CHECK_ARG(G == 0 || (gt_boxes_dev && gt_labels_dev), "ssd_match_encode_cfg: NULL gt pointer");
    SSD_UNSUPPORTED_IF((size_t)G * 20 > 60 * 1024, "ssd_match_encode_cfg: G=%d exceeds the LDS-staged limit", G);
    SSD_UNSUPPORTED_IF(B > 65535, "ssd_match_encode_cfg: B=%d exceeds 65535 images", B);
    const size_t need = ssd_match_encode_cfg_workspace_bytes(B, N, G, cfg);
    SSD_CHECK_ARG(workspace_dev != nullptr, "ssd_match_encode_cfg: workspace is NULL");
    SSD_CHECK_ARG(workspace_bytes >= need, "ssd_match_encode_cfg: workspace %zu < required %zu", workspace_bytes, need);
    SSD_CHECK_ARG(((uintptr_t)workspace_dev & 15) == 0, "ssd_match_encode_cfg: workspace must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const float4 v4 = make_float4(var[0], var[1], var[2], var[3]);
    const float4* pri = (const float4*)priors_dev;
    const float4* gt = (const float4*)gt_boxes_dev;
    const dim3 grid(cdiv(N, 256), B);
    if (cfg->strategy == SSD_MATCH_BIPARTITE) {
        int* owner = (int*)workspace_dev;
        u64* best = (u64*)((char*)workspace_dev + align_up((size_t)B * N * sizeof(int), 16));
        SSD_HIP(hipMemsetAsync(best, 0, (size_t)B * G * sizeof(u64), st));
        hipLaunchKernelGGL(bipartite_best_kernel, grid, dim3(256), (size_t)G * 20 + 16, st, pri, gt, gt_labels_dev, N, G, best,
                           owner);
        SSD_LAUNCH_CHECK();
        hipLaunchKernelGGL(bipartite_kernel, dim3(B), dim3(kBipThreads), (size_t)G * 16, st, pri, gt, gt_labels_dev, N, G,
                           (const u64*)best, owner);
        SSD_LAUNCH_CHECK();
        hipLaunchKernelGGL(assign_kernel<SSD_MATCH_BIPARTITE>, grid, dim3(256), (size_t)G * 20 + 16, st, pri, gt, gt_labels_dev,
                           v4, cfg->iou_threshold, N, G, L, (const void*)workspace_dev, (float4*)deltas_out_dev,
                           label_idx_out_dev, match_idx_out_dev, onehot_out_dev);
        SSD_LAUNCH_CHECK();
        return SSD_OK;
    }
    SSD_HIP(hipMemsetAsync(workspace_dev, 0, need, st));
    if (G > 0) {                                             // B * G <= 65535 * 3072 workgroups
        AtssLevels lv;
        lv.n = cfg->n_levels;
        lv.topk = cfg->topk;
        for (int l = 0; l <= SSD_MATCH_MAX_LEVELS; ++l) lv.start[l] = l <= cfg->n_levels ? cfg->level_start[l] : N;
        hipLaunchKernelGGL(atss_candidates_kernel, dim3(B * G), dim3(kAtssThreads), 0, st, pri, gt, gt_labels_dev, N, G, lv,
                           (u64*)workspace_dev);
        SSD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(assign_kernel<SSD_MATCH_ATSS>, grid, dim3(256), 0, st, pri, gt, gt_labels_dev, v4, 0.0f, N, G, L,
                       (const void*)workspace_dev, (float4*)deltas_out_dev, label_idx_out_dev, match_idx_out_dev,
                       onehot_out_dev);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

}  // extern "C"
