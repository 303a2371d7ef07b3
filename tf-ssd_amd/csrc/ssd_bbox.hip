// Box-math kernels for gfx950: prior boxes, decode, class-mask + threshold compaction,
// per-class greedy NMS (bitonic sort + ballot suppression), per-image top-K merge,
// pairwise IoU and target matching.  HBM/latency-bound integer + fp32 work: wavefront
// primitives (64-wide ballot / shuffle / popcount), LDS staging, no MFMA.
//
// Built with -ffp-contract=off: every product and sum is rounded separately, exactly as
// the reference's chain of elementwise TF ops does (utils/bbox_utils.py), so that anchor
// indices kept by NMS and match indices are bit-exact against the oracle.
#include "box_math.h"
#include "common.h"

#include <algorithm>
#include <cmath>

namespace ssd {

// ------------------------------------------------------------------ shared device math
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

// ------------------------------------------------- decode + class mask + compaction (D3)
// One block = 256 consecutive anchors of one image.  The [256, L] probability slab is
// contiguous in HBM: it is staged through LDS with coalesced loads, then each lane walks
// its own row (row stride L words: conflict-free for odd L such as 21).
// Candidates (score > thr, strict) are appended to the per-(image,class) list with one
// atomic each; the later sort makes the result independent of the append order.
// softmax of one row in place (models/header.py:66 `Activation("softmax")`): THE definition of the net's class
// probabilities -- softmax_kernel (ssd_net_forward's output) and the fused compact kernel of ssd_net_predict both call
// it from this translation unit, so the two paths produce the same bits
__device__ __forceinline__ void softmax_row(float* row, const int L) {
    float mx = row[0];
    for (int c = 1; c < L; ++c) mx = fmaxf(mx, row[c]);
    float s = 0.f;
    for (int c = 0; c < L; ++c) {
        const float ev = expf(row[c] - mx);
        row[c] = ev;
        s += ev;
    }
    for (int c = 0; c < L; ++c) row[c] = row[c] / s;
}

// 256 rows per block staged through LDS (coalesced in/out); one lane per row.
__global__ __launch_bounds__(256) void softmax_kernel(const float* __restrict__ in, const long rows,
                                                      const int L, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const long r0 = (long)blockIdx.x * 256;
    const int nrows = (int)min((long)256, rows - r0);
    const int n = nrows * L;
    const float* src = in + r0 * L;
    for (int e = threadIdx.x; e < n; e += 256) tile[e] = src[e];
    __syncthreads();
    if ((int)threadIdx.x < nrows) softmax_row(tile + threadIdx.x * L, L);
    __syncthreads();
    float* dst = out + r0 * L;
    for (int e = threadIdx.x; e < n; e += 256) dst[e] = tile[e];
}

// LOGITS (ssd_net_predict): `probs` holds the head convs' LOGITS; the softmax runs on the LDS-staged slab right here
// (no separate softmax pass over the [B, N, L] buffer, no launch); needs use_lds.
// AGN (class-agnostic suppression): one list per image, `cap` = N * L, the key already in the selection kernel's form
// [score desc : 32][anchor : 22][class : 10]; the image's counter is cand_count[b].
template <bool DECODE, bool LOGITS, bool AGN = false>
__global__ __launch_bounds__(256) void compact_kernel(
    const float4* __restrict__ deltas, const float* __restrict__ probs,
    const float4* __restrict__ priors, const float4 var, const int N, const int L,
    const float score_thr, const int use_lds, float4* __restrict__ boxes_out,
    unsigned long long* __restrict__ cand_keys, int* __restrict__ cand_count, const int cap) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int b = blockIdx.y;
    const int i0 = blockIdx.x * 256;
    const int rows = min(256, N - i0);
    const float* src = probs + ((size_t)b * N + i0) * L;
    if (use_lds) {
        const int n = rows * L;
        for (int e = threadIdx.x; e < n; e += 256) tile[e] = src[e];
        __syncthreads();
    }
    const int t = threadIdx.x;
    if (t >= rows) return;
    const int i = i0 + t;
    if (LOGITS) softmax_row(tile + t * L, L);
    const float* row = use_lds ? (tile + t * L) : (src + (size_t)t * L);
    bool masked = false;
    if (DECODE) {
        // models/decoder.py:44-45: argmax (first max wins) == 0 -> zero the whole row.
        int am = 0;
        float best = row[0];
        for (int c = 1; c < L; ++c) {
            const float v = row[c];
            if (v > best) { best = v; am = c; }
        }
        masked = (am == 0);
    }
    bool any = false;
    for (int c = 0; c < L; ++c) {
        const float s = masked ? 0.0f : row[c];
        if (s > score_thr) {
            if (AGN) {
                const int slot = atomicAdd(&cand_count[b], 1);
                if (slot < cap)
                    cand_keys[(size_t)b * cap + slot] = ((unsigned long long)score_desc_key(s) << 32) |
                                                        ((unsigned)i << kClsBits) | (unsigned)c;
            } else {
                const int slot = atomicAdd(&cand_count[b * L + c], 1);
                if (slot < cap)
                    cand_keys[((size_t)b * L + c) * cap + slot] =
                        ((unsigned long long)score_desc_key(s) << 32) | (unsigned)i;
            }
            any = true;
        }
    }
    if (DECODE && any)
        boxes_out[(size_t)b * N + i] = decode_box(priors[i], deltas[(size_t)b * N + i], var, true);
}

// ------------------------------------------------------------------ block-wide sort
// "Normalized" bitonic network (every merge ascending; first sub-step mirrored), which
// sorts any n in place with no padding: a comparator whose upper index is >= n is a no-op.
// 256 threads; keys may live in LDS or in global memory (big-n fallback).
template <typename K>
__device__ void block_sort_asc(K* keys, const int n) {
    if (n < 2) { __syncthreads(); return; }
    int P = 2;
    while (P < n) P <<= 1;
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        const int hk = k >> 1;
        for (int t = threadIdx.x; t < half; t += blockDim.x) {
            const int blk = t / hk, pos = t - blk * hk;
            const int i = blk * k + pos;
            const int l = blk * k + (k - 1 - pos);
            if (l < n) {
                const K a = keys[i], c = keys[l];
                if (a > c) { keys[i] = c; keys[l] = a; }
            }
        }
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += blockDim.x) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i + j;
                if (l < n) {
                    const K a = keys[i], c = keys[l];
                    if (a > c) { keys[i] = c; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ per-class greedy NMS
// One 256-thread block per (image, class).  Sorted candidates are consumed in chunks of
// 256: (1) every thread tests its candidate against the boxes already kept (LDS list);
// (2) the survivors are compacted with ballot + popcount prefix; (3) wave 0 resolves the
// survivors in score order: the lowest set bit of the 64-wide alive ballot is kept, its
// box is broadcast by readlane and the remaining lanes clear their alive bit if IoU > thr.
constexpr int kSortLds = 4096;   // candidates sorted in LDS (32 KB); above: in place in HBM

__global__ __launch_bounds__(256) void nms_class_kernel(
    unsigned long long* __restrict__ cand_keys, int* __restrict__ cand_count,
    const float4* __restrict__ boxes, const int N, const int L, const int cap, const int maxk,
    const float iou_thr, unsigned long long* __restrict__ kept_keys, int* __restrict__ kept_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* kept_box = reinterpret_cast<float4*>(smem);                       // [maxk]
    float4* surv_box = kept_box + maxk;                                       // [256]
    unsigned long long* surv_key = reinterpret_cast<unsigned long long*>(surv_box + 256);   // [256]
    unsigned long long* skeys = surv_key + 256;                               // [kSortLds]
    int* s_misc = reinterpret_cast<int*>(skeys + kSortLds);                   // [8]

    const int bc = blockIdx.x;          // b * L + c
    const int b = bc / L, c = bc - b * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(cand_count[bc], cap);
    // every thread has read the count: its (image, class) owner resets it, so the NEXT call on this workspace starts from
    // zero without a memset launch (the net's predict path; a caller-owned workspace is still zeroed by the launcher)
    __syncthreads();
    if (tid == 0) cand_count[bc] = 0;
    if (n == 0) {
        if (tid == 0) kept_count[bc] = 0;
        return;
    }
    unsigned long long* gkeys = cand_keys + (size_t)bc * cap;
    unsigned long long* keys;
    if (n <= kSortLds) {
        for (int i = tid; i < n; i += 256) skeys[i] = gkeys[i];
        __syncthreads();
        keys = skeys;
    } else {
        keys = gkeys;
    }
    block_sort_asc(keys, n);

    const float4* img_boxes = boxes + (size_t)b * N;
    unsigned long long* out_keys = kept_keys + (size_t)bc * maxk;
    int kept = 0;
    for (int base = 0; base < n && kept < maxk; base += 256) {
        const int j = base + tid;
        bool alive = j < n;
        unsigned long long key = 0;
        float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
        if (alive) {
            key = keys[j];
            box = img_boxes[(unsigned)(key & 0xffffffffu)];
            for (int q = kept - 1; q >= 0; --q)
                if (nms_iou(box, kept_box[q]) > iou_thr) { alive = false; break; }
        }
        const unsigned long long m = __ballot(alive);
        if (lane == 0) s_misc[wave] = __popcll(m);
        __syncthreads();
        int off = 0;
        for (int w = 0; w < wave; ++w) off += s_misc[w];
        const int nsurv = s_misc[0] + s_misc[1] + s_misc[2] + s_misc[3];
        if (alive) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
            surv_box[pos] = box;
            surv_key[pos] = key;
        }
        __syncthreads();
        if (wave == 0) {
            const int chunk_start = kept;
            for (int sb = 0; sb < nsurv && kept < maxk; sb += 64) {
                const int p = sb + lane;
                bool a = p < nsurv;
                float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
                unsigned long long ky = 0;
                if (a) {
                    bx = surv_box[p];
                    ky = surv_key[p];
                    for (int q = kept - 1; q >= chunk_start; --q)
                        if (nms_iou(bx, kept_box[q]) > iou_thr) { a = false; break; }
                }
                unsigned long long mask = __ballot(a);
                while (mask != 0ull && kept < maxk) {
                    const int jl = __ffsll((long long)mask) - 1;
                    float4 kb;
                    kb.x = __shfl(bx.x, jl);
                    kb.y = __shfl(bx.y, jl);
                    kb.z = __shfl(bx.z, jl);
                    kb.w = __shfl(bx.w, jl);
                    if (lane == jl) {
                        kept_box[kept] = bx;
                        // merge key: [score desc : 32][anchor : 22][class : 10]
                        out_keys[kept] = (ky & 0xffffffff00000000ull) |
                                         ((ky & 0xffffffffull) << kClsBits) | (unsigned)c;
                    }
                    ++kept;
                    if (a && lane > jl && nms_iou(bx, kb) > iou_thr) a = false;
                    mask = __ballot(a) & ~((2ull << jl) - 1ull);
                }
            }
            if (lane == 0) s_misc[4] = kept;
        }
        __syncthreads();
        kept = s_misc[4];
        __syncthreads();
    }
    if (tid == 0) kept_count[bc] = kept;
}

// ------------------------------------------------------------------ Soft-NMS / class-agnostic selection
// include/ssd_hip.h states the arithmetic.  The order of a list is not fixed in advance (every selection changes the
// scores that are left), so nothing is sorted: one 256-thread block per list keeps the candidates as u64 keys
// [score_desc_key(CURRENT score) : 32][anchor : 22][class : 10] -- the minimum key IS the winner under the tie rule, and
// (anchor, class) makes every key of a list unique -- and thread t owns the slots t, t + 256, ..., of which the first
// `cnt` are alive.  One selection = one pass of every thread over its own live slots (drop the last winner, decay the
// others by it, drop what left the list, move the survivors down to the front of the thread's stripe, keep the running
// minimum and ITS box in registers) + a minimum over the block: DPP and readlane within the wave (wave_min_u64), then
// one (key, box) pair per wave through a double-buffered LDS slot, so a selection costs ONE barrier (the pairs of
// selection k + 1 go to the other buffer while late threads still read those of k).  The winner's box travels with its
// key, so no thread reads another thread's slots and the per-stripe compaction needs no synchronisation; a pass costs what
// is still alive, not what the list started with.  Lists of up to `lds_cap` (<= kSoftLds) candidates hold keys and boxes
// in LDS (24 B a candidate, 96 KiB at kSoftLds); longer ones keep the keys where the compaction left them in the workspace
// (rewritten in place) and gather the boxes by anchor -- the same loop, two pointers.
// Cost: selections x (live candidates / 256 box tests per thread + the wave minimum + one barrier), nothing but the list's
// own latency; B * L (or B) blocks, occupancy is not the concern.
constexpr int kSoftLds = 4096;
constexpr unsigned long long kDeadKey = ~0ull;    // no candidate has it: score_desc_key is 0xffffffff for a NaN only
enum { kNmsHard = 0, kNmsGaussian = 1, kNmsLinear = 2 };     // SSD_NMS_*

// minimum over the wave, the same value in every lane.  Within a row of 16 lanes by DPP (quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror, row_mirror: every lane ends with its row's minimum), then the four rows by readlane + scalar compares:
// no LDS crossbar (ds_bpermute) on the loop's critical path -- six dependent __shfl_xor pairs cost ~1500 of the ~2500
// cycles a selection took with them
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_min_u64(unsigned long long v) {
    const int lo = (int)(unsigned)(v & 0xffffffffull), hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o < v ? o : v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    v = dpp_min_u64<0xb1>(v);
    v = dpp_min_u64<0x4e>(v);
    v = dpp_min_u64<0x141>(v);
    v = dpp_min_u64<0x140>(v);
    const int lo = (int)(unsigned)(v & 0xffffffffull), hi = (int)(unsigned)(v >> 32);
    unsigned long long r = ~0ull;
#pragma unroll
    for (int row = 0; row < 64; row += 16) {
        const unsigned long long o = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, row) << 32) |
                                     (unsigned)__builtin_amdgcn_readlane(lo, row);
        r = o < r ? o : r;
    }
    return r;
}

__device__ __forceinline__ float4 readlane_box(const float4 v, const int src) {
    float4 r;
    r.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.x), src));
    r.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.y), src));
    r.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.z), src));
    r.w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v.w), src));
    return r;
}

template <int METHOD>
__global__ __launch_bounds__(256) void soft_nms_kernel(
    unsigned long long* __restrict__ cand_keys, int* __restrict__ cand_count, const float4* __restrict__ boxes,
    const int N, const int L, const int agnostic, const int cap, const int lds_cap, const int limit,
    const int kept_stride, const float iou_thr, const float score_thr, const float scale,
    unsigned long long* __restrict__ kept_keys, int* __restrict__ kept_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* sbox = reinterpret_cast<float4*>(smem);                                         // [lds_cap]
    unsigned long long* skeys = reinterpret_cast<unsigned long long*>(sbox + lds_cap);      // [lds_cap]
    __shared__ __attribute__((aligned(16))) float4 x_box[2][4];
    __shared__ unsigned long long x_key[2][4];

    const int list = blockIdx.x;        // b * L + c, or b
    const int b = agnostic ? list : list / L;
    const unsigned c = agnostic ? 0u : (unsigned)(list - b * L);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(cand_count[list], cap);
    // as nms_class_kernel: the list's owner leaves its counter at zero for the next call on this workspace
    __syncthreads();
    if (tid == 0) cand_count[list] = 0;
    if (n == 0) {
        if (tid == 0) kept_count[list] = 0;
        return;
    }
    unsigned long long* gkeys = cand_keys + (size_t)list * cap;
    const bool in_lds = n <= lds_cap;
    unsigned long long* keys = in_lds ? skeys : gkeys;
    const float4* img_boxes = boxes + (size_t)b * N;
    unsigned long long local = kDeadKey;        // this thread's best live key and that candidate's box
    float4 lbox = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;                                // live slots of this thread: tid + 256 * i, i < cnt
    for (int j = tid; j < n; j += 256, ++cnt) {
        unsigned long long k = gkeys[j];
        if (!agnostic) k = (k & 0xffffffff00000000ull) | ((k & 0xffffffffull) << kClsBits) | c;
        keys[j] = k;
        if (in_lds) {
            const float4 box = img_boxes[(unsigned)(k & 0xffffffffull) >> kClsBits];
            sbox[j] = box;
            if (k < local) lbox = box;
        }
        if (k < local) local = k;
    }
    if (!in_lds && local != kDeadKey) lbox = img_boxes[(unsigned)(local & 0xffffffffull) >> kClsBits];
    unsigned long long* out_keys = kept_keys + (size_t)list * kept_stride;
    const int lim = min(min(limit, n), kept_stride);
    int sel = 0, buf = 0;
    for (; sel < lim; ++sel) {
        const unsigned long long wm = wave_min_u64(local);
        // the first lane that holds the wave's minimum hands over its box (all lanes hold the dead key: any box, never used)
        const float4 wave_box = readlane_box(lbox, __ffsll((long long)__ballot(local == wm)) - 1);
        if (lane == 0) { x_key[buf][wave] = wm; x_box[buf][wave] = wave_box; }
        __syncthreads();
        unsigned long long wk = x_key[buf][0];
        int ww = 0;
        for (int w = 1; w < 4; ++w) {
            const unsigned long long k = x_key[buf][w];
            if (k < wk) { wk = k; ww = w; }
        }
        if (wk == kDeadKey) break;          // nothing alive (the same value in every thread)
        if (tid == 0) out_keys[sel] = wk;
        const float4 wbox = x_box[buf][ww];
        local = kDeadKey;
        int live = 0;
        for (int i = 0; i < cnt; ++i) {
            const int j = tid + 256 * i;
            unsigned long long k = keys[j];
            if (k == wk) continue;          // the winner leaves (keys are unique)
            const float4 box = in_lds ? sbox[j] : img_boxes[(unsigned)(k & 0xffffffffull) >> kClsBits];
            const float o = nms_iou(box, wbox);
            if (METHOD == kNmsHard) {
                if (o > iou_thr) continue;
            } else {
                float s = score_from_key((unsigned)(k >> 32));
                if (METHOD == kNmsLinear) {
                    if (o > iou_thr) s = s * (1.0f - o);
                } else {
                    s = s * expf((scale * o) * o);
                }
                if (!(s > score_thr)) continue;
                k = ((unsigned long long)score_desc_key(s) << 32) | (k & 0xffffffffull);
            }
            // survivor: down to the front of this thread's stripe
            const int jd = tid + 256 * live;
            if (METHOD != kNmsHard || live != i) keys[jd] = k;
            if (in_lds && live != i) sbox[jd] = box;
            if (k < local) { local = k; lbox = box; }
            ++live;
        }
        cnt = live;
        buf ^= 1;
    }
    if (tid == 0) kept_count[list] = sel;
}

// ------------------------------------------------------------------ per-image top-K merge
// One block per image: gather the kept (score, anchor, class) keys of all classes, sort,
// emit the first max_total rows (boxes clipped to [0,1] when clip), zero-pad the rest.
__global__ __launch_bounds__(256) void merge_topk_kernel(
    const unsigned long long* __restrict__ kept_keys, const int* __restrict__ kept_count,
    const float4* __restrict__ boxes, const int N, const int L, const int maxk,
    const int max_total, const int clip, const int use_lds,
    unsigned long long* __restrict__ merge_ws, float4* __restrict__ out_boxes,
    float* __restrict__ out_labels, float* __restrict__ out_scores, int* __restrict__ out_valid,
    int* __restrict__ out_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* s_off = reinterpret_cast<int*>(smem);                                  // [L + 1]
    unsigned long long* lkeys =
        reinterpret_cast<unsigned long long*>(smem + ((size_t)(L + 1) * 4 + 15) / 16 * 16);
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int acc = 0;
        for (int c = 0; c < L; ++c) { s_off[c] = acc; acc += kept_count[b * L + c]; }
        s_off[L] = acc;
    }
    __syncthreads();
    const int total = s_off[L];
    unsigned long long* keys = use_lds ? lkeys : (merge_ws + (size_t)b * L * maxk);
    for (int c = 0; c < L; ++c) {
        const int cnt = s_off[c + 1] - s_off[c];
        const unsigned long long* src = kept_keys + ((size_t)b * L + c) * maxk;
        for (int i = tid; i < cnt; i += 256) keys[s_off[c] + i] = src[i];
    }
    __syncthreads();
    block_sort_asc(keys, total);
    const int nv = min(total, max_total);
    if (tid == 0) out_valid[b] = nv;
    for (int r = tid; r < max_total; r += 256) {
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        float lab = 0.f, sc = 0.f;
        int idx = -1;
        if (r < nv) {
            const unsigned long long k = keys[r];
            const unsigned lo = (unsigned)(k & 0xffffffffull);
            idx = (int)(lo >> kClsBits);
            lab = (float)(lo & ((1u << kClsBits) - 1u));
            sc = score_from_key((unsigned)(k >> 32));
            bx = boxes[(size_t)b * N + idx];
            if (clip) {
                bx.x = fminf(fmaxf(bx.x, 0.0f), 1.0f);
                bx.y = fminf(fmaxf(bx.y, 0.0f), 1.0f);
                bx.z = fminf(fmaxf(bx.z, 0.0f), 1.0f);
                bx.w = fminf(fmaxf(bx.w, 0.0f), 1.0f);
            }
        }
        out_boxes[(size_t)b * max_total + r] = bx;
        out_labels[(size_t)b * max_total + r] = lab;
        out_scores[(size_t)b * max_total + r] = sc;
        if (out_idx) out_idx[(size_t)b * max_total + r] = idx;
    }
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

// ------------------------------------------------------------------ host side
struct NmsWs {
    int* cand_count;
    int* kept_count;
    unsigned long long* cand_keys;
    unsigned long long* kept_keys;
    unsigned long long* merge_ws;
    float4* boxes;
    size_t bytes;
};

static NmsWs carve_ws(void* base, int B, int N, int L, int maxk) {
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

static int check_nms_args(int B, int N, int L, int max_per_class, int max_total) {
    SSD_CHECK_ARG(B >= 0 && N >= 0 && L >= 1, "decode_nms: bad sizes B=%d N=%d L=%d", B, N, L);
    SSD_CHECK_ARG(max_per_class >= 1 && max_total >= 1, "decode_nms: max_per_class=%d max_total=%d",
                  max_per_class, max_total);
    SSD_UNSUPPORTED_IF(N >= (1 << kIdxBits), "decode_nms: N=%d exceeds %d anchors", N, 1 << kIdxBits);
    SSD_UNSUPPORTED_IF(L > (1 << kClsBits), "decode_nms: L=%d exceeds %d classes", L, 1 << kClsBits);
    return SSD_OK;
}

// Shared driver: DECODE=true -> SSDDecoder path; false -> raw combined NMS.
// flags (the net's own predict path): kNmsLogits -- `scores` holds logits, softmax fused into the compaction;
// kNmsCountsClean -- the workspace's candidate counters are known to be zero (zeroed at allocation, re-zeroed by
// nms_class_kernel of the previous call): no memset launch
// mode (NULL: the reference's hard per-class NMS, the launches below as they always were): Soft-NMS and / or one pooled
// list per image -- the compaction's AGN form, soft_nms_kernel in place of nms_class_kernel, the same merge
enum { kNmsLogits = 1, kNmsCountsClean = 2 };
struct NmsMode { int method; int agnostic; float scale; };
static int run_nms(bool decode, const float* deltas, const float* scores, const float* priors_or_boxes,
                   const float* var, int B, int N, int L, int max_per_class, int max_total,
                   float iou_thr, float score_thr, int clip, float* boxes_out, float* labels_out,
                   float* scores_out, int* valid_out, int* kept_idx, void* ws, size_t ws_bytes,
                   hipStream_t st, int flags = 0, int ws_batch = 0, const NmsMode* mode = nullptr) {
    int rc = check_nms_args(B, N, L, max_per_class, max_total);
    if (rc) return rc;
    const bool agn = mode && mode->agnostic;
    SSD_UNSUPPORTED_IF(agn && (long)N * L > 0x7fffffffL, "decode_nms: N=%d x L=%d candidates in one class-agnostic list", N, L);
    if (B == 0) return SSD_OK;
    if (N == 0) {   // nothing to select: all-zero outputs
        SSD_HIP(hipMemsetAsync(boxes_out, 0, (size_t)B * max_total * 16, st));
        SSD_HIP(hipMemsetAsync(labels_out, 0, (size_t)B * max_total * 4, st));
        SSD_HIP(hipMemsetAsync(scores_out, 0, (size_t)B * max_total * 4, st));
        SSD_HIP(hipMemsetAsync(valid_out, 0, (size_t)B * 4, st));
        if (kept_idx) SSD_HIP(hipMemsetAsync(kept_idx, 0xff, (size_t)B * max_total * 4, st));
        return SSD_OK;
    }
    const int maxk = max_per_class < N ? max_per_class : N;
    const size_t nms_lds = (size_t)maxk * 16 + 256 * 16 + 256 * 8 + (size_t)kSortLds * 8 + 64;
    SSD_UNSUPPORTED_IF(nms_lds > 160 * 1024, "decode_nms: max_per_class=%d needs %zu B of LDS",
                       max_per_class, nms_lds);
    SSD_CHECK_ARG(ws != nullptr, "decode_nms: workspace is NULL");
    // the workspace is carved for ws_batch images when given (>= B): with kNmsCountsClean the counters have to sit at the
    // same place whatever batch a call runs (a layout carved for a smaller B would put its kept counts where a larger
    // batch's candidate counters live)
    SSD_CHECK_ARG(ws_batch == 0 || ws_batch >= B, "decode_nms: workspace carved for %d images, batch %d", ws_batch, B);
    NmsWs w = carve_ws(ws, ws_batch ? ws_batch : B, N, L, maxk);
    SSD_CHECK_ARG(ws_bytes >= w.bytes, "decode_nms: workspace %zu < required %zu", ws_bytes, w.bytes);
    SSD_CHECK_ARG(((uintptr_t)ws & 15) == 0, "decode_nms: workspace must be 16-byte aligned");

    if (!(flags & kNmsCountsClean)) SSD_HIP(hipMemsetAsync(w.cand_count, 0, (size_t)B * L * 4, st));
    const float4 v4 = var ? make_float4(var[0], var[1], var[2], var[3]) : make_float4(1, 1, 1, 1);
    const size_t tile_bytes = (size_t)256 * L * 4;
    const int use_lds = tile_bytes <= 96 * 1024;
    SSD_CHECK_ARG(!(flags & kNmsLogits) || (decode && use_lds), "decode_nms: fused softmax needs the LDS-staged decoder path");
    if (tile_bytes > 64 * 1024 && use_lds) {
        SSD_HIP(hipFuncSetAttribute((const void*)compact_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
        SSD_HIP(hipFuncSetAttribute((const void*)compact_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
        SSD_HIP(hipFuncSetAttribute((const void*)compact_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
        SSD_HIP(hipFuncSetAttribute((const void*)compact_kernel<true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
        SSD_HIP(hipFuncSetAttribute((const void*)compact_kernel<true, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
        SSD_HIP(hipFuncSetAttribute((const void*)compact_kernel<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes));
    }
    dim3 grid(cdiv(N, 256), B);
    if (agn) {
        // one list per image: N * L keys, the image's slice of the cand_keys carve
        const float4* d4 = decode ? (const float4*)deltas : nullptr;
        const float4* p4 = decode ? (const float4*)priors_or_boxes : nullptr;
        float4* bo = decode ? w.boxes : nullptr;
        if (decode && (flags & kNmsLogits))
            hipLaunchKernelGGL((compact_kernel<true, true, true>), grid, dim3(256), tile_bytes, st, d4, scores, p4, v4, N, L,
                               score_thr, use_lds, bo, w.cand_keys, w.cand_count, N * L);
        else if (decode)
            hipLaunchKernelGGL((compact_kernel<true, false, true>), grid, dim3(256), use_lds ? tile_bytes : 0, st, d4, scores,
                               p4, v4, N, L, score_thr, use_lds, bo, w.cand_keys, w.cand_count, N * L);
        else
            hipLaunchKernelGGL((compact_kernel<false, false, true>), grid, dim3(256), use_lds ? tile_bytes : 0, st, d4, scores,
                               p4, v4, N, L, score_thr, use_lds, bo, w.cand_keys, w.cand_count, N * L);
    } else if (decode && (flags & kNmsLogits)) {
        hipLaunchKernelGGL((compact_kernel<true, true>), grid, dim3(256), tile_bytes, st,
                           (const float4*)deltas, scores, (const float4*)priors_or_boxes, v4, N, L,
                           score_thr, use_lds, w.boxes, w.cand_keys, w.cand_count, N);
    } else if (decode) {
        hipLaunchKernelGGL((compact_kernel<true, false>), grid, dim3(256), use_lds ? tile_bytes : 0, st,
                           (const float4*)deltas, scores, (const float4*)priors_or_boxes, v4, N, L,
                           score_thr, use_lds, w.boxes, w.cand_keys, w.cand_count, N);
    } else {
        hipLaunchKernelGGL((compact_kernel<false, false>), grid, dim3(256), use_lds ? tile_bytes : 0, st,
                           (const float4*)nullptr, scores, (const float4*)nullptr, v4, N, L,
                           score_thr, use_lds, (float4*)nullptr, w.cand_keys, w.cand_count, N);
    }
    SSD_LAUNCH_CHECK();
    const float4* nms_boxes = decode ? w.boxes : (const float4*)priors_or_boxes;
    if (mode) {
        const int lists = agn ? B : B * L;
        const int cap = agn ? N * L : N;
        const int kept_stride = agn ? L * maxk : maxk;      // an image's (class's) slice of the kept_keys carve
        const int limit = agn ? std::min(std::min(max_per_class, max_total), kept_stride) : maxk;
        const int lds_cap = std::min(cap, kSoftLds);
        const size_t lds = (size_t)lds_cap * 24;
        const void* fn = mode->method == kNmsHard ? (const void*)soft_nms_kernel<kNmsHard>
                         : mode->method == kNmsLinear ? (const void*)soft_nms_kernel<kNmsLinear>
                                                      : (const void*)soft_nms_kernel<kNmsGaussian>;
        if (lds > 64 * 1024) SSD_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(lists), dim3(256), lds, st, w.cand_keys, w.cand_count, nms_boxes, N, L,
                               agn ? 1 : 0, cap, lds_cap, limit, kept_stride, iou_thr, score_thr, mode->scale, w.kept_keys,
                               w.kept_count);
        };
        if (mode->method == kNmsHard) launch(soft_nms_kernel<kNmsHard>);
        else if (mode->method == kNmsLinear) launch(soft_nms_kernel<kNmsLinear>);
        else launch(soft_nms_kernel<kNmsGaussian>);
        SSD_LAUNCH_CHECK();
        // the merge of an agnostic image: ONE list of up to kept_stride rows, already in order
        const int mL = agn ? 1 : L;
        const size_t mkeys = (size_t)mL * kept_stride * 8;
        const size_t mhdr = align_up((size_t)(mL + 1) * 4, 16);
        const int mlds_ok = mhdr + mkeys <= 64 * 1024;
        hipLaunchKernelGGL(merge_topk_kernel, dim3(B), dim3(256), mhdr + (mlds_ok ? mkeys : 0), st, w.kept_keys, w.kept_count,
                           nms_boxes, N, mL, kept_stride, max_total, clip, mlds_ok, w.merge_ws, (float4*)boxes_out, labels_out,
                           scores_out, valid_out, kept_idx);
        SSD_LAUNCH_CHECK();
        return SSD_OK;
    }
    if (nms_lds > 64 * 1024)
        SSD_HIP(hipFuncSetAttribute((const void*)nms_class_kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)nms_lds));
    hipLaunchKernelGGL(nms_class_kernel, dim3(B * L), dim3(256), nms_lds, st, w.cand_keys,
                       w.cand_count, nms_boxes, N, L, N, maxk, iou_thr, w.kept_keys, w.kept_count);
    SSD_LAUNCH_CHECK();
    const size_t merge_keys = (size_t)L * maxk * 8;
    const size_t merge_hdr = align_up((size_t)(L + 1) * 4, 16);
    const int merge_lds_ok = merge_hdr + merge_keys <= 64 * 1024;
    hipLaunchKernelGGL(merge_topk_kernel, dim3(B), dim3(256),
                       merge_hdr + (merge_lds_ok ? merge_keys : 0), st, w.kept_keys, w.kept_count,
                       nms_boxes, N, L, maxk, max_total, clip, merge_lds_ok, w.merge_ws,
                       (float4*)boxes_out, labels_out, scores_out, valid_out, kept_idx);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

// ssd_nms_config -> what run_nms takes: *use stays NULL for the reference's post-processor (HARD, per class), which then
// runs on its own kernels; SSD_E_INVALID for the arguments include/ssd_hip.h rejects
int nms_mode_of(const ssd_nms_config* cfg, NmsMode* mode, const NmsMode** use) {
    SSD_CHECK_ARG(cfg != nullptr, "nms config is NULL");
    SSD_CHECK_ARG(cfg->method == SSD_NMS_HARD || cfg->method == SSD_NMS_GAUSSIAN || cfg->method == SSD_NMS_LINEAR,
                  "nms config: unknown method %d", cfg->method);
    SSD_CHECK_ARG(cfg->method != SSD_NMS_GAUSSIAN || (std::isfinite(cfg->sigma) && cfg->sigma > 0.0f),
                  "nms config: sigma=%g (SSD_NMS_GAUSSIAN needs a finite sigma > 0)", (double)cfg->sigma);
    SSD_CHECK_ARG(cfg->iou_threshold >= 0.0f && cfg->iou_threshold <= 1.0f, "nms config: iou_threshold=%g outside [0, 1]",
                  (double)cfg->iou_threshold);
    mode->method = cfg->method;
    mode->agnostic = cfg->class_agnostic != 0;
    mode->scale = cfg->method == SSD_NMS_GAUSSIAN ? -0.5f / cfg->sigma : 0.0f;
    *use = (cfg->method == SSD_NMS_HARD && !mode->agnostic) ? nullptr : mode;
    return SSD_OK;
}

// The net's own predict path (csrc/ssd_net.hip): head LOGITS in, softmax fused into the compaction, no counter memset.
// `ws` is the net's workspace, zeroed at allocation.  Returns SSD_E_UNSUPPORTED when the fused form cannot run (L too
// large for the LDS-staged slab): the caller then runs the softmax layer + ssd_decode_nms.
bool decode_nms_fused_ok(int L) { return (size_t)256 * L * 4 <= 96 * 1024; }
int decode_nms_fused(const float* deltas, const float* logits, const float* priors, const float* var, int B, int N, int L,
                     int max_per_class, int max_total, float iou_thr, float score_thr, float* boxes, float* labels,
                     float* scores, int* valid, void* ws, size_t ws_bytes, int ws_batch, hipStream_t st) {
    return run_nms(true, deltas, logits, priors, var, B, N, L, max_per_class, max_total, iou_thr, score_thr, 1, boxes,
                   labels, scores, valid, nullptr, ws, ws_bytes, st, kNmsLogits | kNmsCountsClean, ws_batch);
}
int decode_nms_fused_cfg(const float* deltas, const float* logits, const float* priors, const float* var, int B, int N, int L,
                         const ssd_nms_config* cfg, float* boxes, float* labels, float* scores, int* valid, void* ws,
                         size_t ws_bytes, int ws_batch, hipStream_t st) {
    NmsMode mode;
    const NmsMode* m = nullptr;
    if (const int rc = nms_mode_of(cfg, &mode, &m)) return rc;
    return run_nms(true, deltas, logits, priors, var, B, N, L, cfg->max_per_class, cfg->max_total, cfg->iou_threshold,
                   cfg->score_threshold, 1, boxes, labels, scores, valid, nullptr, ws, ws_bytes, st,
                   kNmsLogits | kNmsCountsClean, ws_batch, m);
}
int launch_softmax_lds(const float* in, long rows, int L, float* out, hipStream_t st) {
    hipLaunchKernelGGL(softmax_kernel, dim3(cdiv(rows, 256)), dim3(256), (size_t)256 * L * 4, st, in, rows, L, out);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
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

size_t ssd_decode_nms_workspace_bytes(int B, int N, int L, int max_per_class) {
    if (B <= 0 || N <= 0 || L <= 0 || max_per_class <= 0) return 256;
    const int maxk = max_per_class < N ? max_per_class : N;
    return carve_ws(nullptr, B, N, L, maxk).bytes;
}

int ssd_decode_nms(const float* deltas_dev, const float* probs_dev, const float* priors_dev,
                   const float* var, int B, int N, int L, int max_per_class, int max_total,
                   float iou_thr, float score_thr, float* boxes_dev, float* labels_dev,
                   float* scores_dev, int* valid_dev, int* kept_idx_dev, void* workspace_dev,
                   size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(var != nullptr, "ssd_decode_nms: variances pointer is NULL");
    SSD_CHECK_ARG(B == 0 || (boxes_dev && labels_dev && scores_dev && valid_dev),
                  "ssd_decode_nms: NULL output pointer");
    SSD_CHECK_ARG(B == 0 || N == 0 || (deltas_dev && probs_dev && priors_dev),
                  "ssd_decode_nms: NULL input pointer");
    return run_nms(true, deltas_dev, probs_dev, priors_dev, var, B, N, L, max_per_class, max_total,
                   iou_thr, score_thr, 1, boxes_dev, labels_dev, scores_dev, valid_dev, kept_idx_dev,
                   workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int ssd_combined_nms(const float* boxes_dev, const float* scores_dev, int B, int N, int C,
                     int max_per_class, int max_total, float iou_thr, float score_thr, int clip_boxes,
                     float* boxes_out_dev, float* scores_out_dev, float* classes_out_dev,
                     int* valid_dev, int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes,
                     void* stream) {
    SSD_CHECK_ARG(B == 0 || (boxes_out_dev && scores_out_dev && classes_out_dev && valid_dev),
                  "ssd_combined_nms: NULL output pointer");
    SSD_CHECK_ARG(B == 0 || N == 0 || (boxes_dev && scores_dev), "ssd_combined_nms: NULL input pointer");
    return run_nms(false, nullptr, scores_dev, boxes_dev, nullptr, B, N, C, max_per_class, max_total,
                   iou_thr, score_thr, clip_boxes, boxes_out_dev, classes_out_dev, scores_out_dev,
                   valid_dev, kept_idx_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

size_t ssd_nms_config_bytes(void) { return sizeof(ssd_nms_config); }
int ssd_nms_lds_candidates(void) { return kSoftLds; }

size_t ssd_decode_nms_cfg_workspace_bytes(int B, int N, int L, const ssd_nms_config* cfg) {
    return ssd_decode_nms_workspace_bytes(B, N, L, cfg ? cfg->max_per_class : 0);
}

int ssd_decode_nms_cfg(const float* deltas_dev, const float* probs_dev, const float* priors_dev, const float* var,
                       int B, int N, int L, const ssd_nms_config* cfg, float* boxes_dev, float* labels_dev,
                       float* scores_dev, int* valid_dev, int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream) {
    NmsMode mode;
    const NmsMode* m = nullptr;
    if (const int rc = nms_mode_of(cfg, &mode, &m)) return rc;
    SSD_CHECK_ARG(var != nullptr, "ssd_decode_nms_cfg: variances pointer is NULL");
    SSD_CHECK_ARG(B == 0 || (boxes_dev && labels_dev && scores_dev && valid_dev), "ssd_decode_nms_cfg: NULL output pointer");
    SSD_CHECK_ARG(B == 0 || N == 0 || (deltas_dev && probs_dev && priors_dev), "ssd_decode_nms_cfg: NULL input pointer");
    return run_nms(true, deltas_dev, probs_dev, priors_dev, var, B, N, L, cfg->max_per_class, cfg->max_total,
                   cfg->iou_threshold, cfg->score_threshold, 1, boxes_dev, labels_dev, scores_dev, valid_dev, kept_idx_dev,
                   workspace_dev, workspace_bytes, (hipStream_t)stream, 0, 0, m);
}

int ssd_combined_nms_cfg(const float* boxes_dev, const float* scores_dev, int B, int N, int C, const ssd_nms_config* cfg,
                         float* boxes_out_dev, float* scores_out_dev, float* classes_out_dev, int* valid_dev,
                         int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    NmsMode mode;
    const NmsMode* m = nullptr;
    if (const int rc = nms_mode_of(cfg, &mode, &m)) return rc;
    SSD_CHECK_ARG(B == 0 || (boxes_out_dev && scores_out_dev && classes_out_dev && valid_dev),
                  "ssd_combined_nms_cfg: NULL output pointer");
    SSD_CHECK_ARG(B == 0 || N == 0 || (boxes_dev && scores_dev), "ssd_combined_nms_cfg: NULL input pointer");
    return run_nms(false, nullptr, scores_dev, boxes_dev, nullptr, B, N, C, cfg->max_per_class, cfg->max_total,
                   cfg->iou_threshold, cfg->score_threshold, cfg->clip_boxes, boxes_out_dev, classes_out_dev, scores_out_dev,
                   valid_dev, kept_idx_dev, workspace_dev, workspace_bytes, (hipStream_t)stream, 0, 0, m);
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
