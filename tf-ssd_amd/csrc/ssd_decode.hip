// The detection post-processor (SSDDecoder, models/decoder.py) for gfx950: softmax, decode + class mask + threshold
// compaction, per-class greedy NMS (bitonic sort + ballot suppression) or the Soft-NMS / class-agnostic selection kernel,
// per-image top-K merge.  HBM/latency-bound integer + fp32 work: wavefront primitives (64-wide ballot / shuffle /
// popcount, DPP), LDS staging, no MFMA.  Host side: ssd_decode.h plans a call (pure), the driver below launches the plan.
// Built with -ffp-contract=off and correctly rounded fp32 division like ssd_bbox.hip: every product and sum is rounded
// separately, exactly as the reference's chain of elementwise TF ops does (utils/bbox_utils.py), so that the anchor
// indices kept by NMS are bit-exact against the oracle.
#include "ssd_decode.h"

namespace ssd {

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
// Up to kSortLds (ssd_decode.h) candidates are sorted in LDS; above: in place in HBM.
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
constexpr unsigned long long kDeadKey = ~0ull;    // no candidate has it: score_desc_key is 0xffffffff for a NaN only

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

// ------------------------------------------------------------------ host side
// The driver: launches what nms_plan (ssd_decode.h) decided and decides nothing itself.  One table lookup per launch from
// the plan's kernel id; the LDS attribute is raised for the kernel about to run, and only where the plan says so.
using CompactFn = decltype(&compact_kernel<true, false>);
using SoftFn = decltype(&soft_nms_kernel<kNmsHard>);
static const CompactFn kCompactFn[2 * kCompactAgn] = {      // kCompactDecode, kCompactLogits, kCompactRaw; + kCompactAgn
    compact_kernel<true, false>,       compact_kernel<true, true>,       compact_kernel<false, false>,
    compact_kernel<true, false, true>, compact_kernel<true, true, true>, compact_kernel<false, false, true>};
static const SoftFn kSoftFn[3] = {soft_nms_kernel<kNmsHard>, soft_nms_kernel<kNmsGaussian>, soft_nms_kernel<kNmsLinear>};

static int raise_lds(const void* fn, const NmsLaunch& l) {
    if (l.raise) SSD_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds));
    return SSD_OK;
}

static int nms_launch(const NmsCall& c, const NmsPlan& p, hipStream_t st) {
    const int B = c.B, N = c.N, L = c.L, max_total = c.cfg.max_total;
    if (p.what == NmsPlan::kNothing) return SSD_OK;
    if (p.what == NmsPlan::kZeroFill) {
        SSD_HIP(hipMemsetAsync(c.boxes_out, 0, (size_t)B * max_total * 16, st));
        SSD_HIP(hipMemsetAsync(c.labels_out, 0, (size_t)B * max_total * 4, st));
        SSD_HIP(hipMemsetAsync(c.scores_out, 0, (size_t)B * max_total * 4, st));
        SSD_HIP(hipMemsetAsync(c.valid_out, 0, (size_t)B * 4, st));
        if (c.kept_idx) SSD_HIP(hipMemsetAsync(c.kept_idx, 0xff, (size_t)B * max_total * 4, st));
        return SSD_OK;
    }
    const NmsWs& w = p.ws;
    if (!c.counts_clean) SSD_HIP(hipMemsetAsync(w.cand_count, 0, (size_t)B * L * 4, st));
    const float4 v4 = c.var ? make_float4(c.var[0], c.var[1], c.var[2], c.var[3]) : make_float4(1, 1, 1, 1);
    const CompactFn compact = kCompactFn[p.compact.kernel];
    if (const int rc = raise_lds((const void*)compact, p.compact)) return rc;
    hipLaunchKernelGGL(compact, p.compact.grid, dim3(256), p.compact.lds, st, c.decode ? (const float4*)c.deltas : nullptr,
                       c.scores, c.decode ? (const float4*)c.priors_or_boxes : nullptr, v4, N, L, c.cfg.score_threshold,
                       p.use_lds, c.decode ? w.boxes : nullptr, w.cand_keys, w.cand_count, p.cap);
    SSD_LAUNCH_CHECK();
    const float4* nms_boxes = c.decode ? w.boxes : (const float4*)c.priors_or_boxes;
    if (p.select.kernel == kSelectClass) {
        if (const int rc = raise_lds((const void*)nms_class_kernel, p.select)) return rc;
        hipLaunchKernelGGL(nms_class_kernel, p.select.grid, dim3(256), p.select.lds, st, w.cand_keys, w.cand_count, nms_boxes,
                           N, L, p.cap, p.maxk, c.cfg.iou_threshold, w.kept_keys, w.kept_count);
    } else {
        const SoftFn soft = kSoftFn[p.select.kernel - kSelectSoft];
        if (const int rc = raise_lds((const void*)soft, p.select)) return rc;
        hipLaunchKernelGGL(soft, p.select.grid, dim3(256), p.select.lds, st, w.cand_keys, w.cand_count, nms_boxes, N, L, p.agn,
                           p.cap, p.lds_cap, p.limit, p.kept_stride, c.cfg.iou_threshold, c.cfg.score_threshold, p.scale,
                           w.kept_keys, w.kept_count);
    }
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_topk_kernel, p.merge.grid, dim3(256), p.merge.lds, st, w.kept_keys, w.kept_count, nms_boxes, N,
                       p.merge_L, p.kept_stride, max_total, p.clip, p.merge_in_lds, w.merge_ws, (float4*)c.boxes_out,
                       c.labels_out, c.scores_out, c.valid_out, c.kept_idx);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

// every entry point, public or the net's own predict path (csrc/ssd_net.hip), ends here: `who` names it in the NULL checks
int decode_nms(const NmsCall& c, const char* who, hipStream_t st) {
    SSD_CHECK_ARG(!c.decode || c.var != nullptr, "%s: variances pointer is NULL", who);
    SSD_CHECK_ARG(c.B == 0 || (c.boxes_out && c.labels_out && c.scores_out && c.valid_out), "%s: NULL output pointer", who);
    SSD_CHECK_ARG(c.B == 0 || c.N == 0 || (c.scores && c.priors_or_boxes && (!c.decode || c.deltas)), "%s: NULL input pointer", who);
    NmsPlan p;
    if (const int rc = nms_plan(c, &p)) return rc;
    return nms_launch(c, p, st);
}

int launch_softmax_lds(const float* in, long rows, int L, float* out, hipStream_t st) {
    hipLaunchKernelGGL(softmax_kernel, dim3(cdiv(rows, 256)), dim3(256), (size_t)256 * L * 4, st, in, rows, L, out);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

}  // namespace ssd

using namespace ssd;

// the two forms of a public call as records; the entry points without a config ask for {SSD_NMS_HARD, per class}
static NmsCall decoder_call(const float* deltas, const float* probs, const float* priors, const float* var, int B, int N, int L,
                            float* boxes, float* labels, float* scores, int* valid, int* kept_idx, void* ws, size_t ws_bytes) {
    return {.deltas = deltas, .scores = probs, .priors_or_boxes = priors, .var = var, .B = B, .N = N, .L = L, .decode = true,
            .boxes_out = boxes, .labels_out = labels, .scores_out = scores, .valid_out = valid, .kept_idx = kept_idx,
            .ws = ws, .ws_bytes = ws_bytes};
}
static NmsCall raw_call(const float* boxes, const float* scores, int B, int N, int C, float* boxes_out, float* scores_out,
                        float* classes_out, int* valid, int* kept_idx, void* ws, size_t ws_bytes) {
    return {.scores = scores, .priors_or_boxes = boxes, .B = B, .N = N, .L = C, .boxes_out = boxes_out,
            .labels_out = classes_out, .scores_out = scores_out, .valid_out = valid, .kept_idx = kept_idx, .ws = ws,
            .ws_bytes = ws_bytes};
}

extern "C" {

size_t ssd_decode_nms_workspace_bytes(int B, int N, int L, int max_per_class) {
    if (B <= 0 || N <= 0 || L <= 0 || max_per_class <= 0) return 256;
    return nms_carve(nullptr, B, N, L, max_per_class < N ? max_per_class : N).bytes;
}

int ssd_decode_nms(const float* deltas_dev, const float* probs_dev, const float* priors_dev, const float* var, int B, int N,
                   int L, int max_per_class, int max_total, float iou_thr, float score_thr, float* boxes_dev,
                   float* labels_dev, float* scores_dev, int* valid_dev, int* kept_idx_dev, void* workspace_dev,
                   size_t workspace_bytes, void* stream) {
    NmsCall c = decoder_call(deltas_dev, probs_dev, priors_dev, var, B, N, L, boxes_dev, labels_dev, scores_dev, valid_dev,
                             kept_idx_dev, workspace_dev, workspace_bytes);
    c.cfg = {SSD_NMS_HARD, 0, max_per_class, max_total, 1, iou_thr, score_thr, 0.0f};
    return decode_nms(c, "ssd_decode_nms", (hipStream_t)stream);
}

int ssd_combined_nms(const float* boxes_dev, const float* scores_dev, int B, int N, int C, int max_per_class, int max_total,
                     float iou_thr, float score_thr, int clip_boxes, float* boxes_out_dev, float* scores_out_dev,
                     float* classes_out_dev, int* valid_dev, int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes,
                     void* stream) {
    NmsCall c = raw_call(boxes_dev, scores_dev, B, N, C, boxes_out_dev, scores_out_dev, classes_out_dev, valid_dev,
                         kept_idx_dev, workspace_dev, workspace_bytes);
    c.cfg = {SSD_NMS_HARD, 0, max_per_class, max_total, clip_boxes, iou_thr, score_thr, 0.0f};
    return decode_nms(c, "ssd_combined_nms", (hipStream_t)stream);
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
    NmsCall c = decoder_call(deltas_dev, probs_dev, priors_dev, var, B, N, L, boxes_dev, labels_dev, scores_dev, valid_dev,
                             kept_idx_dev, workspace_dev, workspace_bytes);
    if (const int rc = nms_set_config(&c, cfg)) return rc;
    return decode_nms(c, "ssd_decode_nms_cfg", (hipStream_t)stream);
}

int ssd_combined_nms_cfg(const float* boxes_dev, const float* scores_dev, int B, int N, int C, const ssd_nms_config* cfg,
                         float* boxes_out_dev, float* scores_out_dev, float* classes_out_dev, int* valid_dev,
                         int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    NmsCall c = raw_call(boxes_dev, scores_dev, B, N, C, boxes_out_dev, scores_out_dev, classes_out_dev, valid_dev,
                         kept_idx_dev, workspace_dev, workspace_bytes);
    if (const int rc = nms_set_config(&c, cfg)) return rc;
    return decode_nms(c, "ssd_combined_nms_cfg", (hipStream_t)stream);
}

}  // extern "C"
