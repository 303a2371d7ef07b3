// Focal confidence loss (Keras CategoricalFocalCrossentropy(alpha, gamma) on probabilities) beside the reference's
// localisation term, parallel over anchors: ssd_focal_loss in include/ssd_hip.h states the arithmetic.
//
// No select is needed (every anchor counts), so the work is a grid of (anchor tile, image) instead of ssd_loss.hip's one
// workgroup per image.  A tile's y and q rows are contiguous in memory (tile * L floats each): they are copied into LDS
// with coalesced 16-byte loads and each thread then walks its own row there; the row stride is L | 1 floats, odd, so the
// 64 rows of a wave fall into different banks.  The gradient rows go back the same way.  Two launches, because an
// anchor's gradient is divided by the image's positive count:
//   focal_partial_kernel   per (image, tile): loss sum, Huber sum, the two positive counts -> workspace; ce_out, mask_out
//   focal_finish_kernel    every workgroup adds its image's partials in tile order (one fixed tree, so the same bits in
//                          every workgroup and at every grid size), tile 0 writes the two losses, all write gradients
// No floating-point atomics; an anchor's values depend on its own rows and on the image's two counts alone.
#include "common.h"
#include "loss_reduce.h"

namespace ssd {

constexpr int kFocalThreads = 256;
constexpr int kFocalWaves = kFocalThreads / 64;
// both LDS tiles of a workgroup together: two workgroups (and their reduction scratch) fit a CU's 160 KiB, and the
// dynamic allocation stays below the 64 KiB a plain launch may ask for
constexpr int kFocalTileBytes = 60 * 1024;

// anchors per workgroup: 256 (one per thread) while both tiles fit, else a multiple of the wave size; 0: rows too long
// for LDS (L > 119), the threads read their rows from memory directly
static int focal_staged_tile(int L) {
    const int t = kFocalTileBytes / (8 * (L | 1));
    return t >= kFocalThreads ? kFocalThreads : t / 64 * 64;
}

struct FocalPartial {
    float conf, loc;        // sum of the tile's per-anchor focal values / of its positives' Huber sums
    int pos_conf, pos_loc;
};

struct FocalParams {
    const float* yd;      // actual_deltas [B,N,4]           (nullable: skip the localisation term)
    const float* pd;      // pred_deltas   [B,N,4]
    const float* yl;      // actual_labels [B,N,L]           (nullable: skip the confidence term)
    const float* pp;      // pred_labels   [B,N,L] probabilities
    int B, N, L;
    int T, tiles, Ls;     // anchors per tile, tiles per image, LDS row stride (L | 1)
    float loc_alpha, alpha, gamma;
    float* loc_loss;      // [B] (nullable)
    float* conf_loss;     // [B] (nullable)
    float* ce_out;        // [B,N] per-anchor focal value (nullable)
    float* mask_out;      // [B,N] all ones (nullable)
    float* grad_deltas;   // [B,N,4] (nullable)
    float* grad_logits;   // [B,N,L] (nullable)
    float grad_scale;
    FocalPartial* part;   // workspace [B][tiles]
};

__device__ __forceinline__ int lds_index(int k, int L, int Ls) { return L == Ls ? k : (k / L) * Ls + k % L; }

// `count` contiguous floats (rows of L) from memory into LDS rows of stride Ls: 16-byte loads at the 16-byte boundaries
// of the source, single floats for the partial vectors at the two ends (nothing outside [src, src + count) is read)
__device__ __forceinline__ void stage_in(float* dst, const float* src, int count, int L, int Ls) {
    const int mis = (int)(((uintptr_t)src >> 2) & 3);
    const float4* a = reinterpret_cast<const float4*>(src - mis);
    const int nvec = (mis + count + 3) >> 2;
    const bool flat16 = mis == 0 && L == Ls;
    for (int v = threadIdx.x; v < nvec; v += kFocalThreads) {
        const int k0 = 4 * v - mis;
        if (k0 >= 0 && k0 + 4 <= count) {
            const float4 x = a[v];
            if (flat16) {
                reinterpret_cast<float4*>(dst)[v] = x;
            } else {
                dst[lds_index(k0, L, Ls)] = x.x;
                dst[lds_index(k0 + 1, L, Ls)] = x.y;
                dst[lds_index(k0 + 2, L, Ls)] = x.z;
                dst[lds_index(k0 + 3, L, Ls)] = x.w;
            }
        } else {
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j;
                if (k >= 0 && k < count) dst[lds_index(k, L, Ls)] = src[k];
            }
        }
    }
}
// and back (nothing outside [dst, dst + count) is written)
__device__ __forceinline__ void stage_out(float* dst, const float* src, int count, int L, int Ls) {
    const int mis = (int)(((uintptr_t)dst >> 2) & 3);
    float4* a = reinterpret_cast<float4*>(dst - mis);
    const int nvec = (mis + count + 3) >> 2;
    const bool flat16 = mis == 0 && L == Ls;
    for (int v = threadIdx.x; v < nvec; v += kFocalThreads) {
        const int k0 = 4 * v - mis;
        if (k0 >= 0 && k0 + 4 <= count) {
            float4 x;
            if (flat16) {
                x = reinterpret_cast<const float4*>(src)[v];
            } else {
                x.x = src[lds_index(k0, L, Ls)];
                x.y = src[lds_index(k0 + 1, L, Ls)];
                x.z = src[lds_index(k0 + 2, L, Ls)];
                x.w = src[lds_index(k0 + 3, L, Ls)];
            }
            a[v] = x;
        } else {
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j;
                if (k >= 0 && k < count) dst[k] = src[lds_index(k, L, Ls)];
            }
        }
    }
}

// One anchor's focal value f = sum_c (alpha * (1 - r_c)^gamma) * -(y_c * log r_c), added in class order, every operation
// rounded on its own.  A class with y_c == 0 adds exactly 0 and is skipped (no logf / powf for it).
__device__ __forceinline__ float focal_row(const float* y, const float* q, int L, float alpha, float gamma, bool& pos) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll 4
    for (int c = 0; c < L; ++c) s += q[c];
    float acc = 0.f;
    pos = false;
#pragma unroll 1        // one copy of the logf / powf path
    for (int c = 0; c < L; ++c) {
        const float yc = y[c];
        if (yc == 0.f) continue;
        if (c > 0) pos = true;
        const float r = fminf(fmaxf(q[c] / s, 1e-7f), 1.0f - 1e-7f);
        const float mod = gamma == 0.f ? 1.0f : powf(1.0f - r, gamma);
        acc += (alpha * mod) * -(yc * logf(r));
    }
    return acc;
}

// df/dr_c where q_c / s lies inside the clip range (bounds included), 0 outside it and where y_c == 0:
//   y_c * alpha * (gamma * (1 - r)^(gamma - 1) * log r - (1 - r)^gamma / r),   (1 - r)^(gamma - 1) = (1 - r)^gamma / (1 - r)
// gamma == 0: the first term is exactly 0 and the modulating factor exactly 1.
__device__ __forceinline__ float focal_dfdr(float yc, float qc, float s, float alpha, float gamma) {
#pragma clang fp contract(off)
    if (yc == 0.f) return 0.f;
    const float r = qc / s;
    if (!(r >= 1e-7f && r <= 1.0f - 1e-7f)) return 0.f;
    const float om = 1.0f - r;
    const float mod = gamma == 0.f ? 1.0f : powf(om, gamma);
    const float first = gamma == 0.f ? 0.f : gamma * (mod / om) * logf(r);
    return (yc * alpha) * (first - mod / r);
}

// The anchor's gradient row w.r.t. the LOGITS: through the renormalisation r = q / s and the softmax backward, the steps
// of ssd_loss_kernel phase D with g_c = df/dr_c.  g_c is evaluated once per class and parked in `g`; IN_PLACE: y, g and out
// are one row (the thread's y row in LDS), where a class with y_c == 0 already holds its g_c = 0.  Every element is read
// before it is overwritten.  The loop that may take the logf / powf path is not unrolled: one copy of that code.
template <bool IN_PLACE>
__device__ __forceinline__ void focal_row_grad(const float* y, const float* __restrict__ q, int L, float alpha, float gamma,
                                               float gce, float* g, float* out) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll 4
    for (int c = 0; c < L; ++c) s += q[c];
    // dL/dp_j = gce * (g_j / s - (sum_c g_c p_c) / s^2)
    float t = 0.f;
#pragma unroll 1
    for (int c = 0; c < L; ++c) {
        const float yc = y[c];
        if (yc == 0.f) {
            if (!IN_PLACE) g[c] = 0.f;
            continue;
        }
        const float gc = focal_dfdr(yc, q[c], s, alpha, gamma);
        g[c] = gc;
        if (gc != 0.f) t += gc * q[c];
    }
    const float ts = t / (s * s);
    // a class with g_c == 0 (nearly all of a one-hot row): 0 / s - ts = -ts, the same bits without the division
    const float dp0 = gce * (0.f - ts);
    float dot = 0.f;        // sum_j p_j dL/dp_j  (softmax backward)
#pragma unroll 4
    for (int c = 0; c < L; ++c) {
        const float gc = g[c];
        dot += q[c] * (gc != 0.f ? gce * (gc / s - ts) : dp0);
    }
#pragma unroll 4
    for (int c = 0; c < L; ++c) {
        const float gc = g[c];
        const float dp = gc != 0.f ? gce * (gc / s - ts) : dp0;
        out[c] = q[c] * (dp - dot);
    }
}

template <bool STAGED>
__global__ __launch_bounds__(kFocalThreads) void focal_partial_kernel(const FocalParams p) {
    extern __shared__ float4 focal_lds[];
    __shared__ float shf[kFocalWaves];
    __shared__ int shi[kFocalWaves];
    const int tid = threadIdx.x, L = p.L;
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int n0 = tile * p.T, cnt = min(p.T, p.N - n0);
    const long row0 = (long)b * p.N + n0;
    float* ly = reinterpret_cast<float*>(focal_lds);
    float* lq = ly + p.T * p.Ls;
    if (STAGED && p.yl) {
        stage_in(ly, p.yl + row0 * L, cnt * L, L, p.Ls);
        stage_in(lq, p.pp + row0 * L, cnt * L, L, p.Ls);
        __syncthreads();
    }
    float conf_part = 0.f, loc_part = 0.f;
    int npos_conf = 0, npos_loc = 0;
    if (tid < cnt) {
        const long row = row0 + tid;
        if (p.yl) {
            const float* y = STAGED ? ly + tid * p.Ls : p.yl + row * L;
            const float* q = STAGED ? lq + tid * p.Ls : p.pp + row * L;
            bool pos;
            conf_part = focal_row(y, q, L, p.alpha, p.gamma, pos);
            npos_conf = pos ? 1 : 0;
            if (p.ce_out) p.ce_out[row] = conf_part;
            if (p.mask_out) p.mask_out[row] = 1.0f;
        }
        if (p.yd) {
            const float4 t = *reinterpret_cast<const float4*>(p.yd + row * 4);
            const float4 o = *reinterpret_cast<const float4*>(p.pd + row * 4);
            const float e[4] = {o.x - t.x, o.y - t.y, o.z - t.z, o.w - t.w};
            float h = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = fabsf(e[k]);
                const float qd = fminf(a, 1.0f);
                h += 0.5f * (qd * qd) + 1.0f * (a - qd);          // TF-2.0 huber_loss, delta = 1 (as ssd_loss_kernel)
            }
            if (t.x != 0.f || t.y != 0.f || t.z != 0.f || t.w != 0.f) {
                npos_loc = 1;
                loc_part = h;
            }
        }
    }
    FocalPartial out;
    out.conf = block_sum<kFocalWaves>(conf_part, shf);
    out.loc = block_sum<kFocalWaves>(loc_part, shf);
    out.pos_conf = block_sum_i<kFocalWaves>(npos_conf, shi);
    out.pos_loc = block_sum_i<kFocalWaves>(npos_loc, shi);
    if (tid == 0) p.part[blockIdx.x] = out;
}

template <bool STAGED>
__global__ __launch_bounds__(kFocalThreads) void focal_finish_kernel(const FocalParams p) {
    extern __shared__ float4 focal_lds[];
    __shared__ float shf[kFocalWaves];
    __shared__ int shi[kFocalWaves];
    const int tid = threadIdx.x, L = p.L;
    const bool grads = p.grad_deltas || p.grad_logits;       // without them the grid is one workgroup per image
    const int b = grads ? blockIdx.x / p.tiles : blockIdx.x, tile = grads ? blockIdx.x % p.tiles : 0;
    // the image's totals: thread i adds the partials i, i + 256, ... in tile order, then the fixed tree
    float conf_sum = 0.f, loc_sum = 0.f;
    int pos_conf = 0, pos_loc = 0;
    for (int i = tid; i < p.tiles; i += kFocalThreads) {
        const FocalPartial v = p.part[(long)b * p.tiles + i];
        conf_sum += v.conf;
        loc_sum += v.loc;
        pos_conf += v.pos_conf;
        pos_loc += v.pos_loc;
    }
    conf_sum = block_sum<kFocalWaves>(conf_sum, shf);
    loc_sum = block_sum<kFocalWaves>(loc_sum, shf);
    pos_conf = block_sum_i<kFocalWaves>(pos_conf, shi);
    pos_loc = block_sum_i<kFocalWaves>(pos_loc, shi);
    const float conf_den = pos_conf == 0 ? 1.0f : (float)pos_conf;
    const float loc_den = pos_loc == 0 ? 1.0f : (float)pos_loc;
    if (tile == 0 && tid == 0) {
        if (p.yd && p.loc_loss) p.loc_loss[b] = loc_sum / loc_den * p.loc_alpha;
        if (p.yl && p.conf_loss) p.conf_loss[b] = conf_sum / conf_den;
    }
    if (!grads) return;

    // gradients of grad_scale * (loc_loss[b] + conf_loss[b])
    const int n0 = tile * p.T, cnt = min(p.T, p.N - n0);
    const long row0 = (long)b * p.N + n0;
    if (p.grad_deltas && p.yd && tid < cnt) {
        const long row = row0 + tid;
        const float g = p.grad_scale * p.loc_alpha / loc_den;
        const float4 t = *reinterpret_cast<const float4*>(p.yd + row * 4);
        float4 r = {0.f, 0.f, 0.f, 0.f};
        if (t.x != 0.f || t.y != 0.f || t.z != 0.f || t.w != 0.f) {
            const float4 o = *reinterpret_cast<const float4*>(p.pd + row * 4);
            r.x = g * fminf(fmaxf(o.x - t.x, -1.0f), 1.0f);
            r.y = g * fminf(fmaxf(o.y - t.y, -1.0f), 1.0f);
            r.z = g * fminf(fmaxf(o.z - t.z, -1.0f), 1.0f);
            r.w = g * fminf(fmaxf(o.w - t.w, -1.0f), 1.0f);
        }
        *reinterpret_cast<float4*>(p.grad_deltas + row * 4) = r;
    }
    if (p.grad_logits && p.yl) {
        const float gce = p.grad_scale / conf_den;
        float* ly = reinterpret_cast<float*>(focal_lds);
        float* lq = ly + p.T * p.Ls;
        if (STAGED) {
            stage_in(ly, p.yl + row0 * L, cnt * L, L, p.Ls);
            stage_in(lq, p.pp + row0 * L, cnt * L, L, p.Ls);
            __syncthreads();
        }
        if (tid < cnt) {
            const long row = row0 + tid;
            const float* y = STAGED ? ly + tid * p.Ls : p.yl + row * L;
            const float* q = STAGED ? lq + tid * p.Ls : p.pp + row * L;
            float* out = STAGED ? ly + tid * p.Ls : p.grad_logits + row * L;     // staged: over the thread's own y row
            focal_row_grad<STAGED>(y, q, L, p.alpha, p.gamma, gce, out, out);
        }
        if (STAGED) {
            __syncthreads();
            stage_out(p.grad_logits + row0 * L, ly, cnt * L, L, p.Ls);
        }
    }
}

static size_t focal_workspace(int B, int N, int L) {
    const int T = focal_staged_tile(L) ? focal_staged_tile(L) : kFocalThreads;
    return align_up((size_t)B * (size_t)cdiv(N, T) * sizeof(FocalPartial), 256);
}

}  // namespace ssd

using namespace ssd;

extern "C" {

int ssd_focal_loss_tile(int L, int* staged_out) {
    if (L < 1) return 0;
    const int t = focal_staged_tile(L);
    if (staged_out) *staged_out = t ? 1 : 0;
    return t ? t : kFocalThreads;
}

size_t ssd_focal_loss_workspace_bytes(int B, int N, int L) {
    if (B < 0 || N < 0 || L < 1) return 0;
    return focal_workspace(B, N, L);
}

int ssd_focal_loss(const float* actual_deltas_dev, const float* pred_deltas_dev, const float* actual_labels_dev,
                   const float* pred_labels_dev, int B, int N, int L, float loc_loss_alpha, float focal_alpha,
                   float focal_gamma, float* loc_loss_dev, float* conf_loss_dev, float* ce_out_dev, float* mask_out_dev,
                   float* grad_deltas_dev, float* grad_logits_dev, float grad_scale, void* workspace_dev,
                   size_t workspace_bytes, void* stream) {
    SSD_CHECK_ARG(B >= 0 && N >= 1 && L >= 1, "ssd_focal_loss: bad sizes B=%d N=%d L=%d", B, N, L);
    SSD_CHECK_ARG(focal_alpha > 0.f && focal_alpha < INFINITY && focal_gamma >= 0.f && focal_gamma < INFINITY,
                  "ssd_focal_loss: alpha must be > 0 and gamma >= 0 (finite), got alpha=%g gamma=%g", (double)focal_alpha,
                  (double)focal_gamma);
    if (B == 0) return SSD_OK;
    const bool loc = actual_deltas_dev != nullptr, conf = actual_labels_dev != nullptr;
    SSD_CHECK_ARG(loc || conf, "ssd_focal_loss: neither a localisation nor a confidence target given");
    SSD_CHECK_ARG(!loc || pred_deltas_dev, "ssd_focal_loss: pred_deltas is NULL");
    SSD_CHECK_ARG(!conf || pred_labels_dev, "ssd_focal_loss: pred_labels is NULL");
    SSD_CHECK_ARG(!grad_deltas_dev || loc, "ssd_focal_loss: grad_deltas needs the localisation target");
    SSD_CHECK_ARG(!grad_logits_dev || conf, "ssd_focal_loss: grad_logits needs the confidence target");
    SSD_CHECK_ARG(workspace_dev && workspace_bytes >= focal_workspace(B, N, L),
                  "ssd_focal_loss: workspace too small (%zu < %zu bytes)", workspace_bytes, focal_workspace(B, N, L));
    SSD_CHECK_ARG((((uintptr_t)actual_deltas_dev | (uintptr_t)pred_deltas_dev | (uintptr_t)grad_deltas_dev) & 15) == 0,
                  "ssd_focal_loss: delta tensors must be 16-byte aligned");
    SSD_CHECK_ARG((((uintptr_t)actual_labels_dev | (uintptr_t)pred_labels_dev | (uintptr_t)grad_logits_dev |
                    (uintptr_t)workspace_dev) & 3) == 0,
                  "ssd_focal_loss: label tensors and the workspace must be 4-byte aligned");
    FocalParams p{};
    p.yd = actual_deltas_dev; p.pd = pred_deltas_dev; p.yl = actual_labels_dev; p.pp = pred_labels_dev;
    p.B = B; p.N = N; p.L = L;
    const int staged_tile = focal_staged_tile(L);
    const bool staged = staged_tile != 0;
    p.T = staged ? staged_tile : kFocalThreads;
    p.tiles = cdiv(N, p.T);
    p.Ls = L | 1;
    SSD_UNSUPPORTED_IF((long)B * p.tiles > 0x7fffffffL, "ssd_focal_loss: B * tiles = %ld workgroups exceed the grid limit",
                       (long)B * p.tiles);
    p.loc_alpha = loc_loss_alpha; p.alpha = focal_alpha; p.gamma = focal_gamma;
    p.loc_loss = loc_loss_dev; p.conf_loss = conf_loss_dev; p.ce_out = ce_out_dev; p.mask_out = mask_out_dev;
    p.grad_deltas = grad_deltas_dev; p.grad_logits = grad_logits_dev; p.grad_scale = grad_scale;
    p.part = (FocalPartial*)workspace_dev;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned all = (unsigned)((long)B * p.tiles);
    const size_t lds = staged && conf ? (size_t)2 * p.T * p.Ls * sizeof(float) : 0;
    const bool grads = grad_deltas_dev || grad_logits_dev;
    const size_t lds2 = grad_logits_dev ? lds : 0;
    if (staged) {
        hipLaunchKernelGGL(focal_partial_kernel<true>, dim3(all), dim3(kFocalThreads), lds, st, p);
        SSD_LAUNCH_CHECK();
        hipLaunchKernelGGL(focal_finish_kernel<true>, dim3(grads ? all : (unsigned)B), dim3(kFocalThreads), lds2, st, p);
    } else {
        hipLaunchKernelGGL(focal_partial_kernel<false>, dim3(all), dim3(kFocalThreads), 0, st, p);
        SSD_LAUNCH_CHECK();
        hipLaunchKernelGGL(focal_finish_kernel<false>, dim3(grads ? all : (unsigned)B), dim3(kFocalThreads), 0, st, p);
    }
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

}  // extern "C"
