// Training step of the SSD graphs (reference trainer.py:50-76):
// training-mode forward (BatchNorm on batch statistics, moving averages updated with Keras'
// momentum 0.999), the HIP loss (csrc/ssd_loss.hip) and backward of every layer; the optimizer
// that follows is csrc/ssd_optim.hip.
//
//   conv backward-data   = the forward MFMA implicit-GEMM kernel (conv_mfma_kernel) on dY with the
//                          180-degree-rotated, in/out-transposed weights; stride-2 3x3 convs go
//                          through a zero-inserted dY (they are the four small SSD extras);
//   conv backward-weights= wgrad_mfma_kernel below: dW[K,N] = im2col(X)^T [K,M] * dY [M,N] on
//                          v_mfma_f32_16x16x4_f32, M split over the grid, deterministic two-stage sum;
//   depthwise backward   = gather kernels (HBM-bound);
//   BatchNorm            = two-pass batch statistics and the usual two-reduction backward, all
//                          reductions deterministic (fixed chunking, fixed order).
// Gradients leave through a caller-owned flat buffer (parameter-table order), which is what the
// host all-reduces over RCCL between backward and the optimizer step.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "ssd_bf16x3.h"
#include "ssd_train.h"

using namespace ssd;

extern "C" size_t ssd_loss_workspace_bytes(int B, int N);
extern "C" int ssd_loss(const float*, const float*, const float*, const float*, int, int, int, float, float, float*,
                        float*, float*, float*, float*, float*, float, void*, size_t, void*);

namespace ssd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kBnEps = 1e-3f;          // keras-applications MobileNetV2: BatchNormalization(epsilon=1e-3, momentum=0.999)
constexpr float kBnMomentum = 0.999f;

// ------------------------------------------------------------------ small elementwise kernels
__device__ __forceinline__ float bn_z(float y, float mean, float istd, float gamma, float beta) {
    return (y - mean) * istd * gamma + beta;
}
__device__ __forceinline__ float act_fwd(float z, int act) {
    if (act == SSD_ACT_RELU) return fmaxf(z, 0.f);
    if (act == SSD_ACT_RELU6) return fminf(fmaxf(z, 0.f), 6.f);
    return z;
}
// TF ReluGrad / Relu6Grad: gradient passes strictly inside the linear range
__device__ __forceinline__ float act_mask(float z, int act) {
    if (act == SSD_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == SSD_ACT_RELU6) return (z > 0.f && z < 6.f) ? 1.f : 0.f;
    return 1.f;
}

// out = act(bn(pre)) (+ residual)
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ pre, const long M, const int C,
                                                      const float* __restrict__ mean, const float* __restrict__ istd,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const int act, const float* __restrict__ res,
                                                      float* __restrict__ out) {
    const long total = M * C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        float v = act_fwd(bn_z(pre[e], mean[c], istd[c], gamma[c], beta[c]), act);
        if (res) v += res[e];
        out[e] = v;
    }
}

// dy = gamma * istd * (dz - dbeta / M - xhat * dgamma / M),  dz = dout * act'(z)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dout, const float* __restrict__ pre,
                                                          const long M, const int C, const float* __restrict__ mean,
                                                          const float* __restrict__ istd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const int act,
                                                          const float* __restrict__ dgamma,
                                                          const float* __restrict__ dbeta, float* __restrict__ dy) {
    const long total = M * C;
    const float invM = 1.0f / (float)M;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        const float xh = (pre[e] - mean[c]) * istd[c];
        const float z = xh * gamma[c] + beta[c];
        const float dz = dout[e] * act_mask(z, act);
        dy[e] = gamma[c] * istd[c] * (dz - dbeta[c] * invM - xh * dgamma[c] * invM);
    }
}

// dz = dout * (out > 0)   (bias + ReLU layers)
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                     const long total, const int act, float* __restrict__ dz) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        dz[e] = dout[e] * act_mask(out[e], act);
}

// Backward through a FROZEN BatchNorm (Keras trainable = False: it normalises with the moving statistics, which are
// constants of the step): bn_bwd_apply_kernel's formula without the two batch-mean terms,
//   dy = gamma * istd_moving * dout * act'(z) = dout * act'(out) * scale[c],   scale = gamma / sqrt(moving_var + eps)
// (the folded scale of the forward).  The pass-mask comes from the stored OUTPUT: act(z) lies strictly inside the linear
// range exactly where z does; a layer with a residual add has no activation (the host checks), so `out` is then not read.
// Bandwidth-bound: 16-byte accesses (C % 4 == 0, 16-byte aligned tensors), the scalar form for anything else.
__global__ __launch_bounds__(256) void bn_frozen_bwd4_kernel(const f32x4* __restrict__ dout, const f32x4* __restrict__ out,
                                                            const f32x4* __restrict__ scale, const long total4, const int C4,
                                                            const int act, f32x4* __restrict__ dy) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
        f32x4 g = dout[e] * scale[(int)(e % C4)];
        if (act) {
            const f32x4 o = out[e];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] *= act_mask(o[j], act);
        }
        dy[e] = g;
    }
}
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                           const float* __restrict__ scale, const long total, const int C,
                                                           const int act, float* __restrict__ dy) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        dy[e] = dout[e] * scale[(int)(e % C)] * (act ? act_mask(out[e], act) : 1.f);
}

// Every frozen BatchNorm of the net folded into its per-channel scale / shift as ONE launch (blockIdx.y = job), the
// arithmetic of fold_bn_kernel (csrc/ssd_ops.hip): the conv epilogue of the training forward then writes
// act(scale * conv + shift) (+ residual) directly
struct FoldJob {
    const float *gamma, *beta, *mean, *var;
    float *scale, *shift;
    int C;
};
__global__ __launch_bounds__(256) void bn_fold_jobs_kernel(const FoldJob* __restrict__ jobs, const float eps) {
    const FoldJob j = jobs[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= j.C) return;
    const float inv = j.gamma[c] / sqrtf(j.var[c] + eps);
    j.scale[c] = inv;
    j.shift[c] = j.beta[c] - j.mean[c] * inv;
}

// dst (+)= src
__global__ __launch_bounds__(256) void add_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                 const long total, const int accumulate) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        dst[e] = accumulate ? dst[e] + src[e] : src[e];
}

// Keras moving average: var -= (var - value) * (1 - momentum)
// (the fused BatchNorm op hands Keras the Bessel-corrected batch variance, var * M / (M - 1), and Keras'
// BatchNormalization keeps it for the moving average -- `_bessels_correction_test_only` -- while the
// normalisation and the backward use the biased one)
__global__ void moving_update_kernel(float* mm, float* mv, const float* mean, const float* var, const int C,
                                     const float one_minus_momentum, const float bessel) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        mm[c] -= (mm[c] - mean[c]) * one_minus_momentum;
        mv[c] -= (mv[c] - var[c] * bessel) * one_minus_momentum;
    }
}

// Wt[ky'][kx'][co_off + co][ci] = W[kh-1-ky'][kw-1-kx'][ci][co]   (HWIO -> rotated, transposed HWIO
// with I = CoPad, O = Ci; rows co >= Co stay zero: the caller memsets Wt)
__global__ __launch_bounds__(256) void rot_transpose_kernel(const float* __restrict__ w, const int kh, const int kw,
                                                           const int Ci, const int Co, const int CoPad,
                                                           const int co_off, float* __restrict__ wt) {
    const long total = (long)kh * kw * Ci * Co;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int co = (int)(e % Co);
        long r = e / Co;
        const int ci = (int)(r % Ci);
        r /= Ci;
        const int kx = (int)(r % kw), ky = (int)(r / kw);
        wt[((long)((kh - 1 - ky) * kw + (kw - 1 - kx)) * CoPad + co_off + co) * Ci + ci] = w[e];
    }
}

// Every weight re-pack of a training step as ONE launch (the weights change every step; 103 forward
// packs + 54 rotate/transposes + 50 backward packs were 0.75 ms of 5 us launches): blockIdx.y = job.
//   mode 0  forward:        dst[n][k] = W[k][n]                          ([Npad][Kpad], zero padded;
//           a head conv's label (w, Cout1 columns) and box (w2) kernels are stacked along n)
//   mode 1  backward-data:  dst[ci][(ky', kx', co')] = W[kh-1-ky'][kw-1-kx'][ci][co']   (rotated and
//           transposed: the forward conv kernel then computes dX from dY; co' < CoPad, zero padded)
struct PackJob {
    const float* w;
    const float* w2;
    float* dst;
    int mode, K, Cout, Cout1, Kpad, Npad, kh, kw, Ci, CoPad;
    int bf16;       // the net's precision: 0 -> the planes h, m, l (split-bf16 tiles) are written, 1 -> only the rounding r (bf16 tiles)
};
__global__ __launch_bounds__(256) void pack_jobs_kernel(const PackJob* __restrict__ jobs) {
    const PackJob j = jobs[blockIdx.y];
    const int total = j.Npad * j.Kpad;            // < 2^31 (ssd_net_train_begin checks): 32-bit index arithmetic
    const int C2 = j.Cout - j.Cout1;
    // the jobs differ by three orders of magnitude (a 16 x 32 pointwise kernel .. head level 2's 160 x 11 520): every job gets
    // gridDim.x blocks, the small ones leave at once (16 blocks per job took 309 us of a 10.8 ms step)
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int n = e / j.Kpad, k = e - n * j.Kpad;
        float v = 0.f;
        if (j.mode == 0) {
            if (n < j.Cout && k < j.K) v = n < j.Cout1 ? j.w[(long)k * j.Cout1 + n] : j.w2[(long)k * C2 + (n - j.Cout1)];
        } else if (n < j.Ci && k < j.kh * j.kw * j.CoPad) {
            const int co = k % j.CoPad, tap = k / j.CoPad;
            if (co < j.Cout) {
                const int ky = j.kh - 1 - tap / j.kw, kx = j.kw - 1 - tap % j.kw;
                const long row = (long)(ky * j.kw + kx) * j.Ci + n;
                v = co < j.Cout1 ? j.w[row * j.Cout1 + co] : j.w2[row * C2 + (co - j.Cout1)];
            }
        }
        j.dst[e] = v;
        // the same matrix as four bf16 planes behind the fp32 one: the exact split h, m, l (split-bf16 conv tiles,
        // ssd_conv3.hip) and the bf16 rounding r (bf16 tiles)
        // (only the planes this precision's tiles read: the re-pack runs every step)
        short* pl = reinterpret_cast<short*>(j.dst + total);
        const long d = plane_elem(n, k, j.Npad);          // planes: [Kpad / 32][Npad][32] (ssd_bf16x3.h)
        if (j.bf16) {
            pl[3 * (long)total + d] = rne1(v);
        } else {
            short h, m, l;
            split1(v, h, m, l);
            pl[d] = h;
            pl[(long)total + d] = m;
            pl[2 * (long)total + d] = l;
        }
    }
}

// dense[b][p][c] (row stride ld) = src[b * bs + off + p * ps + c]   (one head level out of the
// concatenated [B,N,K] gradient buffer); col0 = first dense column written
__global__ __launch_bounds__(256) void gather_head_kernel(const float* __restrict__ src, const long bs, const long off,
                                                         const long ps, const int B, const int P, const int C,
                                                         float* __restrict__ dense, const int ld, const int col0) {
    const long total = (long)B * P * C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        const long r = e / C;
        const int p = (int)(r % P), b = (int)(r / P);
        dense[r * ld + col0 + c] = src[b * bs + off + (long)p * ps + c];
    }
}

// z[b][2*oy][2*ox][c] = y[b][oy][ox][c], zero elsewhere (the caller memsets z)
__global__ __launch_bounds__(256) void dilate2_kernel(const float* __restrict__ y, const int B, const int Ho, const int Wo,
                                                     const int C, const int Hz, const int Wz, float* __restrict__ z) {
    const long total = (long)B * Ho * Wo * C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C);
        long r = e / C;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho), b = (int)(r / Ho);
        z[(((long)b * Hz + 2 * oy) * Wz + 2 * ox) * C + c] = y[e];
    }
}

// ------------------------------------------------------------------ column reductions over [M][C]
// block = 64 columns x 4 row lanes; grid = (ceil(C/64), chunks); partial[chunk][2][C].
enum { RED_SUM = 0, RED_SQDEV = 1, RED_BN_BWD = 2, RED_ACT_BWD = 3, RED_STATS = 4 };
struct RedParams {
    const float* a;       // SUM/SQDEV: x;  BN_BWD / ACT_BWD: dout
    const float* b;       // BN_BWD: pre;   ACT_BWD: out (nullable: no activation)
    const float *mean, *istd, *gamma, *beta;
    long M;
    int C, lda, act, cw;
    long rows_per_chunk;
    float* partial;
};
template <int OP>
__global__ __launch_bounds__(256) void col_reduce_kernel(const RedParams p) {
    // block = CW columns x (256 / CW) row lanes; CW in {16, 32, 64} chosen on the host so that
    // narrow tensors (C = 16 .. 32) keep every lane busy
    __shared__ float sh[2][256];
    const int CW = p.cw, RL = 256 / CW;
    const int cl = threadIdx.x % CW, rl = threadIdx.x / CW;
    const int c = blockIdx.x * CW + cl;
    const long r0 = (long)blockIdx.y * p.rows_per_chunk;
    const long r1 = r0 + p.rows_per_chunk < p.M ? r0 + p.rows_per_chunk : p.M;
    float s1 = 0.f, s2 = 0.f;
    if (c < p.C) {
        float mean = 0.f, istd = 0.f, gamma = 0.f, beta = 0.f;
        if (OP == RED_SQDEV || OP == RED_BN_BWD) mean = p.mean[c];
        if (OP == RED_BN_BWD) { istd = p.istd[c]; gamma = p.gamma[c]; beta = p.beta[c]; }
        for (long r = r0 + rl; r < r1; r += RL) {
            const float a = p.a[r * p.lda + c];
            if (OP == RED_SUM) s1 += a;
            else if (OP == RED_SQDEV) { const float d = a - mean; s1 += d * d; }
            else if (OP == RED_BN_BWD) {
                const float xh = (p.b[r * p.C + c] - mean) * istd;
                const float dz = a * act_mask(xh * gamma + beta, p.act);
                s1 += dz;
                s2 += dz * xh;
            } else {
                s1 += p.b ? a * act_mask(p.b[r * p.C + c], p.act) : a;
            }
        }
    }
    sh[0][threadIdx.x] = s1;
    sh[1][threadIdx.x] = s2;
    __syncthreads();
    if (rl == 0 && c < p.C) {
        float t1 = 0.f, t2 = 0.f;
        for (int k = 0; k < RL; ++k) {           // fixed order: deterministic
            t1 += sh[0][k * CW + cl];
            t2 += sh[1][k * CW + cl];
        }
        const long o = (long)blockIdx.y * 2 * p.C;
        p.partial[o + c] = t1;
        p.partial[o + p.C + c] = t2;
    }
}

// 16-byte form of col_reduce_kernel for C % 4 == 0 (every tensor of both graphs): thread = 4
// consecutive channels; block = CQ channel quads x (256 / CQ) row lanes.  RED_STATS: one pass for
// the batch statistics -- sums of (x - K) and (x - K)^2 with a per-column shift K common to every chunk.
// K = mean of four samples of the column from the interior of the tensor (rows (2j + 1) M / 8): (mean - K)^2 is
// ~ var / 4, so s2/M - (s1/M)^2 cancels at most a fraction of var.  (A single sample is not enough: K = x[0][c], a
// zero-padded corner pixel, lay up to several sigma off the mean and cost the variance ~80 u sum (|x| + |mean|)^2 / M.)
// Every thread of every chunk and col_finalize_kernel form K with the same expression: bit-identical.
typedef float tf32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ long stats_shift_row(const long M, const int j) { return (2 * j + 1) * M / 8; }
template <int OP>
__global__ __launch_bounds__(256) void col_reduce4_kernel(const RedParams p) {
    __shared__ tf32x4 sh[2][256];
    const int CQ = p.cw, RL = 256 / CQ;
    const int cl = threadIdx.x % CQ, rl = threadIdx.x / CQ;
    const int c = (blockIdx.x * CQ + cl) * 4;
    const long r0 = (long)blockIdx.y * p.rows_per_chunk;
    const long r1 = r0 + p.rows_per_chunk < p.M ? r0 + p.rows_per_chunk : p.M;
    tf32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (c < p.C) {
        tf32x4 mean = s1, istd = s1, gamma = s1, beta = s1;
        if (OP == RED_SQDEV || OP == RED_BN_BWD) mean = *reinterpret_cast<const tf32x4*>(p.mean + c);
        if (OP == RED_STATS) {                                                          // the shift K
            const tf32x4 k0 = *reinterpret_cast<const tf32x4*>(p.a + stats_shift_row(p.M, 0) * p.lda + c);
            const tf32x4 k1 = *reinterpret_cast<const tf32x4*>(p.a + stats_shift_row(p.M, 1) * p.lda + c);
            const tf32x4 k2 = *reinterpret_cast<const tf32x4*>(p.a + stats_shift_row(p.M, 2) * p.lda + c);
            const tf32x4 k3 = *reinterpret_cast<const tf32x4*>(p.a + stats_shift_row(p.M, 3) * p.lda + c);
            mean = ((k0 + k1) + (k2 + k3)) * 0.25f;
        }
        if (OP == RED_BN_BWD) {
            istd = *reinterpret_cast<const tf32x4*>(p.istd + c);
            gamma = *reinterpret_cast<const tf32x4*>(p.gamma + c);
            beta = *reinterpret_cast<const tf32x4*>(p.beta + c);
        }
#pragma unroll 4
        for (long r = r0 + rl; r < r1; r += RL) {
            const tf32x4 a = *reinterpret_cast<const tf32x4*>(p.a + r * p.lda + c);
            if (OP == RED_SUM) s1 += a;
            else if (OP == RED_SQDEV) { const tf32x4 d = a - mean; s1 += d * d; }
            else if (OP == RED_STATS) { const tf32x4 d = a - mean; s1 += d; s2 += d * d; }
            else if (OP == RED_BN_BWD) {
                const tf32x4 xh = (*reinterpret_cast<const tf32x4*>(p.b + r * p.C + c) - mean) * istd;
                const tf32x4 z = xh * gamma + beta;
                tf32x4 dz;
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[j] = a[j] * act_mask(z[j], p.act);
                s1 += dz;
                s2 += dz * xh;
            } else {
                if (p.b) {
                    const tf32x4 o = *reinterpret_cast<const tf32x4*>(p.b + r * p.C + c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s1[j] += a[j] * act_mask(o[j], p.act);
                } else {
                    s1 += a;
                }
            }
        }
    }
    sh[0][threadIdx.x] = s1;
    sh[1][threadIdx.x] = s2;
    __syncthreads();
    if (rl == 0 && c < p.C) {
        tf32x4 t1 = {0.f, 0.f, 0.f, 0.f}, t2 = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < RL; ++k) {           // fixed order: deterministic
            t1 += sh[0][k * CQ + cl];
            t2 += sh[1][k * CQ + cl];
        }
        const long o = (long)blockIdx.y * 2 * p.C;
        *reinterpret_cast<tf32x4*>(p.partial + o + c) = t1;
        *reinterpret_cast<tf32x4*>(p.partial + o + p.C + c) = t2;
    }
}
// out1[c] = scale * sum_chunks partial[.][0][c]; out2 likewise (nullable); mode 1: out2 = rsqrt(out1 + eps);
// mode 2 (batch statistics from RED_STATS partials of the [shift_M][C] tensor `shift`): out1 = mean, out2 = biased variance,
// out3 = rsqrt(var + eps), and the Keras moving averages mm / mv move towards them
__global__ __launch_bounds__(256) void col_finalize_kernel(const float* __restrict__ partial, const int chunks, const int C,
                                                          const float scale, float* out1, float* out2, const int mode,
                                                          const float eps, const float* shift = nullptr, float* out3 = nullptr,
                                                          float* mm = nullptr, float* mv = nullptr,
                                                          const float one_minus_momentum = 0.f, const float bessel = 1.f,
                                                          const long shift_M = 0) {
    // block = 16 columns x 16 chunk lanes (lane k sums chunks k, k+16, ... in order; the 16 lane
    // sums are combined in a fixed order: deterministic).  The data is tiny; the kernel is latency
    // bound, hence many short dependent chains instead of few long ones.
    __shared__ float sh[2][16][16];
    const int cl = threadIdx.x & 15, kl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    float s1 = 0.f, s2 = 0.f;
    // eight chunks' loads in flight per lane before the (in-order) adds: the loop is a chain of L2 round trips otherwise
    // (256 chunks = 16 trips of ~0.4 us: 6.9 us per launch, 118 launches per MobileNetV2 step)
    if (c < C)
        for (int k0 = kl; k0 < chunks; k0 += 128) {
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + 16 * u;
                const bool ok = k < chunks;
                const long o = (long)(ok ? k : 0) * 2 * C + c;
                a[u] = partial[o];
                b[u] = partial[o + C];
                if (!ok) a[u] = b[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s1 += a[u];
                s2 += b[u];
            }
        }
    sh[0][kl][cl] = s1;
    sh[1][kl][cl] = s2;
    __syncthreads();
    if (kl != 0 || c >= C) return;
    s1 = s2 = 0.f;
    for (int k = 0; k < 16; ++k) {
        s1 += sh[0][k][cl];
        s2 += sh[1][k][cl];
    }
    s1 *= scale;
    s2 *= scale;
    if (mode == 2) {
        const float K = ((shift[stats_shift_row(shift_M, 0) * C + c] + shift[stats_shift_row(shift_M, 1) * C + c]) +
                         (shift[stats_shift_row(shift_M, 2) * C + c] + shift[stats_shift_row(shift_M, 3) * C + c])) * 0.25f;
        const float mean = K + s1;
        const float var = fmaxf(s2 - s1 * s1, 0.0f);
        out1[c] = mean;
        out2[c] = var;
        out3[c] = 1.0f / sqrtf(var + eps);
        mm[c] -= (mm[c] - mean) * one_minus_momentum;       // Keras moving average: v -= (v - value) * (1 - momentum)
        mv[c] -= (mv[c] - var * bessel) * one_minus_momentum;   // Bessel-corrected value, see moving_update_kernel
        return;
    }
    if (out1) out1[c] = s1;
    if (mode == 1) out2[c] = 1.0f / sqrtf(s1 + eps);
    else if (out2) out2[c] = s2;
}
// out[i] = sum_chunks partial[chunk][i]: block = 64 elements x 4 chunk lanes (lane k sums chunks
// k, k+4, ... in order, then the 4 lane sums in a fixed order: deterministic)
__global__ __launch_bounds__(256) void chunk_sum_kernel(const float* __restrict__ partial, const int chunks,
                                                       const long n, float* __restrict__ out) {
    __shared__ float sh[4][64];
    const int el = threadIdx.x & 63, kl = threadIdx.x >> 6;
    for (long e0 = (long)blockIdx.x * 64; e0 < n; e0 += (long)gridDim.x * 64) {
        const long e = e0 + el;
        float s = 0.f;
        if (e < n)
            for (int k = kl; k < chunks; k += 4) s += partial[(long)k * n + e];
        __syncthreads();
        sh[kl][el] = s;
        __syncthreads();
        if (kl == 0 && e < n) out[e] = (sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el]);
    }
}

// 16-byte form for n % 4 == 0: block = EQ element quads x (256 / EQ) chunk lanes (lane k sums chunks
// k, k + KL, ... in order, then the KL lane sums in a fixed order: deterministic).  Small outputs
// (a 96 x 24 pointwise kernel summed over 1024 M-chunks) get EQ = 4: 16 elements per block, 64
// chunk lanes -- the 64-element / 4-lane form left such layers with 36 blocks walking 256 chunks each.
template <int EQ>
__global__ __launch_bounds__(256) void chunk_sum4_kernel(const float* __restrict__ partial, const int chunks,
                                                        const long n, float* __restrict__ out, const int aligned_out) {
    constexpr int KL = 256 / EQ;
    __shared__ tf32x4 sh[KL][EQ];
    const int el = threadIdx.x % EQ, kl = threadIdx.x / EQ;
    const long e = ((long)blockIdx.x * EQ + el) * 4;
    tf32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (e < n)
        for (int k0 = kl; k0 < chunks; k0 += 8 * KL) {          // eight loads in flight, added in chunk order
            tf32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + u * KL;
                v[u] = *reinterpret_cast<const tf32x4*>(partial + (long)(k < chunks ? k : 0) * n + e);
                if (k >= chunks) v[u] = tf32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
    sh[kl][el] = acc;
    __syncthreads();
    if (kl != 0 || e >= n) return;
    tf32x4 t = sh[0][el];
    for (int k = 1; k < KL; ++k) t += sh[k][el];
    if (aligned_out) *reinterpret_cast<tf32x4*>(out + e) = t;
    else
        for (int j = 0; j < 4; ++j) out[e + j] = t[j];
}
static int chunk_sum(const float* partial, long chunks, long n, float* out, hipStream_t st) {
    if (n % 4 == 0 && ((uintptr_t)partial & 15) == 0) {
        const int aligned = ((uintptr_t)out & 15) == 0;
        if (n < 65536) hipLaunchKernelGGL(chunk_sum4_kernel<4>, dim3((unsigned)((n / 4 + 3) / 4)), dim3(256), 0, st, partial, (int)chunks, n, out, aligned);
        else hipLaunchKernelGGL(chunk_sum4_kernel<16>, dim3((unsigned)((n / 4 + 15) / 16)), dim3(256), 0, st, partial, (int)chunks, n, out, aligned);
    } else {
        const long b = (n * 4 + 255) / 256;
        hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b))), dim3(256), 0, st, partial,
                           (int)chunks, n, out);
    }
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

// ------------------------------------------------------------------ conv backward-weights (MFMA)
// dW[k = (tap, ci)][n] = sum_m X[pixel(m, tap)][ci] * G[m][n].  One workgroup = a 64 (ci) x 64 (n)
// tile of one tap over one M chunk; both operands are staged row-major ([m][channel], exactly as
// they lie in HBM: coalesced 16-byte loads) into LDS with an 80-float row stride, so that the
// MFMA fragments -- A[i][kk] = X[m0+kk][c0+i], B[kk][j] = G[m0+kk][n0+j], kk = lane/16 -- are
// conflict-free ds_read_b32 (bank = 16*kk + lane%16).
constexpr int WG_BM = 32;
struct WgradParams {
    const float* x;
    const float* g;
    float* partial;       // [chunks][K][N]
    int B, H, W, Cin, Ho, Wo, kh, kw, stride, dil, pad_t, pad_l;
    int N, ldg, K;
    long M, rows_per_chunk;
    int ctiles, ntiles;   // channel tiles per tap, n tiles
    int vec_x, vec_g;
    int im2col;           // 1 (Cin % 4 != 0: the RGB stems): a tile's rows are k = (tap, ci) jointly, one "tap"
};
// Tile shape = (WC x WN wave grid) x (TI x TJ 16x16 MFMA tiles per wave): TC = 16*TI*WC input channels by
// TN = 16*TJ*WN output channels.  MobileNetV2 has many 16-32 channel sides (a 16 -> 96 expand fills 19 %
// of a 64 x 64 tile), so the host picks per layer the shape with the least padded area.
template <int WC, int WN_, int TI, int TJ>
__global__ __launch_bounds__(256) void wgrad_mfma_kernel(const WgradParams p) {
    static_assert(WC * WN_ == 4, "4 waves");
    constexpr int TC = 16 * TI * WC, TN = 16 * TJ * WN_;
    // row strides = 16 (mod 64) floats: the four 16-lane groups of a fragment read (rows 4s + kk) hit
    // disjoint bank quarters
    constexpr int LDX = (TC + 63) / 64 * 64 + 16, LDG = (TN + 63) / 64 * 64 + 16;
    constexpr int XQ = TC / 4, GQ = TN / 4;                // float4 per row
    constexpr int XU = WG_BM * XQ, GU = WG_BM * GQ;        // float4 units per slab
    __shared__ __attribute__((aligned(16))) float Xs[WG_BM * LDX];
    __shared__ __attribute__((aligned(16))) float Gs[WG_BM * LDG];
    int t = blockIdx.x;
    const int nt = t % p.ntiles;
    t /= p.ntiles;
    const int ct = t % p.ctiles, tap = t / p.ctiles;           // im2col: tap == 0
    const int ky = tap / p.kw, kx = tap % p.kw;
    const int c0 = ct * TC, n0 = nt * TN;
    const int climit = p.im2col ? p.K : p.Cin;                  // valid rows of the tile
    const long mBeg = (long)blockIdx.y * p.rows_per_chunk;
    const long mEnd = mBeg + p.rows_per_chunk < p.M ? mBeg + p.rows_per_chunk : p.M;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wk = wv / WN_, wn = wv % WN_;
    f32x4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long m0 = mBeg; m0 < mEnd; m0 += WG_BM) {
        __syncthreads();
#pragma unroll
        for (int u0 = 0; u0 < XU; u0 += 256) {
            const int u = u0 + tid;
            if (XU % 256 != 0 && u >= XU) break;
            const int row = u / XQ, q = (u - row * XQ) * 4;
            const long m = m0 + row;
            f32x4 xv = {0.f, 0.f, 0.f, 0.f};
            if (m < mEnd && p.im2col) {
                // K = kh*kw*Cin is small (27 for the RGB stems): the tile row index IS k = tap * Cin + ci
                const int ox = (int)(m % p.Wo);
                const long r = m / p.Wo;
                const int oy = (int)(r % p.Ho), b = (int)(r / p.Ho);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = c0 + q + j;
                    if (k >= p.K) continue;
                    const int tp = k / p.Cin, ci = k - tp * p.Cin;
                    const int iy = oy * p.stride - p.pad_t + (tp / p.kw) * p.dil, ix = ox * p.stride - p.pad_l + (tp % p.kw) * p.dil;
                    if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
                        xv[j] = p.x[(((long)b * p.H + iy) * p.W + ix) * p.Cin + ci];
                }
            } else if (m < mEnd) {
                const int ox = (int)(m % p.Wo);
                const long r = m / p.Wo;
                const int oy = (int)(r % p.Ho), b = (int)(r / p.Ho);
                const int iy = oy * p.stride - p.pad_t + ky * p.dil, ix = ox * p.stride - p.pad_l + kx * p.dil;
                if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                    const float* xp = p.x + (((long)b * p.H + iy) * p.W + ix) * p.Cin + c0 + q;
                    if (p.vec_x && c0 + q + 3 < p.Cin) xv = *reinterpret_cast<const f32x4*>(xp);
                    else
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (c0 + q + j < p.Cin) xv[j] = xp[j];
                }
            }
            *reinterpret_cast<f32x4*>(&Xs[row * LDX + q]) = xv;
        }
#pragma unroll
        for (int u0 = 0; u0 < GU; u0 += 256) {
            const int u = u0 + tid;
            if (GU % 256 != 0 && u >= GU) break;
            const int row = u / GQ, q = (u - row * GQ) * 4;
            const long m = m0 + row;
            f32x4 gv = {0.f, 0.f, 0.f, 0.f};
            if (m < mEnd) {
                const float* gp = p.g + m * p.ldg + n0 + q;
                if (p.vec_g && n0 + q + 3 < p.N) gv = *reinterpret_cast<const f32x4*>(gp);
                else
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (n0 + q + j < p.N) gv[j] = gp[j];
            }
            *reinterpret_cast<f32x4*>(&Gs[row * LDG + q]) = gv;
        }
        __syncthreads();
        const int kk = lane >> 4, li = lane & 15;
#pragma unroll
        for (int s = 0; s < WG_BM / 4; ++s) {
            const int r = 4 * s + kk;
            float av[TI], bv[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) av[i] = Xs[r * LDX + (wk * TI + i) * 16 + li];
#pragma unroll
            for (int j = 0; j < TJ; ++j) bv[j] = Gs[r * LDG + (wn * TJ + j) * 16 + li];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // lane owns D[i = 4*(lane/16) + r][j = lane%16] of each 16x16 tile
    float* out = p.partial + (long)blockIdx.y * p.K * p.N;
    const int li = lane & 15, lr = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int n = n0 + (wn * TJ + j) * 16 + li;
            if (n >= p.N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = c0 + (wk * TI + i) * 16 + lr + r;
                if (ci < climit) out[((long)tap * p.Cin + ci) * p.N + n] = acc[i][j][r];
            }
        }
}
typedef void (*wgrad_kernel_t)(const WgradParams);
struct WgradCfg {
    int tc, tn;
    wgrad_kernel_t fn;
};
#define WGCFG(WC, WN_, TI, TJ) {16 * TI * WC, 16 * TJ * WN_, wgrad_mfma_kernel<WC, WN_, TI, TJ>}
static const WgradCfg kWgrad[] = {
    WGCFG(2, 2, 2, 2),      // 64 x 64
    WGCFG(1, 4, 1, 2),      // 16 x 128
    WGCFG(1, 4, 2, 2),      // 32 x 128
    WGCFG(1, 4, 1, 1),      // 16 x 64
    WGCFG(2, 2, 1, 2),      // 32 x 64
    WGCFG(4, 1, 2, 1),      // 128 x 16
    WGCFG(4, 1, 2, 2),      // 128 x 32
    WGCFG(2, 2, 2, 1),      // 64 x 32
    WGCFG(4, 1, 1, 1),      // 64 x 16
    WGCFG(2, 2, 4, 4),      // 128 x 128
    WGCFG(2, 2, 4, 2),      // 128 x 64
    WGCFG(2, 2, 2, 4),      // 64 x 128
};

// ------------------------------------------------------------------ depthwise 3x3 backward
struct DwBwdParams {
    const float* x;       // [B,H,W,C] forward input
    const float* g;       // [B,Ho,Wo,C] dY
    const float* w;       // [9][C]
    float* dx;            // [B,H,W,C]
    float* partial;       // [chunks][9][C]
    int B, H, W, C, Ho, Wo, stride, pad_t, pad_l, accumulate;
    long M, rows_per_chunk;
};
// dW[tap][c] partial sums: block = 16 channel quads (64 channels, 16-byte loads) x 16 row lanes,
// grid (ceil(C/64), chunks)
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const DwBwdParams p) {
    __shared__ __attribute__((aligned(16))) float sh[16][64];
    const int ql = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + ql * 4;
    const long r0 = (long)blockIdx.y * p.rows_per_chunk;
    const long r1 = r0 + p.rows_per_chunk < p.M ? r0 + p.rows_per_chunk : p.M;
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < p.C) {
        // row lane rl walks a CONTIGUOUS run of output pixels with a sliding 3x3 window of x in registers:
        // along a row each step loads one new column (stride 1) or two (stride 2) instead of nine taps
        const long seg = (r1 - r0 + 15) / 16;
        const long mb = r0 + rl * seg, me = mb + seg < r1 ? mb + seg : r1;
        f32x4 xw[3][3];
        int pox = -2, poy = -1, pb = -1;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (long m = mb; m < me; ++m) {
            const int ox = (int)(m % p.Wo);
            const long r = m / p.Wo;
            const int oy = (int)(r % p.Ho), b = (int)(r / p.Ho);
            const f32x4 g = *reinterpret_cast<const f32x4*>(p.g + m * p.C + c);
            const bool slide = ox == pox + 1 && oy == poy && b == pb;
            const int first = slide ? 3 - p.stride : 0;            // first window column to (re)load
            if (slide) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    if (p.stride == 1) { xw[ky][0] = xw[ky][1]; xw[ky][1] = xw[ky][2]; }
                    else xw[ky][0] = xw[ky][2];
                }
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = oy * p.stride - p.pad_t + ky;
                const bool rowok = (unsigned)iy < (unsigned)p.H;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if (kx < first) continue;
                    const int ix = ox * p.stride - p.pad_l + kx;
                    xw[ky][kx] = (rowok && (unsigned)ix < (unsigned)p.W)
                                     ? *reinterpret_cast<const f32x4*>(p.x + (((long)b * p.H + iy) * p.W + ix) * p.C + c)
                                     : zero;
                }
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx] += xw[ky][kx] * g;
            pox = ox; poy = oy; pb = b;
        }
    }
    float* out = p.partial + (long)blockIdx.y * 9 * p.C;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
        *reinterpret_cast<f32x4*>(&sh[rl][ql * 4]) = acc[t];
        __syncthreads();
        if (threadIdx.x < 64 && blockIdx.x * 64 + (int)threadIdx.x < p.C) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) v += sh[k][threadIdx.x];       // fixed order: deterministic
            out[t * p.C + blockIdx.x * 64 + threadIdx.x] = v;
        }
    }
}
// dX[b][iy][ix][c] = sum_taps dY[b][(iy + pt - ky)/s][(ix + pl - kx)/s][c] * w[ky][kx][c]
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const DwBwdParams p) {
    const int C4 = p.C >> 2;
    const long total = (long)p.B * p.H * p.W * C4;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C4) * 4;
        long r = e / C4;
        const int ix = (int)(r % p.W);
        r /= p.W;
        const int iy = (int)(r % p.H), b = (int)(r / p.H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = iy + p.pad_t - ky;
            if (ty < 0 || ty % p.stride) continue;
            const int oy = ty / p.stride;
            if (oy >= p.Ho) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = ix + p.pad_l - kx;
                if (tx < 0 || tx % p.stride) continue;
                const int ox = tx / p.stride;
                if (ox >= p.Wo) continue;
                const f32x4 g = *reinterpret_cast<const f32x4*>(p.g + (((long)b * p.Ho + oy) * p.Wo + ox) * p.C + c);
                const f32x4 w = *reinterpret_cast<const f32x4*>(p.w + (ky * 3 + kx) * p.C + c);
                acc += g * w;
            }
        }
        f32x4* d = reinterpret_cast<f32x4*>(p.dx + (((long)b * p.H + iy) * p.W + ix) * p.C + c);
        *d = p.accumulate ? *d + acc : acc;
    }
}

// stride-1 form (13 of the 17 depthwise layers): thread = 4 consecutive ix x 4 channels; the 3 x 6 window
// of dY serves all four outputs (4.5 loads per output instead of 9)
__global__ __launch_bounds__(256) void dw_dgrad4_kernel(const DwBwdParams p) {
    const int C4 = p.C >> 2, W4 = (p.W + 3) >> 2;
    const long total = (long)p.B * p.H * W4 * C4;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % C4) * 4;
        long r = e / C4;
        const int ix0 = (int)(r % W4) * 4;
        r /= W4;
        const int iy = (int)(r % p.H), b = (int)(r / p.H);
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int oy = iy + p.pad_t - ky;
            if ((unsigned)oy >= (unsigned)p.Ho) continue;
            f32x4 g[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int ox = ix0 + p.pad_l - 2 + q;            // = (ix0 + j) + pad_l - kx  for  q = j + 2 - kx
                g[q] = (unsigned)ox < (unsigned)p.Wo ? *reinterpret_cast<const f32x4*>(p.g + (((long)b * p.Ho + oy) * p.Wo + ox) * p.C + c)
                                                     : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(p.w + (ky * 3 + kx) * p.C + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += g[j + 2 - kx] * w;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ix0 + j >= p.W) break;
            f32x4* d = reinterpret_cast<f32x4*>(p.dx + (((long)b * p.H + iy) * p.W + ix0 + j) * p.C + c);
            *d = p.accumulate ? *d + acc[j] : acc[j];
        }
    }
}

// ------------------------------------------------------------------ max pool / L2 normalisation backward
// MaxPool2D backward, gather form (deterministic, also for the overlapping 3x3 stride-1 pool5): an
// input element receives dY of every window whose FIRST maximum (row-major scan over the valid
// cells -- TF ignores padded cells) it is.
struct PoolBwdParams {
    const float* x;      // [B,H,W,C] forward input
    const float* g;      // [B,Ho,Wo,C]
    float* dx;
    int B, H, W, C, Ho, Wo, k, stride, pad_t, pad_l, accumulate;
};
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const PoolBwdParams p) {
    const long total = (long)p.B * p.H * p.W * p.C;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int c = (int)(e % p.C);
        long r = e / p.C;
        const int ix = (int)(r % p.W);
        r /= p.W;
        const int iy = (int)(r % p.H), b = (int)(r / p.H);
        const float* xb = p.x + (long)b * p.H * p.W * p.C + c;
        float acc = 0.f;
        // windows containing (iy, ix): oy*s - pt <= iy <= oy*s - pt + k - 1
        const int oy_lo = max(0, (iy + p.pad_t - p.k + 1 + p.stride - 1) / p.stride);
        const int ox_lo = max(0, (ix + p.pad_l - p.k + 1 + p.stride - 1) / p.stride);
        for (int oy = oy_lo; oy < p.Ho && oy * p.stride - p.pad_t <= iy; ++oy)
            for (int ox = ox_lo; ox < p.Wo && ox * p.stride - p.pad_l <= ix; ++ox) {
                float best = -INFINITY;
                int by = -1, bx = -1;
                for (int ky = 0; ky < p.k; ++ky) {
                    const int y = oy * p.stride - p.pad_t + ky;
                    if ((unsigned)y >= (unsigned)p.H) continue;
                    for (int kx = 0; kx < p.k; ++kx) {
                        const int xx = ox * p.stride - p.pad_l + kx;
                        if ((unsigned)xx >= (unsigned)p.W) continue;
                        const float v = xb[((long)y * p.W + xx) * p.C];
                        if (v > best || by < 0) { best = v; by = y; bx = xx; }
                    }
                }
                if (by == iy && bx == ix) acc += p.g[(((long)b * p.Ho + oy) * p.Wo + ox) * p.C + c];
            }
        p.dx[e] = p.accumulate ? p.dx[e] + acc : acc;
    }
}

// y = x * r * gamma, r = rsqrt(max(sum_c x^2, 1e-12)).  One wave per pixel:
//   dx = gamma*dy*r - x * r^3 * sum_c(gamma*dy*x)   (second term only while sum x^2 > 1e-12)
//   tmp = dy * x * r  (column sums of tmp = d gamma)
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        const float* __restrict__ gamma, const long pixels,
                                                        const int C, float* __restrict__ dx, const int accumulate,
                                                        float* __restrict__ tmp) {
    const int lane = threadIdx.x & 63;
    const long wave0 = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * 256) >> 6;
    for (long px = wave0; px < pixels; px += nwaves) {
        const float* xr = x + px * C;
        const float* gr = dy + px * C;
        float s = 0.f, t = 0.f;
        for (int c = lane; c < C; c += 64) {
            s += xr[c] * xr[c];
            t += gamma[c] * gr[c] * xr[c];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); t += __shfl_xor(t, o); }
        const float r = 1.0f / sqrtf(fmaxf(s, 1e-12f));
        const float k3 = s > 1e-12f ? r * r * r * t : 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = gamma[c] * gr[c] * r - xr[c] * k3;
            dx[px * C + c] = accumulate ? dx[px * C + c] + v : v;
            tmp[px * C + c] = gr[c] * xr[c] * r;
        }
    }
}

// g += coef * w   (Keras l2 kernel regulariser: d(l2 * sum w^2)/dw = 2 * l2 * w)
__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ g, const float* __restrict__ w, const long n,
                                                  const float coef) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) g[e] += coef * w[e];
}

static inline int grid_for(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

}  // namespace ssd

// ====================================================================== training state (ssd_train.h)
void ssd_train_state_free(ssd_train_state* s) {
    if (!s) return;
    for (auto e : s->bucket_ev)
        if (e) (void)hipEventDestroy(e);
    if (s->wstream) { (void)hipStreamSynchronize(s->wstream); (void)hipStreamDestroy(s->wstream); }
    for (hipEvent_t e : {s->ev_dy, s->ev_wdone[0], s->ev_wdone[1], s->ev_wall, s->ev_main_pos})
        if (e) (void)hipEventDestroy(e);
    for (float* p : s->owned)
        if (p) (void)hipFree(p);
    if (s->loss_ws) (void)hipFree(s->loss_ws);
    delete s;
}

namespace ssd {

int talloc(ssd_train_state& s, size_t floats, float** out) {
    *out = nullptr;
    if (!floats) return SSD_OK;
    SSD_HIP(hipMalloc((void**)out, floats * sizeof(float)));
    s.owned.push_back(*out);
    return SSD_OK;
}

static bool trainable(const std::string& name) {
    const std::string var = name.substr(name.rfind('/') + 1);
    return var != "moving_mean" && var != "moving_variance";
}

// layers the training step executes: the un-fused layer list (fused kernels fold inference BatchNorm)
static bool train_runs(const Layer& l) { return l.kind == LK_CONV || l.kind == LK_DW || l.kind == LK_POOL || l.kind == LK_L2NORM; }

// ------------------------------------------------------------------ fine-tuning: trainable flags and the backward plan
static std::string keras_layer_of(const std::string& param) { return param.substr(0, param.rfind('/')); }
bool param_frozen(const ssd_net* net, int p) {
    return p >= 0 && !net->frozen.empty() && net->frozen.count(keras_layer_of(net->params[p].name)) != 0;
}
// a Keras layer that owns a trainable variable (one that owns only moving statistics cannot exist under this naming)
static bool known_keras_layer(const ssd_net* net, const std::string& name) {
    for (const auto& p : net->params)
        if (trainable(p.name) && keras_layer_of(p.name) == name) return true;
    return false;
}

// The backward plan: one SSD_PLAN_* word per layer, a pure function of the graph and net->frozen.  A tensor needs a gradient
// iff a trainable parameter lies upstream of it (the image never does); a layer hands a gradient only to inputs that need
// one, and a layer with nothing trainable whose inputs need none drops out of the backward.
static std::vector<int> backward_plan(const ssd_net* net) {
    std::vector<int> plan(net->layers.size(), 0);
    std::vector<char> needs(net->tensors.size(), 0);
    for (size_t i = 0; i < net->layers.size(); ++i) {
        const Layer& l = net->layers[i];
        if (!train_runs(l)) continue;
        int f = 0;
        if (l.kind == LK_L2NORM) {
            if (!param_frozen(net, l.p_gamma)) f |= SSD_PLAN_WGRAD;
        } else if (l.kind != LK_POOL) {
            if (!param_frozen(net, l.p_kernel)) f |= SSD_PLAN_WGRAD;
            if (l.p_kernel2 >= 0 && !param_frozen(net, l.p_kernel2)) f |= SSD_PLAN_WGRAD2;
            if (l.p_bn >= 0 && !param_frozen(net, l.p_bn)) f |= SSD_PLAN_BN_BATCH | SSD_PLAN_BN_PARAMS;
        }
        if (l.in > 0 && needs[l.in]) f |= SSD_PLAN_DGRAD;
        if (l.res >= 0 && needs[l.res]) f |= SSD_PLAN_RESGRAD;
        if (!f) f = SSD_PLAN_SKIP;
        else if (l.out >= 0) needs[l.out] = 1;
        plan[i] = f;
    }
    return plan;
}

static long chunks_for(long M, long unit_blocks, long* rows_per_chunk, long min_rows, long max_chunks) {
    long chunks = (2048 + unit_blocks - 1) / unit_blocks;          // ~8 workgroups per CU in total
    const long maxc = (M + min_rows - 1) / min_rows;
    if (chunks > maxc) chunks = maxc;
    if (chunks > max_chunks) chunks = max_chunks;                    // second-stage sums walk the chunks serially
    if (chunks < 1) chunks = 1;
    long rpc = (M + chunks - 1) / chunks;
    rpc = (rpc + 31) / 32 * 32;
    *rows_per_chunk = rpc;
    return (M + rpc - 1) / rpc;
}

// a partial-sum slab (s.partial / s.partial_w) of at least `floats`: grow-only; the old slab stays owned until the state is
// freed (sizes are planned once per batch)
static int ensure_slab(ssd_train_state& s, size_t floats, float** slab, size_t* have) {
    if (floats <= *have) return SSD_OK;
    float* p = nullptr;
    int rc = talloc(s, floats, &p);
    if (rc) return rc;
    *slab = p;
    *have = floats;
    return SSD_OK;
}

template <int OP>
static int col_reduce(ssd_train_state& s, RedParams p, long* chunks_out, hipStream_t st) {
    const bool vec = p.C % 4 == 0 && p.lda % 4 == 0 && (((uintptr_t)p.a | (uintptr_t)p.b) & 15) == 0;
    SSD_UNSUPPORTED_IF(!vec && OP == RED_STATS, "train: batch statistics need C %% 4 == 0 (C = %d)", p.C);
    // columns of a block: channel quads (16-byte form: a power of two <= 64 that wastes few lanes, C / 4 = 4 .. 320) or channels
    const int q = vec ? p.C / 4 : p.C;
    if (vec) p.cw = q % 64 == 0 ? 64 : (q % 32 == 0 ? 32 : (q % 16 == 0 ? 16 : (q % 8 == 0 ? 8 : (q < 8 ? 4 : (q < 48 ? 16 : 64)))));
    else p.cw = q % 64 == 0 ? 64 : (q % 32 == 0 ? 32 : (q % 16 == 0 ? 16 : (q < 64 ? 32 : 64)));
    const int ctiles = (q + p.cw - 1) / p.cw;
    long rpc = 0;
    const long chunks = chunks_for(p.M, ctiles, &rpc, 64, 256);
    int rc = ensure_slab(s, (size_t)chunks * 2 * p.C, &s.partial, &s.partial_floats);
    if (rc) return rc;
    p.rows_per_chunk = rpc;
    p.partial = s.partial;
    if (vec) hipLaunchKernelGGL(col_reduce4_kernel<OP>, dim3(ctiles, (unsigned)chunks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(col_reduce_kernel<OP>, dim3(ctiles, (unsigned)chunks), dim3(256), 0, st, p);
    SSD_LAUNCH_CHECK();
    *chunks_out = chunks;
    return SSD_OK;
}
static int col_finalize(ssd_train_state& s, long chunks, int C, float scale, float* out1, float* out2, int mode,
                        hipStream_t st) {
    hipLaunchKernelGGL(col_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, s.partial, (int)chunks, C, scale,
                       out1, out2, mode, kBnEps);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
// out[c] = scale * sum_m a[m * lda + c]
static int col_sum(ssd_train_state& s, const float* a, long M, int C, int lda, float scale, float* out, hipStream_t st) {
    RedParams p{};
    p.a = a; p.M = M; p.C = C; p.lda = lda;
    long chunks = 0;
    int rc = col_reduce<RED_SUM>(s, p, &chunks, st);
    if (!rc) rc = col_finalize(s, chunks, C, scale, out, nullptr, 0, st);
    return rc;
}

// batch statistics of pre [M][C] -> mean, var (biased), istd, and the moving-average update (unbiased variance): one
// pass over `pre` (shifted sums, see col_reduce4_kernel) + one finalize launch
static int bn_stats(ssd_train_state& s, TrainLayer& t, long M, int C, float* moving_mean, float* moving_var,
                    hipStream_t st) {
    RedParams p{};
    p.a = t.pre; p.M = M; p.C = C; p.lda = C;
    long chunks = 0;
    const float bessel = M > 1 ? (float)((double)M / (double)(M - 1)) : 1.0f;
    if (C % 4 == 0 && ((uintptr_t)t.pre & 15) == 0) {
        int rc = col_reduce<RED_STATS>(s, p, &chunks, st);
        if (rc) return rc;
        hipLaunchKernelGGL(col_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, s.partial, (int)chunks, C,
                           1.0f / (float)M, t.mean, t.var, 2, kBnEps, t.pre, t.istd, moving_mean, moving_var,
                           1.0f - kBnMomentum, bessel, M);
        SSD_LAUNCH_CHECK();
        return SSD_OK;
    }
    int rc = col_sum(s, t.pre, M, C, C, 1.0f / (float)M, t.mean, st);
    if (rc) return rc;
    p.mean = t.mean;
    rc = col_reduce<RED_SQDEV>(s, p, &chunks, st);
    if (!rc) rc = col_finalize(s, chunks, C, 1.0f / (float)M, t.var, t.istd, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(moving_update_kernel, dim3((C + 255) / 256), dim3(256), 0, st, moving_mean, moving_var, t.mean, t.var, C,
                       1.0f - kBnMomentum, bessel);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

static ConvParams dense_conv_params(int B, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int dil,
                                    int pt, int pl, int Ho, int Wo) {
    ConvParams p{};
    p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
    p.kh = kh; p.kw = kw; p.stride = stride; p.dil = dil; p.pad_t = pt; p.pad_l = pl;
    p.K = kh * kw * Cin;
    p.Kpad = conv_kpad(p.K);
    p.Npad = conv_npad(Cout);
    p.M = (long)B * Ho * Wo;
    p.split_k = 1;
    p.out_pixel_stride = Cout;
    p.out_batch_stride = (long)Ho * Wo * Cout;
    return p;
}

// Brings the training state's plan up to the net's trainable flags (ssd_net_set_trainable): the per-layer backward plan, the
// fold jobs of the frozen BatchNorms and the optimizer's table of the trainable ranges.  Runs when the flags changed since
// the last step / optimizer call, which is rare: it waits for the device (a launch in flight may still read the old tables)
// and uploads with blocking copies.  With nothing frozen there are no fold jobs and the step is the all-trainable one.
int refresh_plan(const ssd_net* net, ssd_train_state& s) {
    if (s.plan_rev == net->trainable_rev) return SSD_OK;
    s.plan = backward_plan(net);
    s.any_frozen = false;
    std::vector<FoldJob> folds;
    s.fold_maxC = 0;
    for (size_t i = 0; i < net->layers.size(); ++i) {
        const Layer& l = net->layers[i];
        if (!s.tl[i].active) continue;
        for (int q : {l.p_kernel, l.p_kernel2, l.p_bn, l.p_gamma}) s.any_frozen |= param_frozen(net, q);
        if (l.p_bn < 0 || (s.plan[i] & SSD_PLAN_BN_BATCH)) continue;
        folds.push_back(FoldJob{net->params[l.p_bn].dev, net->params[l.p_bn + 1].dev, net->params[l.p_bn + 2].dev,
                                net->params[l.p_bn + 3].dev, s.tl[i].fscale, s.tl[i].fshift, l.Cout});
        s.fold_maxC = std::max(s.fold_maxC, l.Cout);
    }
    SSD_CHECK_ARG((int)folds.size() <= s.fold_jobs_cap, "train: %zu BatchNorm fold jobs exceed their plan (%d)", folds.size(), s.fold_jobs_cap);
    SSD_HIP(hipDeviceSynchronize());
    const int rc = opt_refresh_tables(net, s);
    if (rc) return rc;
    if (!folds.empty()) SSD_HIP(hipMemcpy(s.fold_jobs, folds.data(), folds.size() * sizeof(FoldJob), hipMemcpyHostToDevice));
    s.n_fold_jobs = (int)folds.size();
    s.plan_rev = net->trainable_rev;
    return SSD_OK;
}

// The training step's environment switches, read once per process.
struct TrainEnv {
    int autotune;          // SSD_HIP_TRAIN_AUTOTUNE (default 1): 0 the cost model / heuristic tiles, 1 tiles timed on the device, 2 also prints them
    bool wgrad_stream;     // SSD_HIP_TRAIN_WGRAD_STREAM=0 (diagnostics): weight gradients in line on the caller's stream
    bool side_buckets;     // SSD_HIP_WGRAD_SIDE_BUCKETS=0: under gradient buckets the weight gradients run in line (StepCtx::side)
    bool debug_buckets;    // SSD_HIP_DEBUG_BUCKETS set: print every gradient bucket as it becomes final
};
static const TrainEnv& train_env() {
    static const TrainEnv env = [] {
        auto num = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : 1; };
        return TrainEnv{num("SSD_HIP_TRAIN_AUTOTUNE"), num("SSD_HIP_TRAIN_WGRAD_STREAM") != 0, num("SSD_HIP_WGRAD_SIDE_BUCKETS") != 0,
                        getenv("SSD_HIP_DEBUG_BUCKETS") != nullptr};
    }();
    return env;
}

// Tile choice of the training convs (forward and backward-data).  Default (SSD_HIP_TRAIN_AUTOTUNE unset or 1): the first
// time a conv shape is seen every valid tile of the net's precision is TIMED on the device (into a scratch output: a
// residual / accumulate-in-place epilogue must not run twice on the real tensor) and the fastest is kept for the process
// (measured: MobileNetV2 B=32 12.42 -> 11.15 ms per step, bf16 11.69 -> 10.70, VGG16 B=16 31.0 -> 28.8: the cost model
// favours large tiles that the short-K layers of a 32-image batch cannot fill).  Every step of a process runs the same
// tiles; ACROSS processes the choice -- and with it the last bits of a step -- may differ with the box (training has no
// bit-exactness contract; the inference path keeps its shipped tables).  SSD_HIP_TRAIN_AUTOTUNE=0: the cost model
// (conv_pick_config: deterministic); =2 also prints what was found.
struct TrainPickKey {
    long M, ops, obs; int K, Cout, kh, kw, stride, dil, H, W, Cin, flags, pad_t, pad_l;
    bool operator<(const TrainPickKey& o) const { return memcmp(this, &o, sizeof(*this)) < 0; }
};
// The memo of timed picks (conv tiles and weight-gradient tiles).  Nets of several host threads share it: the map and its
// mutex are reachable through the locked lookup and the locked store alone.
class PickMemo {
    std::mutex mu_;
    std::map<TrainPickKey, int> picks_;

public:
    bool lookup(const TrainPickKey& k, int* pick) {
        std::lock_guard<std::mutex> lock(mu_);
        const auto it = picks_.find(k);
        if (it != picks_.end()) *pick = it->second;
        return it != picks_.end();
    }
    void store(const TrainPickKey& k, int pick) {
        std::lock_guard<std::mutex> lock(mu_);
        picks_[k] = pick;
    }
};
static PickMemo& pick_memo() { static PickMemo m; return m; }

// The training step's tile race (windows: EventPair, ssd_net.h): every candidate launches once untimed (a candidate whose launch fails is left out), then takes
// the minimum over 3 trials of `reps` back-to-back launches; a candidate whose first trial takes more than twice the
// incumbent's time stops there.  `launch(c)` must be harmless to repeat.  false: the events could not be created.
struct TimedPick {
    int best;                  // the fastest candidate (`model` if none ran)
    float best_ms, model_ms;   // per `reps` launches
};
template <class Launch>
static bool time_candidates(const std::vector<int>& candidates, int model, int reps, hipStream_t st, Launch launch, TimedPick* out) {
    EventPair ev;
    if (ev.create()) { (void)hipGetLastError(); return false; }
    *out = TimedPick{model, 1e30f, 0.f};
    for (const int c : candidates) {
        if (launch(c)) { (void)hipGetLastError(); continue; }
        float ms = 1e30f;
        for (int trial = 0; trial < 3; ++trial) {
            float t = 0.f;
            (void)ev.window(st, reps, [&] { (void)launch(c); return 0; }, &t);      // (launch errors inside a window are ignored)
            ms = t < ms ? t : ms;
            if (trial == 0 && ms > 2.0f * out->best_ms) break;
        }
        if (c == model) out->model_ms = ms;
        if (ms < out->best_ms) { out->best_ms = ms; out->best = c; }
    }
    return true;
}

static int pick_measured(const ConvParams& p, hipStream_t st, int model_cfg, int verbose) {
    TrainPickKey k{};
    memset(&k, 0, sizeof(k));
    k.M = p.M; k.K = p.K; k.Cout = p.Cout; k.kh = p.kh; k.kw = p.kw; k.stride = p.stride; k.dil = p.dil; k.H = p.H; k.W = p.W;
    k.Cin = p.Cin; k.pad_t = p.pad_t; k.pad_l = p.pad_l; k.ops = p.out_pixel_stride; k.obs = p.out_batch_stride;
    k.flags = (p.residual ? 1 : 0) | (p.n_split ? 2 : 0) | (p.scale ? 4 : 0) | (p.shift ? 8 : 0) | (p.act << 4) | (p.bf16 << 8) |
              (p.vec_store << 9);
    int memo = 0;
    // (a memoised pick is re-validated against THESE parameters: alignment of the pointers is not part of the key)
    if (pick_memo().lookup(k, &memo)) return conv_config_valid(memo, p) ? memo : model_cfg;
    ScopedDev scratch;
    const size_t out_floats = (size_t)p.M * (size_t)(p.out_pixel_stride > p.Cout ? p.out_pixel_stride : p.Cout) + 4096;
    if (hipMalloc((void**)&scratch.p, out_floats * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return model_cfg; }
    ConvParams q = p;
    q.out = scratch.p;
    if (q.n_split) { q.out2 = scratch.p; q.n_split = 0; }          // (timing only: one destination)
    q.out_batch_stride = (long)p.Ho * p.Wo * q.out_pixel_stride;
    std::vector<int> candidates;
    for (int c = 0; c < conv_num_configs(); ++c) {
        if (!conv_config_valid(c, q) || !conv_config_allowed(c, q.bf16)) continue;
        const ConvFamilyId f = conv_config_family(c);
        if (f == CF_WINO || f == CF_SKINNY || (f == CF_DIRECT && c != model_cfg)) continue;
        candidates.push_back(c);
    }
    TimedPick r;
    if (!time_candidates(candidates, model_cfg, 3, st, [&](int c) { return conv_launch(q, c, st); }, &r)) return model_cfg;
    if (verbose)
        fprintf(stderr, "[ssd train tune] M=%ld K=%d N=%d k%dx%d s%d: model %s %.1f us -> %s %.1f us\n", p.M, p.K, p.Cout, p.kh, p.kw,
                p.stride, conv_config_name(model_cfg), r.model_ms * 1000.f / 3, conv_config_name(r.best), r.best_ms * 1000.f / 3);
    pick_memo().store(k, r.best);
    return r.best;
}

// Launches one training conv on its tile and adds its matrix-core FLOPs to the step's counters, per instruction family
// (bench.py prices each at its own peak): s.step_flops[0] fp32-MFMA tiles, [1] split-bf16 / bf16 tiles
static int launch_conv(ssd_train_state& s, ConvParams& p, hipStream_t st) {
    p.vec_store = conv_vec_store(p);
    int cfg = conv_pick_config(p);
    SSD_UNSUPPORTED_IF(cfg < 0, "train: no conv kernel for Cin=%d Cout=%d k=%dx%d", p.Cin, p.Cout, p.kh, p.kw);
    if (const int tune = train_env().autotune) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cs);
        if (cs == hipStreamCaptureStatusNone) cfg = pick_measured(p, st, cfg, tune > 1);
    }
    const ConvFamilyId f = conv_config_family(cfg);
    s.step_flops[(f == CF_MFMA3 || f == CF_BF16) ? 1 : 0] += 2.0 * (double)p.M * p.K * p.Cout;
    return conv_launch(p, cfg, st);
}

// dW [K][N] (row-major, = Keras HWIO) = im2col(X)^T * G with tile shape `cfg`.  The M chunks' partial sums go to the
// caller's slab `partial` (`partial_floats` floats, wgrad_chunks * K * N are needed: too small a slab is an argument error).
static long wgrad_chunks(const Layer& l, int B, int N, const WgradCfg* cfg, long* rows_per_chunk, long* tiles_out) {
    const bool im2col = l.Cin % 4 != 0;
    const int rows = im2col ? l.kh * l.kw * l.Cin : l.Cin;
    const long ctiles = (rows + cfg->tc - 1) / cfg->tc, ntiles = (N + cfg->tn - 1) / cfg->tn;
    const long tiles = (im2col ? 1L : (long)l.kh * l.kw) * ctiles * ntiles;
    const long M = (long)B * l.Ho * l.Wo;
    long rpc = 0;
    long chunks = chunks_for(M, tiles, &rpc, 128, 1024);
    // bound the slab: chunks * K * N floats
    const size_t kn = (size_t)l.kh * l.kw * l.Cin * N;
    while (chunks > 1 && (size_t)chunks * kn > ((size_t)96 << 20)) {
        rpc *= 2;
        chunks = (M + rpc - 1) / rpc;
    }
    *rows_per_chunk = rpc;
    if (tiles_out) *tiles_out = tiles;
    return chunks;
}
static int wgrad_with(const Layer& l, int B, const float* x, const float* g, int ldg, int N, float* dW, hipStream_t st,
                      const WgradCfg* cfg, float* partial, size_t partial_floats) {
    WgradParams p{};
    p.x = x; p.g = g;
    p.B = B; p.H = l.H; p.W = l.W; p.Cin = l.Cin; p.Ho = l.Ho; p.Wo = l.Wo;
    p.kh = l.kh; p.kw = l.kw; p.stride = l.stride; p.dil = l.dil; p.pad_t = l.pt; p.pad_l = l.pl;
    p.N = N; p.ldg = ldg; p.K = l.kh * l.kw * l.Cin;
    p.M = (long)B * l.Ho * l.Wo;
    p.im2col = l.Cin % 4 != 0;            // RGB stems (Cin = 3): one tile spans all K = 27 rows instead of 3 of 16 per tap
    const int rows = p.im2col ? p.K : l.Cin;
    p.ctiles = (rows + cfg->tc - 1) / cfg->tc;
    p.ntiles = (N + cfg->tn - 1) / cfg->tn;
    p.vec_x = (l.Cin % 4 == 0) && (((uintptr_t)x & 15) == 0);
    p.vec_g = (ldg % 4 == 0) && (((uintptr_t)g & 15) == 0);
    long rpc = 0, tiles = 0;
    const long chunks = wgrad_chunks(l, B, N, cfg, &rpc, &tiles);
    const size_t kn = (size_t)p.K * N;
    SSD_CHECK_ARG((size_t)chunks * kn <= partial_floats, "weight gradient: the workspace holds %zu floats, %zu are needed",
                  partial_floats, (size_t)chunks * kn);
    p.rows_per_chunk = rpc;
    p.partial = partial;
    hipLaunchKernelGGL(cfg->fn, dim3((unsigned)tiles, (unsigned)chunks), dim3(256), 0, st, p);
    SSD_LAUNCH_CHECK();
    return chunk_sum(partial, chunks, (long)kn, dW, st);
}
// the training step's slab: grow-only, its own (weight gradients may run beside the reductions of the main chain)
static int wgrad_with(ssd_train_state& s, const Layer& l, int B, const float* x, const float* g, int ldg, int N, float* dW,
                      hipStream_t st, const WgradCfg* cfg) {
    long rpc = 0;
    const size_t need = (size_t)wgrad_chunks(l, B, N, cfg, &rpc, nullptr) * l.kh * l.kw * l.Cin * N;
    const int rc = ensure_slab(s, need, &s.partial_w, &s.partial_w_floats);
    if (rc) return rc;
    return wgrad_with(l, B, x, g, ldg, N, dW, st, cfg, s.partial_w, s.partial_w_floats);
}

// Heuristic tile shape: least padded tile area first (MFMA work); among equals the shape that stages the fewest floats
// per M row (see wgrad below)
static const WgradCfg* wgrad_heuristic(const Layer& l, int N) {
    const bool im2col = l.Cin % 4 != 0;
    const int rows = im2col ? l.kh * l.kw * l.Cin : l.Cin;
    const WgradCfg* cfg = &kWgrad[0];
    long best_area = -1, best_staged = -1;
    for (const auto& c : kWgrad) {
        const long ct = (rows + c.tc - 1) / c.tc, nt = (N + c.tn - 1) / c.tn;
        const long area = ct * c.tc * nt * c.tn, staged = ct * nt * (c.tc + c.tn);
        if (best_area < 0 || area < best_area || (area == best_area && staged < best_staged)) {
            best_area = area; best_staged = staged; cfg = &c;
        }
    }
    return cfg;
}

// Depthwise 3x3 backward: weight gradient (M chunks into dp.partial [chunks][9][C], then their sum) and data gradient
// (stride 1: the four-column form).  dw_bwd_chunks sets dp.rows_per_chunk and returns the chunk count.
static long dw_bwd_chunks(DwBwdParams& dp) {
    long rpc = 0;
    const long chunks = chunks_for(dp.M, (dp.C + 63) / 64, &rpc, 64, 2048);
    dp.rows_per_chunk = rpc;
    return chunks;
}
static int dw_bwd_launch(const DwBwdParams& dp, long chunks, float* dw_out, hipStream_t st, bool want_dw = true, bool want_dx = true) {
    if (want_dw) {
        hipLaunchKernelGGL(dw_wgrad_kernel, dim3((dp.C + 63) / 64, (unsigned)chunks), dim3(256), 0, st, dp);
        const int rc = chunk_sum(dp.partial, chunks, 9L * dp.C, dw_out, st);
        if (rc) return rc;
    }
    if (!want_dx) return SSD_OK;
    if (dp.stride == 1)
        hipLaunchKernelGGL(dw_dgrad4_kernel, dim3(grid_for((long)dp.B * dp.H * ((dp.W + 3) / 4) * (dp.C / 4))), dim3(256), 0, st, dp);
    else
        hipLaunchKernelGGL(dw_dgrad_kernel, dim3(grid_for((long)dp.B * dp.H * dp.W * (dp.C / 4))), dim3(256), 0, st, dp);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

// Tile shape of a weight gradient.  Heuristic: least padded tile area first (MFMA work); among equals the shape that
// stages the fewest floats per M row (every tile re-reads its 32-row slabs of X and G: ctiles * ntiles * (tc + tn)).
// Measured: by staged floats alone 128 x 128 wins everywhere, +4 % on VGG16 (512-channel layers, no padding) but -3 % on
// MobileNetV2 (96 -> 576 expands padded to 128 x 640); the lexicographic rule keeps both.  With SSD_HIP_TRAIN_AUTOTUNE
// (default on, see pick_measured) every shape of the table is timed the first time a layer is seen (dW is written, not
// accumulated: running it repeatedly is harmless) and the fastest kept for the process.  The launch that counts adds its
// matrix-core FLOPs to s.step_flops[2].
static int wgrad(ssd_train_state& s, const Layer& l, int B, const float* x, const float* g, int ldg, int N, float* dW,
                 hipStream_t st) {
    const WgradCfg* cfg = wgrad_heuristic(l, N);
    const long M = (long)B * l.Ho * l.Wo;
    const int K = l.kh * l.kw * l.Cin;
    const int tune = train_env().autotune;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (tune && cs == hipStreamCaptureStatusNone) {
        TrainPickKey k{};
        memset(&k, 0, sizeof(k));
        k.M = M; k.K = K; k.Cout = N; k.kh = l.kh; k.kw = l.kw; k.stride = l.stride;
        k.dil = l.dil; k.H = l.H; k.W = l.W; k.Cin = l.Cin; k.flags = (1 << 20) | ldg;      // bit 20: a weight gradient
        int pick = (int)(cfg - kWgrad);
        if (!pick_memo().lookup(k, &pick)) {
            std::vector<int> candidates;
            for (int c = 0; c < (int)(sizeof(kWgrad) / sizeof(kWgrad[0])); ++c) candidates.push_back(c);
            TimedPick r;
            const auto launch = [&](int c) { return wgrad_with(s, l, B, x, g, ldg, N, dW, st, &kWgrad[c]); };
            if (time_candidates(candidates, pick, 2, st, launch, &r)) {
                if (tune > 1)
                    fprintf(stderr, "[ssd train tune] wgrad M=%ld K=%d N=%d: heuristic %dx%d %.1f us -> %dx%d %.1f us\n", M, K, N, cfg->tc,
                            cfg->tn, r.model_ms * 500.f, kWgrad[r.best].tc, kWgrad[r.best].tn, r.best_ms * 500.f);
                pick_memo().store(k, r.best);
                pick = r.best;
            }
        }
        cfg = &kWgrad[pick];
    }
    s.step_flops[2] += 2.0 * (double)M * K * N;
    return wgrad_with(s, l, B, x, g, ldg, N, dW, st, cfg);
}

// ------------------------------------------------------------------ the step, layer by layer
// What one ssd_net_train_forward_backward call carries from layer to layer.
struct StepCtx {
    ssd_net* net;
    ssd_train_state& s;
    hipStream_t st;             // the caller's stream
    int B;
    float* grads;               // the caller's flat gradient vector
    // The dense convs' weight gradients run on the side stream (s.wstream) beside the rest of the backward: they are needed
    // only at the end of the step / at their gradient bucket, the data-gradient chain does not wait for them.  Under gradient
    // buckets only with SSD_HIP_WGRAD_SIDE_BUCKETS on (the default; off: the communication stream already runs beside the
    // backward, and a third stream measured slower at world size 1 -- 12.6 against 11.5 ms -- than the weight gradients in line)
    bool side;
    int dy_cur = 0;             // dY alternates between s.dy_buf[0] and [1]
    size_t next_bucket = 0;     // gradient buckets at and above this one are published

    // next dY buffer: the main stream first waits for the weight gradient still reading it
    float* acquire_dy() {
        dy_cur ^= 1;
        if (s.wstream && s.wpending[dy_cur]) {
            (void)hipStreamWaitEvent(st, s.ev_wdone[dy_cur], 0);
            s.wpending[dy_cur] = false;
        }
        return s.dy_buf[dy_cur];
    }
    // everything issued on the side stream so far is ordered before what follows on st
    int join_wgrads() {
        if (!s.wstream) return SSD_OK;
        SSD_HIP(hipEventRecord(s.ev_wall, s.wstream));
        SSD_HIP(hipStreamWaitEvent(st, s.ev_wall, 0));
        s.wpending[0] = s.wpending[1] = false;
        return SSD_OK;
    }
    // Everything at or above `threshold` in the flat vector is final: publish those buckets.  A bucket is final when BOTH
    // streams have passed this point: the main stream (BatchNorm / depthwise / bias gradients, the data-gradient chain) and the
    // side stream (the dense convs' weight gradients).  The bucket's event is recorded on the SIDE stream behind a wait for the
    // main stream's position -- the main stream itself never waits (round 4 joined the side stream INTO the main stream here and
    // therefore ran the weight gradients in line under buckets: +0.9 ms per step).
    int mark_ready(long threshold) {
        bool joined = false;
        for (; next_bucket > 0 && s.bucket_lo[next_bucket - 1] >= threshold; --next_bucket) {
            const size_t k = next_bucket - 1;
            if (train_env().debug_buckets) fprintf(stderr, "[ssd] bucket %zu (lo %ld) final at threshold %ld\n", k, s.bucket_lo[k], threshold);
            if (!joined && side) {
                SSD_HIP(hipEventRecord(s.ev_main_pos, st));
                SSD_HIP(hipStreamWaitEvent(s.wstream, s.ev_main_pos, 0));
            } else if (!joined) {
                const int rj = join_wgrads();
                if (rj) return rj;
            }
            joined = true;
            SSD_HIP(hipEventRecord(s.bucket_ev[k], side ? s.wstream : st));
        }
        return SSD_OK;
    }
};

static int train_forward_conv(StepCtx& c, const Layer& l, TrainLayer& t, bool bn_frozen) {
    ssd_train_state& s = c.s;
    ConvParams p = dense_conv_params(c.B, l.H, l.W, l.Cin, l.Cout, l.kh, l.kw, l.stride, l.dil, l.pt, l.pl, l.Ho, l.Wo);
    p.in = s.act[l.in];
    p.w = t.wfwd;
    p.w3 = conv_split_planes(t.wfwd, l.kh * l.kw * l.Cin, l.Cout);
    p.bf16 = c.net->precision;          // precision 1: the cost model takes the bf16 (one-product) tiles
    p.act = l.p_bn >= 0 ? SSD_ACT_NONE : l.act;      // BatchNorm layers: the activation follows the normalisation (bn_apply_kernel)
    if (bn_frozen) {
        // frozen BatchNorm: folded on the moving statistics, the epilogue writes act(scale * conv + shift) (+ residual) --
        // one launch, no `pre` traffic, no statistics pass, no bn_apply_kernel
        p.scale = t.fscale;
        p.shift = t.fshift;
        p.act = l.act;
        p.residual = l.res >= 0 ? s.act[l.res] : nullptr;
        p.out = s.act[l.out];
    } else if (l.p_bn >= 0) {
        p.out = t.pre;
    } else if (l.head_kind == 0) {
        p.shift = l.p_bias2 >= 0 ? nullptr : c.net->params[l.p_bias].dev;
        p.out = s.act[l.out];
    } else {
        // fused label + box head conv: bias vector = [label bias | box bias]
        SSD_HIP(hipMemcpyAsync(s.dgamma_tmp, c.net->params[l.p_bias].dev, (size_t)l.Cout1 * sizeof(float), hipMemcpyDeviceToDevice, c.st));
        SSD_HIP(hipMemcpyAsync(s.dgamma_tmp + l.Cout1, c.net->params[l.p_bias2].dev, (size_t)(l.Cout - l.Cout1) * sizeof(float),
                               hipMemcpyDeviceToDevice, c.st));
        p.shift = s.dgamma_tmp;
        conv_route_head(p, l, s.probs, s.deltas);
    }
    return launch_conv(s, p, c.st);
}

// training-mode forward of layer i: BatchNorm on the batch statistics, moving averages updated -- unless it is frozen
// (Keras trainable = False, TF 2.0: inference mode), then the layer is one launch on the folded moving statistics
static int train_forward_layer(StepCtx& c, size_t i) {
    ssd_train_state& s = c.s;
    const ssd_net* net = c.net;
    const Layer& l = net->layers[i];
    TrainLayer& t = s.tl[i];
    const long M = (long)c.B * l.Ho * l.Wo;
    const float* x = s.act[l.in];
    if (l.kind == LK_POOL) return launch_maxpool(x, c.B, l.H, l.W, l.Cin, l.kh, l.stride, l.pt, l.pl, l.Ho, l.Wo, s.act[l.out], c.st);
    if (l.kind == LK_L2NORM) return launch_l2norm(x, M, l.Cin, net->params[l.p_gamma].dev, s.act[l.out], c.st);
    const bool bn_frozen = l.p_bn >= 0 && !(s.plan[i] & SSD_PLAN_BN_BATCH);
    if (bn_frozen && l.kind == LK_DW) {
        SSD_UNSUPPORTED_IF(l.res >= 0, "train: depthwise layer %s has a residual input", l.name.c_str());
        return launch_dwconv3x3(x, c.B, l.H, l.W, l.Cin, l.stride, l.pt, l.pl, l.Ho, l.Wo, net->params[l.p_kernel].dev, t.fscale,
                                t.fshift, l.act, s.act[l.out], c.st);
    }
    int rc = l.kind == LK_CONV ? train_forward_conv(c, l, t, bn_frozen)
                               : launch_dwconv3x3(x, c.B, l.H, l.W, l.Cin, l.stride, l.pt, l.pl, l.Ho, l.Wo, net->params[l.p_kernel].dev,
                                                  nullptr, nullptr, SSD_ACT_NONE, t.pre, c.st);
    if (rc || l.p_bn < 0 || bn_frozen) return rc;
    rc = bn_stats(s, t, M, l.Cout, net->params[l.p_bn + 2].dev, net->params[l.p_bn + 3].dev, c.st);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(M * l.Cout)), dim3(256), 0, c.st, t.pre, M, l.Cout, t.mean, t.istd,
                       net->params[l.p_bn].dev, net->params[l.p_bn + 1].dev, l.act, l.res >= 0 ? s.act[l.res] : nullptr, s.act[l.out]);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

static int bwd_pool(StepCtx& c, const Layer& l) {
    ssd_train_state& s = c.s;
    PoolBwdParams pp{};
    pp.x = s.act[l.in]; pp.g = s.gact[l.out]; pp.dx = s.gact[l.in];
    pp.B = c.B; pp.H = l.H; pp.W = l.W; pp.C = l.Cin; pp.Ho = l.Ho; pp.Wo = l.Wo;
    pp.k = l.kh; pp.stride = l.stride; pp.pad_t = l.pt; pp.pad_l = l.pl;
    pp.accumulate = s.gwritten[l.in];
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for((long)c.B * l.H * l.W * l.Cin)), dim3(256), 0, c.st, pp);
    SSD_LAUNCH_CHECK();
    s.gwritten[l.in] = 1;
    return SSD_OK;
}

// L2 normalisation: dX, and d gamma = column sums of the per-element products the kernel leaves in `tmp`
// (`plan`: without SSD_PLAN_DGRAD the kernel's dX is left unused -- the input needs no gradient, nobody reads it --, without
// SSD_PLAN_WGRAD the scale is frozen and its column sums are not taken)
static int bwd_l2norm(StepCtx& c, const Layer& l, const TrainLayer& t, float* tmp, int plan) {
    ssd_train_state& s = c.s;
    const long M = (long)c.B * l.Ho * l.Wo, blocks = (M + 3) / 4;
    const bool dgrad = plan & SSD_PLAN_DGRAD;
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, c.st, s.act[l.in], s.gact[l.out],
                       c.net->params[l.p_gamma].dev, M, l.Cin, s.gact[l.in], dgrad ? (int)s.gwritten[l.in] : 0, tmp);
    SSD_LAUNCH_CHECK();
    if (dgrad) s.gwritten[l.in] = 1;
    if (!(plan & SSD_PLAN_WGRAD)) return SSD_OK;
    return col_sum(s, tmp, M, l.Cin, l.Cin, 1.0f, c.grads + t.g_gamma, c.st);
}

// The three ways to dY, the gradient w.r.t. a conv / depthwise output as a dense [M][*ldy] matrix (in `dyb` unless it is dOut
// itself); each also writes the layer's bias or BatchNorm parameter gradients.
// Head conv: one level gathered out of the concatenated [B,N,K] gradients of the loss; bias gradients = its column sums
static int bwd_head_dy(StepCtx& c, const Layer& l, const TrainLayer& t, float* dyb, const float** dY, int* ldy, int plan) {
    ssd_train_state& s = c.s;
    const long M = (long)c.B * l.Ho * l.Wo;
    const int ld = t.cpad, C2 = l.Cout - l.Cout1;
    if (t.cpad != l.Cout) SSD_HIP(hipMemsetAsync(dyb, 0, (size_t)M * ld * sizeof(float), c.st));
    hipLaunchKernelGGL(gather_head_kernel, dim3(grid_for(M * l.Cout1)), dim3(256), 0, c.st, s.glogits, l.head_bs, l.head_off, l.head_ps,
                       c.B, l.Ho * l.Wo, l.Cout1, dyb, ld, 0);
    hipLaunchKernelGGL(gather_head_kernel, dim3(grid_for(M * C2)), dim3(256), 0, c.st, s.gdeltas, l.head2_bs, l.head2_off, l.head2_ps,
                       c.B, l.Ho * l.Wo, C2, dyb, ld, l.Cout1);
    SSD_LAUNCH_CHECK();
    *dY = dyb; *ldy = ld;
    if (!(plan & (SSD_PLAN_WGRAD | SSD_PLAN_WGRAD2))) return SSD_OK;        // both convs of the level frozen: no bias gradients
    const int rc = col_sum(s, dyb, M, l.Cout, ld, 1.0f, s.dbeta_tmp, c.st);
    if (rc) return rc;
    if (plan & SSD_PLAN_WGRAD)
        SSD_HIP(hipMemcpyAsync(c.grads + t.g_bias, s.dbeta_tmp, (size_t)l.Cout1 * sizeof(float), hipMemcpyDeviceToDevice, c.st));
    if (plan & SSD_PLAN_WGRAD2)
        SSD_HIP(hipMemcpyAsync(c.grads + t.g_bias2, s.dbeta_tmp + l.Cout1, (size_t)C2 * sizeof(float), hipMemcpyDeviceToDevice, c.st));
    return SSD_OK;
}
// out = bn(conv) + res: the residual branch receives dOut as is
static int bwd_residual(StepCtx& c, const Layer& l, int plan) {
    if (l.res < 0 || !(plan & SSD_PLAN_RESGRAD)) return SSD_OK;
    const long n = (long)c.B * l.Ho * l.Wo * l.Cout;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, c.st, c.s.gact[l.res], c.s.gact[l.out], n, (int)c.s.gwritten[l.res]);
    SSD_LAUNCH_CHECK();
    c.s.gwritten[l.res] = 1;
    return SSD_OK;
}
// (`plan`: a layer whose conv is frozen and whose input needs no gradient has no use for dY -- only dgamma / dbeta are made)
static int bwd_bn_dy(StepCtx& c, const Layer& l, const TrainLayer& t, float* dyb, const float** dY, int plan) {
    const float* dOut = c.s.gact[l.out];
    int rc = bwd_residual(c, l, plan);
    if (rc) return rc;
    const long M = (long)c.B * l.Ho * l.Wo;
    if (!(plan & SSD_PLAN_BN_BATCH)) {
        // frozen BatchNorm: dY = dOut * act'(out) * scale (bn_frozen_bwd4_kernel), no reductions
        *dY = dyb;
        if (!(plan & (SSD_PLAN_WGRAD | SSD_PLAN_DGRAD))) return SSD_OK;
        SSD_UNSUPPORTED_IF(l.res >= 0 && l.act != SSD_ACT_NONE, "train: %s has a residual add behind an activation: the stored output is no pass-mask",
                           l.name.c_str());
        const float* out = c.s.act[l.out];
        const long total = M * l.Cout;
        if (l.Cout % 4 == 0 && ((((uintptr_t)dOut | (uintptr_t)out | (uintptr_t)t.fscale | (uintptr_t)dyb) & 15) == 0))
            hipLaunchKernelGGL(bn_frozen_bwd4_kernel, dim3(grid_for(total / 4)), dim3(256), 0, c.st, reinterpret_cast<const f32x4*>(dOut),
                               reinterpret_cast<const f32x4*>(out), reinterpret_cast<const f32x4*>(t.fscale), total / 4, l.Cout / 4,
                               l.act, reinterpret_cast<f32x4*>(dyb));
        else
            hipLaunchKernelGGL(bn_frozen_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, c.st, dOut, out, t.fscale, total, l.Cout, l.act, dyb);
        SSD_LAUNCH_CHECK();
        return SSD_OK;
    }
    const float *gamma = c.net->params[l.p_bn].dev, *beta = c.net->params[l.p_bn + 1].dev;
    float *dgamma = c.grads + t.g_gamma, *dbeta = c.grads + t.g_beta;
    RedParams rp{};
    rp.a = dOut; rp.b = t.pre; rp.mean = t.mean; rp.istd = t.istd; rp.gamma = gamma; rp.beta = beta;
    rp.M = M; rp.C = l.Cout; rp.lda = l.Cout; rp.act = l.act;
    long chunks = 0;
    rc = col_reduce<RED_BN_BWD>(c.s, rp, &chunks, c.st);
    if (!rc) rc = col_finalize(c.s, chunks, l.Cout, 1.0f, dbeta, dgamma, 0, c.st);      // s1 = dbeta, s2 = dgamma
    if (rc) return rc;
    *dY = dyb;
    if (!(plan & (SSD_PLAN_WGRAD | SSD_PLAN_DGRAD))) return SSD_OK;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(M * l.Cout)), dim3(256), 0, c.st, dOut, t.pre, M, l.Cout, t.mean, t.istd,
                       gamma, beta, l.act, dgamma, dbeta, dyb);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}
// (`plan`: a frozen conv has no bias gradient; it is in the backward only for its data gradient)
static int bwd_bias_act_dy(StepCtx& c, const Layer& l, const TrainLayer& t, float* dyb, const float** dY, int plan) {
    ssd_train_state& s = c.s;
    const float* dOut = s.gact[l.out];
    int rc = bwd_residual(c, l, plan);
    if (rc) return rc;
    const long M = (long)c.B * l.Ho * l.Wo;
    if (plan & SSD_PLAN_WGRAD) {
        RedParams rp{};
        rp.a = dOut; rp.b = l.act ? s.act[l.out] : nullptr;
        rp.M = M; rp.C = l.Cout; rp.lda = l.Cout; rp.act = l.act;
        long chunks = 0;
        rc = col_reduce<RED_ACT_BWD>(s, rp, &chunks, c.st);
        if (!rc) rc = col_finalize(s, chunks, l.Cout, 1.0f, c.grads + t.g_bias, nullptr, 0, c.st);
        if (rc) return rc;
    }
    *dY = dOut;
    if (!l.act) return SSD_OK;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(M * l.Cout)), dim3(256), 0, c.st, dOut, s.act[l.out], M * l.Cout, l.act, dyb);
    SSD_LAUNCH_CHECK();
    *dY = dyb;
    return SSD_OK;
}

static int bwd_depthwise(StepCtx& c, const Layer& l, const TrainLayer& t, const float* dY, int plan) {
    ssd_train_state& s = c.s;
    DwBwdParams dp{};
    dp.x = s.act[l.in]; dp.g = dY; dp.w = c.net->params[l.p_kernel].dev; dp.dx = s.gact[l.in];
    dp.B = c.B; dp.H = l.H; dp.W = l.W; dp.C = l.Cin; dp.Ho = l.Ho; dp.Wo = l.Wo;
    dp.stride = l.stride; dp.pad_t = l.pt; dp.pad_l = l.pl;
    dp.M = (long)c.B * l.Ho * l.Wo;
    dp.accumulate = s.gwritten[l.in];
    const long chunks = dw_bwd_chunks(dp);
    int rc = ensure_slab(s, (size_t)chunks * 9 * l.Cin, &s.partial, &s.partial_floats);
    if (rc) return rc;
    dp.partial = s.partial;
    const bool dgrad = plan & SSD_PLAN_DGRAD;
    if (dgrad) s.gwritten[l.in] = 1;
    return dw_bwd_launch(dp, chunks, c.grads + t.g_kernel, c.st, plan & SSD_PLAN_WGRAD, dgrad);
}

// dense conv: weight gradient(s), on the side stream behind dY (StepCtx::side)
static int bwd_dense_wgrad(StepCtx& c, const Layer& l, const TrainLayer& t, const float* dY, int ldy, const float* dyb, int plan) {
    ssd_train_state& s = c.s;
    if (!(plan & (SSD_PLAN_WGRAD | SSD_PLAN_WGRAD2))) return SSD_OK;       // frozen
    const float* x = s.act[l.in];
    hipStream_t wst = c.side ? s.wstream : c.st;
    if (c.side) {
        SSD_HIP(hipEventRecord(s.ev_dy, c.st));
        SSD_HIP(hipStreamWaitEvent(s.wstream, s.ev_dy, 0));
    }
    int rc;
    if (l.p_kernel2 < 0) {
        rc = wgrad(s, l, c.B, x, dY, ldy, l.Cout, c.grads + t.g_kernel, wst);
    } else {
        // the label and the box conv of a head level freeze independently
        rc = (plan & SSD_PLAN_WGRAD) ? wgrad(s, l, c.B, x, dY, ldy, l.Cout1, c.grads + t.g_kernel, wst) : SSD_OK;
        if (!rc && (plan & SSD_PLAN_WGRAD2)) rc = wgrad(s, l, c.B, x, dY + l.Cout1, ldy, l.Cout - l.Cout1, c.grads + t.g_kernel2, wst);
    }
    if (rc) return rc;
    // VGG16: kernel_regularizer=l2(5e-4) on every backbone / extra conv (models/ssd_vgg16.py:44-45; the head
    // convs of models/header.py have none): d(5e-4 * sum w^2)/dw = 1e-3 * w, added right behind the layer's
    // weight gradient so that the gradient bucket it lies in is final when the backward has passed the layer
    if (c.net->backbone == SSD_VGG16 && !l.head_kind) {
        const Param& w = c.net->params[l.p_kernel];
        hipLaunchKernelGGL(axpy_kernel, dim3(grid_for((long)w.count)), dim3(256), 0, wst, c.grads + t.g_kernel, w.dev, (long)w.count,
                           2.0f * 5e-4f);
        SSD_LAUNCH_CHECK();
    }
    if (c.side && dY == dyb) {             // the buffer may be rewritten only after this weight gradient
        SSD_HIP(hipEventRecord(s.ev_wdone[c.dy_cur], s.wstream));
        s.wpending[c.dy_cur] = true;
    }
    return SSD_OK;
}

// dense conv: data gradient = conv of dY (stride 2: zero-inserted first) with the rotated / transposed weights
static int bwd_dense_dgrad(StepCtx& c, const Layer& l, const TrainLayer& t, const float* dY, int ldy) {
    ssd_train_state& s = c.s;
    const int d = l.dil, kh = l.kh, kw = l.kw;
    const float* gin = dY;
    int Hg = l.Ho, Wg = l.Wo;
    if (l.stride == 2) {
        Hg = (l.Ho - 1) * 2 + 1;
        Wg = (l.Wo - 1) * 2 + 1;
        SSD_HIP(hipMemsetAsync(s.scratch_dz, 0, (size_t)c.B * Hg * Wg * ldy * sizeof(float), c.st));
        hipLaunchKernelGGL(dilate2_kernel, dim3(grid_for((long)c.B * l.Ho * l.Wo * ldy)), dim3(256), 0, c.st, dY, c.B, l.Ho, l.Wo, ldy, Hg,
                           Wg, s.scratch_dz);
        SSD_LAUNCH_CHECK();
        gin = s.scratch_dz;
    }
    const int pt = (kh - 1) * d - l.pt, pl = (kw - 1) * d - l.pl;
    SSD_UNSUPPORTED_IF(pt < 0 || pl < 0, "train: backward-data padding of %s is negative", l.name.c_str());
    ConvParams p = dense_conv_params(c.B, Hg, Wg, ldy, l.Cin, kh, kw, 1, d, pt, pl, l.H, l.W);
    p.in = gin;
    p.w = t.wbwd;
    p.w3 = conv_split_planes(t.wbwd, p.K, p.Cout);
    p.bf16 = c.net->precision;
    p.out = s.gact[l.in];
    p.act = SSD_ACT_NONE;
    p.residual = s.gwritten[l.in] ? s.gact[l.in] : nullptr;      // accumulate in the epilogue
    s.gwritten[l.in] = 1;
    return launch_conv(s, p, c.st);
}

// ------------------------------------------------------------------ ssd_net_train_begin, step by step
struct TrainSizes {             // the largest of each scratch buffer over the layers
    size_t max_out = 0, max_dz = 0;
    int maxC = 0;
};

// flat parameter vector (trainable parameters in table order) with the optimizer's two slots, and every parameter's offset in it
static int begin_flat(const ssd_net* net, ssd_train_state& s) {
    s.P = ssd_net_trainable_floats(net);
    int rc = talloc(s, s.P, &s.flat);
    if (!rc) rc = talloc(s, s.P, &s.m);
    if (!rc) rc = talloc(s, s.P, &s.v);
    s.poff.assign(net->params.size(), -1);
    long off = 0;
    for (size_t i = 0; i < net->params.size(); ++i) {
        if (!trainable(net->params[i].name)) continue;
        s.poff[i] = off;
        off += (long)net->params[i].count;
    }
    return rc;
}

// activations and their gradients, then per layer: gradient offsets, BatchNorm buffers, packed weights; the scratch sizes
static int begin_plan_layers(const ssd_net* net, ssd_train_state& s, TrainSizes& sz) {
    const int batch = s.batch;
    int rc = SSD_OK;
    s.act.assign(net->tensors.size(), nullptr);
    s.gact.assign(net->tensors.size(), nullptr);
    s.gwritten.assign(net->tensors.size(), 0);
    for (size_t i = 1; i < net->tensors.size() && !rc; ++i) {
        rc = talloc(s, net->tensors[i].per_image * batch, &s.act[i]);
        if (!rc) rc = talloc(s, net->tensors[i].per_image * batch, &s.gact[i]);
    }
    s.tl.assign(net->layers.size(), TrainLayer());
    for (size_t i = 0; i < net->layers.size() && !rc; ++i) {
        const Layer& l = net->layers[i];
        if (!train_runs(l)) continue;
        TrainLayer& t = s.tl[i];
        t.active = true;
        const size_t mc = (size_t)batch * l.Ho * l.Wo * l.Cout;
        sz.maxC = std::max(sz.maxC, l.Cout);
        if (l.kind == LK_POOL) continue;
        if (l.kind == LK_L2NORM) {
            t.g_gamma = s.poff[l.p_gamma];
            sz.max_out = std::max(sz.max_out, mc);
            continue;
        }
        t.g_kernel = s.poff[l.p_kernel];
        if (l.p_bias >= 0) t.g_bias = s.poff[l.p_bias];
        if (l.p_kernel2 >= 0) { t.g_kernel2 = s.poff[l.p_kernel2]; t.g_bias2 = s.poff[l.p_bias2]; }
        if (l.p_bn >= 0) {
            t.g_gamma = s.poff[l.p_bn];
            t.g_beta = s.poff[l.p_bn + 1];
            rc = talloc(s, mc, &t.pre);
            if (!rc) rc = talloc(s, l.Cout, &t.mean);
            if (!rc) rc = talloc(s, l.Cout, &t.var);
            if (!rc) rc = talloc(s, l.Cout, &t.istd);
            if (!rc) rc = talloc(s, l.Cout, &t.fscale);
            if (!rc) rc = talloc(s, l.Cout, &t.fshift);
            ++s.fold_jobs_cap;
        }
        if (l.kind != LK_CONV) {
            sz.max_out = std::max(sz.max_out, mc);
            continue;
        }
        SSD_UNSUPPORTED_IF(l.stride > 2 || (l.stride == 2 && l.dil != 1), "train: unsupported conv geometry in %s", l.name.c_str());
        if (!rc) rc = talloc(s, conv_packed_floats(l.kh * l.kw * l.Cin, l.Cout), &t.wfwd);
        t.cpad = l.head_kind ? round_up(l.Cout, 32) : l.Cout;
        sz.max_out = std::max(sz.max_out, (size_t)batch * l.Ho * l.Wo * t.cpad);
        if (l.in == 0) continue;        // the image needs no gradient
        if (!rc) rc = talloc(s, conv_packed_floats(l.kh * l.kw * t.cpad, l.Cin), &t.wbwd);
        if (l.stride == 2) sz.max_dz = std::max(sz.max_dz, (size_t)batch * ((l.Ho - 1) * 2 + 1) * ((l.Wo - 1) * 2 + 1) * l.Cout);
    }
    return rc;
}

// one PackJob per forward / backward-data weight matrix (the parameters will live at flat + poff)
static int begin_pack_jobs(const ssd_net* net, ssd_train_state& s, std::vector<PackJob>& jobs) {
    for (size_t i = 0; i < net->layers.size(); ++i) {
        const Layer& l = net->layers[i];
        const TrainLayer& t = s.tl[i];
        if (!t.active || l.kind != LK_CONV) continue;
        PackJob j{};
        j.bf16 = net->precision;
        j.w = s.flat + s.poff[l.p_kernel];
        j.w2 = l.p_kernel2 >= 0 ? s.flat + s.poff[l.p_kernel2] : nullptr;
        j.K = l.kh * l.kw * l.Cin;
        j.Cout = l.Cout;
        j.Cout1 = l.p_kernel2 >= 0 ? l.Cout1 : l.Cout;
        j.kh = l.kh; j.kw = l.kw; j.Ci = l.Cin; j.CoPad = t.cpad;
        j.mode = 0; j.dst = t.wfwd; j.Kpad = conv_kpad(j.K); j.Npad = conv_npad(l.Cout);
        jobs.push_back(j);
        if (t.wbwd) {
            j.mode = 1; j.dst = t.wbwd; j.Kpad = conv_kpad(l.kh * l.kw * t.cpad); j.Npad = conv_npad(l.Cin);
            jobs.push_back(j);
        }
    }
    for (const PackJob& j : jobs)
        SSD_UNSUPPORTED_IF((long)j.Npad * j.Kpad > 0x7fffffffL, "train: a packed weight matrix of %d x %d exceeds 32-bit indexing", j.Npad, j.Kpad);
    s.n_pack_jobs = (int)jobs.size();
    s.precision = net->precision;
    return jobs.empty() ? SSD_OK : talloc(s, (jobs.size() * sizeof(PackJob) + 3) / 4, &s.pack_jobs);
}

// the dY ping-pong, the side stream of the weight gradients with its events, and the scratch of the backward and the loss
static int begin_streams_scratch(const ssd_net* net, ssd_train_state& s, const TrainSizes& sz) {
    int rc = talloc(s, sz.max_out, &s.dy_buf[0]);
    if (!rc) rc = talloc(s, sz.max_out, &s.dy_buf[1]);
    if (rc) return rc;
    if (train_env().wgrad_stream) {
        hipEvent_t* const evs[] = {&s.ev_dy, &s.ev_wdone[0], &s.ev_wdone[1], &s.ev_wall, &s.ev_main_pos};
        bool ok = hipStreamCreateWithFlags(&s.wstream, hipStreamNonBlocking) == hipSuccess;
        for (hipEvent_t* e : evs) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            set_error("ssd_net_train_begin: side stream / events for the weight gradients could not be created");
            return SSD_E_HIP;
        }
    }
    const size_t BN = (size_t)s.batch * net->num_priors;
    rc = talloc(s, sz.max_dz, &s.scratch_dz);
    if (!rc) rc = talloc(s, sz.maxC, &s.dgamma_tmp);
    if (!rc) rc = talloc(s, sz.maxC, &s.dbeta_tmp);
    if (!rc) rc = talloc(s, BN * 4, &s.deltas);
    if (!rc) rc = talloc(s, BN * net->L, &s.probs);
    if (!rc) rc = talloc(s, BN * 4, &s.gdeltas);
    if (!rc) rc = talloc(s, BN * net->L, &s.glogits);
    // refresh_plan's tables: a fold job per BatchNorm layer, and the optimizer's
    if (!rc) rc = talloc(s, ((size_t)s.fold_jobs_cap * sizeof(FoldJob) + 3) / 4, &s.fold_jobs);
    if (!rc) rc = opt_alloc_tables(net, s);
    if (rc) return rc;
    // any loss may be chosen per step: the largest of the workspaces (the IoU localisation term runs behind the
    // confidence term on the same stream and takes the workspace over)
    s.loss_ws_bytes = std::max({ssd_loss_workspace_bytes(s.batch, net->num_priors),
                                ssd_focal_loss_workspace_bytes(s.batch, net->num_priors, net->L),
                                ssd_iou_loc_loss_workspace_bytes(s.batch, net->num_priors)});
    if (hipMalloc(&s.loss_ws, s.loss_ws_bytes) != hipSuccess) {
        set_error("ssd_net_train_begin: loss workspace allocation failed");
        return SSD_E_HIP;
    }
    return SSD_OK;
}

// Every allocation succeeded: adopt the optimiser state of `net`'s previous plan (a re-plan for a larger batch keeps it) and
// move the parameters into the flat vector.  Nothing of the net is touched before the last copy has succeeded.
static int begin_adopt(ssd_net* net, ssd_train_state* s, const std::vector<PackJob>& jobs) {
    ssd_train_state* old = net->train;
    bool copy_failed = false;
    if (old) {
        copy_failed |= hipMemcpy(s->m, old->m, s->P * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess;
        copy_failed |= hipMemcpy(s->v, old->v, s->P * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess;
        s->step = old->step;
        s->opt_kind = old->opt_kind;
    } else {
        copy_failed |= hipMemset(s->m, 0, s->P * sizeof(float)) != hipSuccess;
        copy_failed |= hipMemset(s->v, 0, s->P * sizeof(float)) != hipSuccess;
    }
    for (size_t i = 0; i < net->params.size() && !copy_failed; ++i)
        if (s->poff[i] >= 0)
            copy_failed |= hipMemcpy(s->flat + s->poff[i], net->params[i].dev, net->params[i].count * sizeof(float),
                                     hipMemcpyDeviceToDevice) != hipSuccess;
    if (s->n_pack_jobs)
        copy_failed |= hipMemcpy(s->pack_jobs, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice) != hipSuccess;
    if (copy_failed) {
        set_error("ssd_net_train_begin: device copy failed");
        return SSD_E_HIP;
    }
    for (size_t i = 0; i < net->params.size(); ++i) {
        Param& p = net->params[i];
        if (s->poff[i] < 0) continue;
        if (!p.in_flat) (void)hipFree(p.dev);
        p.dev = s->flat + s->poff[i];
        p.in_flat = true;
    }
    if (old) ssd_train_state_free(old);
    net->train = s;
    net->finalized = false;          // derived inference weights must be rebuilt from the (moved) parameters
    net->drop_graphs();
    return SSD_OK;
}

}  // namespace ssd

extern "C" {

size_t ssd_net_trainable_floats(const ssd_net* net) {
    if (!net) return 0;
    size_t n = 0;
    for (const auto& p : net->params)
        if (trainable(p.name)) n += p.count;
    return n;
}

long ssd_net_trainable_offset(const ssd_net* net, const char* name) {
    if (!net || !name) return -1;
    long off = 0;
    for (const auto& p : net->params) {
        if (!trainable(p.name)) continue;
        if (p.name == name) return off;
        off += (long)p.count;
    }
    return -1;
}

int ssd_net_train_begin(ssd_net* net, int batch) {
    SSD_CHECK_ARG(net && batch >= 1, "ssd_net_train_begin: bad arguments");
    for (const auto& p : net->params)
        if (!p.set) {
            set_error("ssd_net_train_begin: parameter '%s' was never set", p.name.c_str());
            return SSD_E_STATE;
        }
    if (net->train && net->train->batch >= batch) return SSD_OK;
    auto* s = new ssd_train_state();
    s->batch = batch;
    TrainSizes sz;
    std::vector<PackJob> jobs;
    int rc = begin_flat(net, *s);
    if (!rc) rc = begin_plan_layers(net, *s, sz);
    if (!rc) rc = begin_pack_jobs(net, *s, jobs);
    if (!rc) rc = begin_streams_scratch(net, *s, sz);
    if (!rc) rc = begin_adopt(net, s, jobs);
    if (rc) ssd_train_state_free(s);        // nothing of the net was touched: the previous state (if any) stays valid
    return rc;
}

// Training-mode forward + loss + backward.  grads_flat_dev [ssd_net_trainable_floats] receives
// d(mean_b (loc_b + conf_b)) / d(parameter) in parameter-table order (Keras layouts);
// loc_loss_dev / conf_loss_dev [B] receive the per-image loss terms.
int ssd_net_train_forward_backward(ssd_net* net, const float* image_dev, int B, const float* actual_deltas_dev,
                                   const float* actual_labels_dev, float neg_pos_ratio, float loc_loss_alpha,
                                   float* grads_flat_dev, float* loc_loss_dev, float* conf_loss_dev, void* stream) {
    ssd_loss_config loss = {};               // the zero-filled tail: SSD_LOC_HUBER, this kernel's own localisation term
    loss.kind = SSD_LOSS_HARD_NEGATIVE;
    loss.neg_pos_ratio = neg_pos_ratio;
    loss.loc_loss_alpha = loc_loss_alpha;
    loss.focal_alpha = 0.25f;
    loss.focal_gamma = 2.0f;
    return ssd_net_train_forward_backward_cfg(net, image_dev, B, actual_deltas_dev, actual_labels_dev, &loss, grads_flat_dev,
                                              loc_loss_dev, conf_loss_dev, stream);
}

size_t ssd_loss_config_bytes(void) { return sizeof(ssd_loss_config); }

// The step with the loss chosen by `loss`: ssd_loss (the reference's mining) or ssd_focal_loss, on the same buffers; with
// a loc_kind other than SSD_LOC_HUBER that kernel evaluates the confidence term alone and ssd_iou_loc_loss the other.
int ssd_net_train_forward_backward_cfg(ssd_net* net, const float* image_dev, int B, const float* actual_deltas_dev,
                                       const float* actual_labels_dev, const ssd_loss_config* loss, float* grads_flat_dev,
                                       float* loc_loss_dev, float* conf_loss_dev, void* stream) {
    SSD_CHECK_ARG(net && image_dev && actual_deltas_dev && actual_labels_dev && grads_flat_dev,
                  "ssd_net_train_forward_backward: NULL argument");
    SSD_CHECK_ARG(loss, "ssd_net_train_forward_backward_cfg: NULL loss");
    SSD_CHECK_ARG(loss->kind == SSD_LOSS_HARD_NEGATIVE || loss->kind == SSD_LOSS_FOCAL,
                  "ssd_net_train_forward_backward_cfg: unknown loss kind %d", loss->kind);
    SSD_CHECK_ARG(loss->kind != SSD_LOSS_FOCAL || (loss->focal_alpha > 0.f && loss->focal_alpha < INFINITY &&
                                                   loss->focal_gamma >= 0.f && loss->focal_gamma < INFINITY),
                  "ssd_net_train_forward_backward_cfg: focal alpha must be > 0 and gamma >= 0 (finite), got alpha=%g gamma=%g",
                  (double)loss->focal_alpha, (double)loss->focal_gamma);
    SSD_CHECK_ARG(loss->loc_kind >= SSD_LOC_HUBER && loss->loc_kind <= SSD_LOC_CIOU,
                  "ssd_net_train_forward_backward_cfg: unknown loc_kind %d", loss->loc_kind);
    const bool iou_loc = loss->loc_kind != SSD_LOC_HUBER;
    if (iou_loc) {
        SSD_CHECK_ARG(loss->priors_dev && ((uintptr_t)loss->priors_dev & 15) == 0,
                      "ssd_net_train_forward_backward_cfg: loc_kind %d needs priors (16-byte aligned)", loss->loc_kind);
        for (int k = 0; k < 4; ++k)
            SSD_CHECK_ARG(loss->variances[k] > 0.f && loss->variances[k] < INFINITY,
                          "ssd_net_train_forward_backward_cfg: variances must be > 0 and finite, got variances[%d]=%g", k,
                          (double)loss->variances[k]);
    }
    if (!net->train) { set_error("ssd_net_train_forward_backward: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    ssd_train_state& s = *net->train;
    SSD_CHECK_ARG(B >= 1 && B <= s.batch, "ssd_net_train_forward_backward: batch %d exceeds the planned %d", B, s.batch);
    if (s.precision != net->precision) {
        set_error("ssd_net_train_forward_backward: the precision option changed since ssd_net_train_begin (the weight re-pack was planned for %d): call ssd_net_train_begin again", s.precision);
        return SSD_E_STATE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int N = net->num_priors, L = net->L;
    s.act[0] = const_cast<float*>(image_dev);
    s.step_flops[0] = s.step_flops[1] = s.step_flops[2] = 0;       // whatever path returns: they hold what this call issued
    const bool side = s.wstream && (s.bucket_lo.empty() || train_env().side_buckets);
    StepCtx c{net, s, st, B, grads_flat_dev, side};
    c.next_bucket = s.bucket_lo.size();
    int rc = refresh_plan(net, s);
    if (rc) return rc;
    if (s.any_frozen) {
        // frozen ranges hold exactly 0.0f for the all-reduce and every other reader: the whole vector is cleared with one
        // memset in front of everything that writes it (the side stream's weight gradients are ordered behind it through ev_dy)
        SSD_HIP(hipMemsetAsync(grads_flat_dev, 0, s.P * sizeof(float), st));
        if (s.n_fold_jobs) {
            hipLaunchKernelGGL(bn_fold_jobs_kernel, dim3((s.fold_maxC + 255) / 256, (unsigned)s.n_fold_jobs), dim3(256), 0, st,
                               reinterpret_cast<const FoldJob*>(s.fold_jobs), kBnEps);
            SSD_LAUNCH_CHECK();
        }
    }

    // re-pack the (just updated) weights of every conv: forward and backward-data forms, one launch
    if (s.n_pack_jobs) {
        hipLaunchKernelGGL(pack_jobs_kernel, dim3(128, (unsigned)s.n_pack_jobs), dim3(256), 0, st,
                           reinterpret_cast<const PackJob*>(s.pack_jobs));
        SSD_LAUNCH_CHECK();
    }
    for (size_t i = 0; i < net->layers.size(); ++i)
        if (s.tl[i].active && (rc = train_forward_layer(c, i))) return rc;
    rc = launch_softmax(s.probs, (long)B * N, L, s.probs, st);
    if (rc) return rc;
    if (iou_loc) {
        if (loss->kind == SSD_LOSS_FOCAL)
            rc = ssd_focal_loss(nullptr, nullptr, actual_labels_dev, s.probs, B, N, L, loss->loc_loss_alpha, loss->focal_alpha,
                                loss->focal_gamma, nullptr, conf_loss_dev, nullptr, nullptr, nullptr, s.glogits,
                                1.0f / (float)B, s.loss_ws, s.loss_ws_bytes, stream);
        else
            rc = ssd_loss(nullptr, nullptr, actual_labels_dev, s.probs, B, N, L, loss->neg_pos_ratio, loss->loc_loss_alpha,
                          nullptr, conf_loss_dev, nullptr, nullptr, nullptr, s.glogits, 1.0f / (float)B, s.loss_ws,
                          s.loss_ws_bytes, stream);
        if (rc) return rc;
        rc = ssd_iou_loc_loss(loss->priors_dev, loss->variances, actual_deltas_dev, s.deltas, B, N, loss->loc_kind,
                              loss->loc_loss_alpha, loc_loss_dev, nullptr, s.gdeltas, 1.0f / (float)B, s.loss_ws,
                              s.loss_ws_bytes, stream);
    } else if (loss->kind == SSD_LOSS_FOCAL)
        rc = ssd_focal_loss(actual_deltas_dev, s.deltas, actual_labels_dev, s.probs, B, N, L, loss->loc_loss_alpha,
                            loss->focal_alpha, loss->focal_gamma, loc_loss_dev, conf_loss_dev, nullptr, nullptr, s.gdeltas,
                            s.glogits, 1.0f / (float)B, s.loss_ws, s.loss_ws_bytes, stream);
    else
        rc = ssd_loss(actual_deltas_dev, s.deltas, actual_labels_dev, s.probs, B, N, L, loss->neg_pos_ratio,
                      loss->loc_loss_alpha, loc_loss_dev, conf_loss_dev, nullptr, nullptr, s.gdeltas, s.glogits,
                      1.0f / (float)B, s.loss_ws, s.loss_ws_bytes, stream);
    if (rc) return rc;

    // backward, last layer first
    std::fill(s.gwritten.begin(), s.gwritten.end(), 0);
    s.wpending[0] = s.wpending[1] = false;
    for (int i = (int)net->layers.size() - 1; i >= 0; --i) {
        const Layer& l = net->layers[i];
        const TrainLayer& t = s.tl[i];
        if (!t.active) continue;
        // layers > i are done: what no layer <= i owns is final
        if (!s.pending_hi.empty() && (rc = c.mark_ready(s.pending_hi[i]))) return rc;
        const int plan = s.plan[i];
        if (plan & SSD_PLAN_SKIP) continue;             // nothing trainable here or upstream: its (zero) ranges are final already
        float* const dyb = l.kind == LK_POOL ? nullptr : c.acquire_dy();      // this layer's dY / scratch buffer
        // (a head conv takes its gradient from the loss; by the plan every other layer that is not skipped has a consumer
        // that hands it one)
        if (!l.head_kind && !s.gwritten[l.out]) {
            set_error("train: no gradient reached tensor '%s'", net->tensors[l.out].name.c_str());
            return SSD_E_STATE;
        }
        if (l.kind == LK_POOL || l.kind == LK_L2NORM) {
            rc = l.kind == LK_POOL ? bwd_pool(c, l) : bwd_l2norm(c, l, t, dyb, plan);
            if (rc) return rc;
            continue;
        }
        const float* dY = nullptr;       // gradient w.r.t. the conv / depthwise output, dense [M][ldy]
        int ldy = l.Cout;
        if (l.head_kind) rc = bwd_head_dy(c, l, t, dyb, &dY, &ldy, plan);
        else if (l.p_bn >= 0) rc = bwd_bn_dy(c, l, t, dyb, &dY, plan);
        else rc = bwd_bias_act_dy(c, l, t, dyb, &dY, plan);
        if (rc) return rc;
        if (l.kind == LK_DW) {
            if (plan & (SSD_PLAN_WGRAD | SSD_PLAN_DGRAD)) rc = bwd_depthwise(c, l, t, dY, plan);
        } else {
            rc = bwd_dense_wgrad(c, l, t, dY, ldy, dyb, plan);
            if (!rc && t.wbwd && (plan & SSD_PLAN_DGRAD)) rc = bwd_dense_dgrad(c, l, t, dY, ldy);
        }
        if (rc) return rc;
    }
    rc = c.join_wgrads();           // the caller's stream sees the complete gradient vector
    if (rc) return rc;
    return c.mark_ready(0);
}

// Gradient buckets for the data-parallel exchange ("prefer ... overlapped with backward"):
// bucket k covers the flat offsets [lo[k], lo[k + 1]) (lo ascending, lo[0] == 0, the last bucket ends at
// ssd_net_trainable_floats).  The backward walks the layers last to first, i.e. it finishes the gradient vector
// from its END; ssd_net_train_forward_backward records an event per bucket at the moment every layer owning a
// parameter at or above lo[k] has been passed, and ssd_net_train_wait_bucket makes another stream (the one the
// RCCL all-reduce of that bucket is issued on) wait for exactly that point -- the exchange of the head / extras
// gradients then runs beside the backward of the backbone.  n == 0 clears the plan.
int ssd_net_train_set_buckets(ssd_net* net, int n, const long* lo) {
    SSD_CHECK_ARG(net && n >= 0 && (n == 0 || lo), "ssd_net_train_set_buckets: bad arguments");
    if (!net->train) { set_error("ssd_net_train_set_buckets: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    ssd_train_state& s = *net->train;
    for (int k = 0; k < n; ++k)
        SSD_CHECK_ARG((k == 0 ? lo[0] == 0 : lo[k] > lo[k - 1]) && lo[k] < (long)s.P, "ssd_net_train_set_buckets: starts must ascend from 0 below %zu", s.P);
    for (auto e : s.bucket_ev)
        if (e) (void)hipEventDestroy(e);
    s.bucket_ev.clear();
    s.bucket_lo.assign(lo, lo + n);
    s.pending_hi.clear();
    if (n == 0) return SSD_OK;
    s.bucket_ev.resize(n, nullptr);
    for (int k = 0; k < n; ++k) SSD_HIP(hipEventCreateWithFlags(&s.bucket_ev[k], hipEventDisableTiming));
    // pending_hi[i] = end of the highest trainable parameter owned by an active layer j <= i
    s.pending_hi.assign(net->layers.size(), 0);
    long run = 0;
    for (size_t i = 0; i < net->layers.size(); ++i) {
        const Layer& l = net->layers[i];
        if (s.tl[i].active)
            for (int q : {l.p_kernel, l.p_bias, l.p_kernel2, l.p_bias2, l.p_bn, l.p_bn >= 0 ? l.p_bn + 1 : -1, l.p_gamma})
                if (q >= 0 && q < (int)s.poff.size() && s.poff[q] >= 0) run = std::max(run, s.poff[q] + (long)net->params[q].count);
        s.pending_hi[i] = run;
    }
    return SSD_OK;
}

int ssd_net_train_wait_bucket(ssd_net* net, int k, void* stream) {
    SSD_CHECK_ARG(net && net->train && k >= 0 && k < (int)net->train->bucket_ev.size(), "ssd_net_train_wait_bucket: bad bucket %d", k);
    SSD_HIP(hipStreamWaitEvent((hipStream_t)stream, net->train->bucket_ev[k], 0));
    return SSD_OK;
}

int ssd_net_set_trainable(ssd_net* net, const char* keras_layer, int trainable_flag) {
    SSD_CHECK_ARG(net && keras_layer, "ssd_net_set_trainable: NULL argument");
    SSD_CHECK_ARG(known_keras_layer(net, keras_layer), "ssd_net_set_trainable: '%s' is no Keras layer with trainable variables of this net", keras_layer);
    const bool changed = trainable_flag ? net->frozen.erase(keras_layer) != 0 : net->frozen.insert(keras_layer).second;
    if (changed) ++net->trainable_rev;
    return SSD_OK;
}

int ssd_net_get_trainable(const ssd_net* net, const char* keras_layer) {
    SSD_CHECK_ARG(net && keras_layer, "ssd_net_get_trainable: NULL argument");
    SSD_CHECK_ARG(known_keras_layer(net, keras_layer), "ssd_net_get_trainable: '%s' is no Keras layer with trainable variables of this net", keras_layer);
    return net->frozen.count(keras_layer) ? 0 : 1;
}

int ssd_net_train_plan(const ssd_net* net, int layer, int* flags) {
    SSD_CHECK_ARG(net && flags, "ssd_net_train_plan: NULL argument");
    SSD_CHECK_ARG(layer >= 0 && layer < (int)net->layers.size(), "ssd_net_train_plan: layer %d is outside 0..%d", layer, (int)net->layers.size() - 1);
    *flags = backward_plan(net)[layer];
    return SSD_OK;
}

int ssd_net_train_matrix_flops(const ssd_net* net, double* out3) {
    SSD_CHECK_ARG(net && out3, "ssd_net_train_matrix_flops: NULL argument");
    if (!net->train) { set_error("ssd_net_train_matrix_flops: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    for (int i = 0; i < 3; ++i) out3[i] = net->train->step_flops[i];
    return SSD_OK;
}

// Debug / parity hook: copy a buffer of the LAST ssd_net_train_forward_backward (at batch B) to the
// host.  what = "probs" | "deltas" | "grad_logits" | "grad_deltas" | "<tensor name>" (training
// activation) | "grad:<tensor name>" | "pre:<layer name>" (conv output before BatchNorm) |
// "mean:<layer>" | "var:<layer>".  Returns the element count (host_out may be NULL to query).
long ssd_net_train_fetch(ssd_net* net, const char* what, int B, float* host_out, size_t cap) {
    if (!net || !what || !net->train || B < 1 || B > net->train->batch) {
        set_error("ssd_net_train_fetch: bad arguments / no training state");
        return SSD_E_INVALID;
    }
    ssd_train_state& s = *net->train;
    const std::string w(what);
    const float* src = nullptr;
    size_t n = 0;
    const size_t N = net->num_priors;
    if (w == "probs") { src = s.probs; n = (size_t)B * N * net->L; }
    else if (w == "deltas") { src = s.deltas; n = (size_t)B * N * 4; }
    else if (w == "grad_logits") { src = s.glogits; n = (size_t)B * N * net->L; }
    else if (w == "grad_deltas") { src = s.gdeltas; n = (size_t)B * N * 4; }
    else if (w.rfind("pre:", 0) == 0 || w.rfind("mean:", 0) == 0 || w.rfind("var:", 0) == 0) {
        const std::string name = w.substr(w.find(':') + 1);
        for (size_t i = 0; i < net->layers.size(); ++i)
            if (net->layers[i].name == name && s.tl[i].active && s.tl[i].pre) {
                const Layer& l = net->layers[i];
                if (w[0] == 'p') { src = s.tl[i].pre; n = (size_t)B * l.Ho * l.Wo * l.Cout; }
                else { src = w[0] == 'm' ? s.tl[i].mean : s.tl[i].var; n = l.Cout; }
            }
    } else {
        const bool grad = w.rfind("grad:", 0) == 0;
        auto it = net->tensor_index.find(grad ? w.substr(5) : w);
        if (it != net->tensor_index.end() && it->second > 0) {
            src = grad ? s.gact[it->second] : s.act[it->second];
            n = net->tensors[it->second].per_image * (size_t)B;
        }
    }
    if (!src) {
        set_error("ssd_net_train_fetch: unknown buffer '%s'", what);
        return SSD_E_INVALID;
    }
    if (!host_out) return (long)n;
    if (cap < n) { set_error("ssd_net_train_fetch: buffer too small"); return SSD_E_INVALID; }
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_out, src, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("ssd_net_train_fetch: copy failed");
        return SSD_E_HIP;
    }
    return (long)n;
}

// ---------------------------------------------------------------------- test / bench hooks of the backward kernels
int ssd_conv_wgrad_num_configs(void) { return (int)(sizeof(kWgrad) / sizeof(kWgrad[0])); }

static bool wgrad_desc_layer(const ssd_conv_desc* d, int N, Layer* out) {
    if (!d || d->B < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || N < 1 || d->kh < 1 || d->kw < 1 || d->stride < 1 ||
        d->dilation < 1 || d->pad_t < 0 || d->pad_l < 0 || d->pad_b < 0 || d->pad_r < 0)
        return false;
    Layer l;
    l.kind = LK_CONV;
    l.H = d->H; l.W = d->W; l.Cin = d->Cin; l.Cout = N;
    l.kh = d->kh; l.kw = d->kw; l.stride = d->stride; l.dil = d->dilation;
    l.pt = d->pad_t; l.pb = d->pad_b; l.pl = d->pad_l; l.pr = d->pad_r;
    l.Ho = ssd_conv_out_size(d->H, d->kh, d->stride, d->dilation, d->pad_t, d->pad_b);
    l.Wo = ssd_conv_out_size(d->W, d->kw, d->stride, d->dilation, d->pad_l, d->pad_r);
    if (l.Ho < 1 || l.Wo < 1) return false;
    *out = l;
    return true;
}

size_t ssd_conv_wgrad_workspace_floats(const ssd_conv_desc* d, int N) {
    Layer l;
    if (!wgrad_desc_layer(d, N, &l)) return 0;
    size_t need = 0;
    for (const auto& c : kWgrad) {           // the chunk count follows the tile count: the largest over the table
        long rpc = 0;
        const size_t f = (size_t)wgrad_chunks(l, d->B, N, &c, &rpc, nullptr) * l.kh * l.kw * l.Cin * N;
        need = f > need ? f : need;
    }
    return need;
}

int ssd_conv2d_wgrad_ex(const ssd_conv_desc* d, const float* x_dev, const float* g_dev, int ldg, int N, int config,
                        float* dW_dev, float* workspace_dev, size_t workspace_floats, void* stream) {
    Layer l;
    SSD_CHECK_ARG(wgrad_desc_layer(d, N, &l), "ssd_conv2d_wgrad_ex: bad geometry");
    SSD_CHECK_ARG(x_dev && g_dev && dW_dev && workspace_dev, "ssd_conv2d_wgrad_ex: NULL argument");
    SSD_CHECK_ARG(ldg >= N, "ssd_conv2d_wgrad_ex: ldg %d is below N %d", ldg, N);
    SSD_CHECK_ARG(config >= -1 && config < ssd_conv_wgrad_num_configs(), "ssd_conv2d_wgrad_ex: config %d is outside -1..%d",
                  config, ssd_conv_wgrad_num_configs() - 1);
    const WgradCfg* cfg = config < 0 ? wgrad_heuristic(l, N) : &kWgrad[config];
    return wgrad_with(l, d->B, x_dev, g_dev, ldg, N, dW_dev, (hipStream_t)stream, cfg, workspace_dev, workspace_floats);
}

int ssd_dwconv3x3_backward(const float* x_dev, const float* g_dev, const float* w_dev, int B, int H, int W, int C, int stride,
                           int pad_t, int pad_l, int accumulate, float* dx_dev, float* dw_dev, float* workspace_dev,
                           size_t workspace_floats, void* stream) {
    SSD_CHECK_ARG(x_dev && g_dev && w_dev && dx_dev && dw_dev && workspace_dev, "ssd_dwconv3x3_backward: NULL argument");
    SSD_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "ssd_dwconv3x3_backward: bad shape (C = %d must be a multiple of 4)", C);
    SSD_CHECK_ARG((stride == 1 || stride == 2) && (pad_t == 0 || pad_t == 1) && (pad_l == 0 || pad_l == 1),
                  "ssd_dwconv3x3_backward: stride %d / pads (%d, %d) unsupported", stride, pad_t, pad_l);
    SSD_CHECK_ARG(((((uintptr_t)x_dev | (uintptr_t)g_dev | (uintptr_t)w_dev | (uintptr_t)dx_dev) & 15) == 0),
                  "ssd_dwconv3x3_backward: tensors must be 16-byte aligned");
    DwBwdParams dp{};
    dp.x = x_dev; dp.g = g_dev; dp.w = w_dev; dp.dx = dx_dev;
    dp.B = B; dp.H = H; dp.W = W; dp.C = C;
    dp.Ho = ssd_conv_out_size(H, 3, stride, 1, pad_t, 1);
    dp.Wo = ssd_conv_out_size(W, 3, stride, 1, pad_l, 1);
    SSD_CHECK_ARG(dp.Ho >= 1 && dp.Wo >= 1, "ssd_dwconv3x3_backward: empty output");
    dp.stride = stride; dp.pad_t = pad_t; dp.pad_l = pad_l;
    dp.M = (long)B * dp.Ho * dp.Wo;
    dp.accumulate = accumulate ? 1 : 0;
    const long chunks = dw_bwd_chunks(dp);
    SSD_CHECK_ARG((size_t)chunks * 9 * C <= workspace_floats, "ssd_dwconv3x3_backward: the workspace holds %zu floats, %zu are needed",
                  workspace_floats, (size_t)chunks * 9 * C);
    dp.partial = workspace_dev;
    return dw_bwd_launch(dp, chunks, dw_dev, (hipStream_t)stream);
}

}  // extern "C"
