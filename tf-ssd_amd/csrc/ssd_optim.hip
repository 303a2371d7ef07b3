// The optimizer of the training step: Adam (TF training_ops.ApplyAdam form) and Keras SGD with clipnorm, clipvalue and
// global_clipnorm (include/ssd_hip.h has the arithmetic), and the regularisation loss.  ONE update kernel walks ONE table of
// the trainable ranges of the flat parameter vector; every setting, frozen layers or not, is an instantiation of it.
// Shares nothing with the forward / backward step (ssd_train.hip) except ssd_train_state (ssd_train.h).
#include <algorithm>
#include <cmath>

#include "ssd_train.h"

using namespace ssd;

namespace ssd {

// sh[0] = sum of the 256 lanes' values through a fixed tree (the same additions in the same order whatever the grid)
__device__ __forceinline__ void block_tree_sum(float* sh, const float x) {
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ regularisation loss
// partial[blockIdx.x] = sum of w^2 over this block's grid-stride slice (fixed slices, fixed in-block tree:
// deterministic); reg_finalize sums the partials in order and applies the l2 factor
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ w, const long n, float* __restrict__ partial) {
    __shared__ float sh[256];
    float s = 0.f;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) s += w[e] * w[e];
    block_tree_sum(sh, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void reg_finalize_kernel(const float* __restrict__ partial, const int n, const float l2, float* out) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)partial[i];
    *out = (float)(s * (double)l2);
}

// ------------------------------------------------------------------ the update and the Keras gradient clips
// The table covers the trainable part of the flat vector in segments of at most kOptSeg elements; a workgroup takes whole
// segments, so var / m / v / grad of a frozen range are not even read, and one launch serves however many ranges there
// are (freezing every BatchNorm leaves ~100 disjoint ones).  A segment never crosses a Keras variable (an entry of the
// parameter table) and names it, so tf.clip_by_norm has its per-variable sum and the update its per-variable scale.
// Streaming kernels: per element SGD without momentum moves 12 B (grad in, var in and out), with momentum 20 B, Adam
// 28 B; the norm pass reads grad once more (4 B).  A segment starts at its variable's offset, which is not always a
// multiple of 4 floats (the 126 label biases of a 21-label head push what follows 8 bytes off): the head of a segment
// up to the next 16-byte boundary and its tail go element by element, the body in 16-byte accesses.
constexpr long kOptSeg = 4096;
// The update kernel puts kOptSplit workgroups on a segment, a 16-byte access per thread (measured: 1, 2, 4, 8; 8 loses).
// With one, MobileNetV2's 2216 workgroups are a round and a quarter of what the device holds at once and move in step, so
// Adam's square root and division do not hide behind the loads.  The split is a kernel argument on purpose: with a constant stride the compiler
// unrolls the body loop four times, every load of a segment is issued before any arithmetic, and Adam takes 47 us on
// MobileNetV2 where this form takes 37 (the flat sweep this kernel replaced: 34).
constexpr int kOptSplit = 4;
struct OptSeg {
    long lo;
    int n, var;      // var: the variable's index among the trainable parameters (table order)
};
struct OptVar {
    int seg0, nseg;  // the variable's segments in the table (nseg 0: frozen)
};
enum { kClipNorm = 1, kClipGlobal = 2, kClipValue = 4 };
constexpr int kOptMaxVars = 2048;
struct OptArgs {
    float lr;        // Adam: alpha = lr * sqrt(1 - b2^t) / (1 - b1^t)
    float b1, b2, eps, momentum, grad_scale, clipnorm, clipvalue;
};

// cs: clipnorm max(norm, c) of the element's variable; global_clipnorm the one scale c * min(1 / gn, 1 / c)
template <int CLIP>
__device__ __forceinline__ float opt_clip(const float graw, const OptArgs& a, const float cs) {
    float g = graw * a.grad_scale;
    if (CLIP & kClipNorm) g = (g * a.clipnorm) / cs;
    if (CLIP & kClipGlobal) g *= cs;
    if (CLIP & kClipValue) g = fminf(fmaxf(g, -a.clipvalue), a.clipvalue);
    return g;
}
// Adam: m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); var -= alpha * m / (sqrt(v) + eps); g already holds the l2
// regulariser's gradient (bwd_dense_wgrad adds it behind the layer's weight gradient).  The only Adam there is, and its
// roundings are spelled out: nothing is contracted, fmaf stands where one rounding is meant.  Left to the compiler, the same
// expression came out fused in one loop of a kernel and unfused in the next, so an element's bits depended on the table.
template <int OPT, bool NESTEROV, bool ACC>
__device__ __forceinline__ void opt_apply(float& var, float& m, float& v, const float g, const OptArgs& a) {
    if (OPT == SSD_OPT_ADAM) {
#pragma clang fp contract(off)
        const float mm = m + (g - m) * (1.0f - a.b1);
        const float vv = fmaf(1.0f - a.b2, fmaf(g, g, -v), v);
        m = mm;
        v = vv;
        var -= a.lr * mm / (sqrtf(vv) + a.eps);
    } else if (ACC) {
        const float acc = a.momentum * m - a.lr * g;
        m = acc;
        var += NESTEROV ? a.momentum * acc - a.lr * g : acc;
    } else {
        var -= a.lr * g;
    }
}
// the three pieces of a segment: [0, head) and [head + 4 * nv, n) scalar, nv float4 between them (vec == 0: all scalar)
__device__ __forceinline__ void opt_split(const OptSeg& sg, const int vec, int& head, int& nv) {
    head = vec ? min(sg.n, (int)((4 - (sg.lo & 3)) & 3)) : sg.n;
    nv = (sg.n - head) >> 2;
}

template <int OPT, bool NESTEROV, bool ACC, int CLIP>
__global__ __launch_bounds__(256) void opt_update_kernel(float* __restrict__ var, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ grad, const OptSeg* __restrict__ segs,
                                                        const int nseg, const float* __restrict__ cscale, const OptArgs a,
                                                        const int vec, const int split) {
    constexpr bool kM = OPT == SSD_OPT_ADAM || ACC, kV = OPT == SSD_OPT_ADAM;
    for (int w = blockIdx.x; w < nseg * split; w += gridDim.x) {
        const OptSeg sg = segs[w / split];
        const int part = w % split;
        const float cs = (CLIP & (kClipNorm | kClipGlobal)) ? cscale[sg.var] : 1.0f;
        int head, nv;
        opt_split(sg, vec, head, nv);
        const auto one = [&](const long e) {
            float w = var[e], mm = kM ? m[e] : 0.f, vv = kV ? v[e] : 0.f;
            opt_apply<OPT, NESTEROV, ACC>(w, mm, vv, opt_clip<CLIP>(grad[e], a, cs), a);
            var[e] = w;
            if (kM) m[e] = mm;
            if (kV) v[e] = vv;
        };
        if (part == 0)
            for (int i = threadIdx.x; i < head; i += 256) one(sg.lo + i);
        const long body = sg.lo + head;
        for (int i = part * 256 + threadIdx.x; i < nv; i += 256 * split) {
            const long e = body + 4L * i;
            const float4 g4 = *reinterpret_cast<const float4*>(grad + e);
            float4 w4 = *reinterpret_cast<const float4*>(var + e);
            float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
            if (kM) m4 = *reinterpret_cast<const float4*>(m + e);
            if (kV) v4 = *reinterpret_cast<const float4*>(v + e);
            opt_apply<OPT, NESTEROV, ACC>(w4.x, m4.x, v4.x, opt_clip<CLIP>(g4.x, a, cs), a);
            opt_apply<OPT, NESTEROV, ACC>(w4.y, m4.y, v4.y, opt_clip<CLIP>(g4.y, a, cs), a);
            opt_apply<OPT, NESTEROV, ACC>(w4.z, m4.z, v4.z, opt_clip<CLIP>(g4.z, a, cs), a);
            opt_apply<OPT, NESTEROV, ACC>(w4.w, m4.w, v4.w, opt_clip<CLIP>(g4.w, a, cs), a);
            *reinterpret_cast<float4*>(var + e) = w4;
            if (kM) *reinterpret_cast<float4*>(m + e) = m4;
            if (kV) *reinterpret_cast<float4*>(v + e) = v4;
        }
        if (part == split - 1)
            for (int i = head + 4 * nv + threadIdx.x; i < sg.n; i += 256) one(sg.lo + i);
    }
}

// Norm pass, launch 1: partial[s] = sum of (grad * grad_scale)^2 over segment s.  A thread adds its elements in index
// order, the 256 sums go through a fixed tree; which workgroup takes a segment changes nothing: no atomics, the same
// bits at every grid size.
__global__ __launch_bounds__(256) void opt_sumsq_kernel(const float* __restrict__ grad, const OptSeg* __restrict__ segs, const int nseg,
                                                       const float grad_scale, float* __restrict__ partial, const int vec) {
    __shared__ float sh[256];
    for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
        const OptSeg sg = segs[s];
        int head, nv;
        opt_split(sg, vec, head, nv);
        float acc = 0.f;
        const auto sq = [&](const float x) { const float g = x * grad_scale; acc += g * g; };
        for (int i = threadIdx.x; i < head; i += 256) sq(grad[sg.lo + i]);
        const long body = sg.lo + head;
        for (int i = threadIdx.x; i < nv; i += 256) {
            const float4 g4 = *reinterpret_cast<const float4*>(grad + body + 4L * i);
            sq(g4.x); sq(g4.y); sq(g4.z); sq(g4.w);
        }
        for (int i = head + 4 * nv + threadIdx.x; i < sg.n; i += 256) sq(grad[sg.lo + i]);
        block_tree_sum(sh, acc);
        if (threadIdx.x == 0) partial[s] = sh[0];
        __syncthreads();
    }
}
// Norm pass, launch 2 (one workgroup): every variable's partials, which lie in table order, summed in double -- lane l of
// a wavefront takes partials l, l + 64, ... in that order, the 64 sums go through a fixed butterfly -- then what the update
// reads per variable: clipnorm max(norm, c) with norm = s > 0 ? sqrt(s) : s (tf.clip_by_norm: an all-zero gradient
// divides by c and stays zero), global_clipnorm the one scale c * min(1 / gn, 1 / c) over the sum of every s.
__global__ __launch_bounds__(1024) void opt_norm_finish_kernel(const float* __restrict__ partial, const OptVar* __restrict__ vars,
                                                              const int nvars, float* __restrict__ cscale, const float clipnorm,
                                                              const float global_clipnorm) {
    __shared__ double ssum[kOptMaxVars];
    __shared__ double total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = wave; q < nvars; q += 16) {
        const OptVar r = vars[q];
        double s = 0.0;
        for (int i = lane; i < r.nseg; i += 64) s += (double)partial[r.seg0 + i];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) ssum[q] = s;
    }
    __syncthreads();
    if (global_clipnorm > 0.f) {
        if (wave == 0) {
            double t = 0.0;
            for (int q = lane; q < nvars; q += 64) t += ssum[q];
            for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
            if (lane == 0) total = t;
        }
        __syncthreads();
        const float gn = (float)sqrt(total);
        const float sc = global_clipnorm * fminf(1.0f / gn, 1.0f / global_clipnorm);
        for (int q = threadIdx.x; q < nvars; q += 1024) cscale[q] = sc;
    } else {
        for (int q = threadIdx.x; q < nvars; q += 1024) {
            const double s = ssum[q];
            cscale[q] = fmaxf(s > 0.0 ? (float)sqrt(s) : 0.f, clipnorm);
        }
    }
}

// ------------------------------------------------------------------ the table
// Room for every trainable parameter cut into segments, a variable entry each, and the norm pass's scratch.
int opt_alloc_tables(const ssd_net* net, ssd_train_state& s) {
    for (size_t q = 0; q < net->params.size(); ++q)
        if (s.poff[q] >= 0) {
            s.opt_segs_cap += (int)((net->params[q].count + kOptSeg - 1) / kOptSeg);
            ++s.n_opt_vars;
        }
    int rc = talloc(s, ((size_t)s.opt_segs_cap * sizeof(OptSeg) + 3) / 4, &s.opt_segs);
    if (!rc) rc = talloc(s, ((size_t)s.n_opt_vars * sizeof(OptVar) + 3) / 4, &s.opt_vars);
    if (!rc) rc = talloc(s, (size_t)s.opt_segs_cap, &s.opt_partial);
    if (!rc) rc = talloc(s, (size_t)s.n_opt_vars, &s.opt_norm);
    return rc;
}

// The table of the net's current trainable flags, made per Keras variable whether anything is frozen or not (clipped and
// frozen runs share one reduction order).  Blocking copies: the caller has waited for the device.
int opt_refresh_tables(const ssd_net* net, ssd_train_state& s) {
    std::vector<OptSeg> segs;
    std::vector<OptVar> vars;
    for (size_t q = 0; q < net->params.size(); ++q) {
        if (s.poff[q] < 0) continue;
        OptVar ov{(int)segs.size(), 0};
        if (!param_frozen(net, (int)q))
            for (long b = 0; b < (long)net->params[q].count; b += kOptSeg, ++ov.nseg)
                segs.push_back(OptSeg{s.poff[q] + b, (int)std::min(kOptSeg, (long)net->params[q].count - b), (int)vars.size()});
        vars.push_back(ov);
    }
    SSD_CHECK_ARG((int)segs.size() <= s.opt_segs_cap && (int)vars.size() == s.n_opt_vars,
                  "train: the optimizer's table (%zu segments, %zu variables) exceeds its plan", segs.size(), vars.size());
    if (!segs.empty()) SSD_HIP(hipMemcpy(s.opt_segs, segs.data(), segs.size() * sizeof(OptSeg), hipMemcpyHostToDevice));
    if (!vars.empty()) SSD_HIP(hipMemcpy(s.opt_vars, vars.data(), vars.size() * sizeof(OptVar), hipMemcpyHostToDevice));
    s.n_opt_segs = (int)segs.size();
    return SSD_OK;
}

// opt_update_kernel's instantiation for an optimizer and a clip mask (norm and global norm exclude each other)
template <int OPT, bool NESTEROV, bool ACC>
static void launch_opt_update(const int clip, ssd_train_state& s, const float* grad, const OptArgs& a, const int vec, hipStream_t st) {
    const dim3 grid(std::min(s.n_opt_segs * kOptSplit, 65536));
    const OptSeg* segs = reinterpret_cast<const OptSeg*>(s.opt_segs);
#define SSD_OPT_CASE(C)                                                                                                    \
    case C:                                                                                                                \
        hipLaunchKernelGGL((opt_update_kernel<OPT, NESTEROV, ACC, C>), grid, dim3(256), 0, st, s.flat, s.m, s.v, grad, segs, \
                           s.n_opt_segs, s.opt_norm, a, vec, kOptSplit);                                                             \
        break;
    switch (clip) {
        SSD_OPT_CASE(0)
        SSD_OPT_CASE(kClipNorm)
        SSD_OPT_CASE(kClipGlobal)
        SSD_OPT_CASE(kClipValue)
        SSD_OPT_CASE(kClipNorm | kClipValue)
        SSD_OPT_CASE(kClipGlobal | kClipValue)
    }
#undef SSD_OPT_CASE
}

}  // namespace ssd

extern "C" {

// Sum of the layers' regularisation losses, the term Keras adds to `loss` / `val_loss` beside the compiled
// losses: VGG16's kernel_regularizer=l2(5e-4) on every backbone / extra conv (models/ssd_vgg16.py:44-45),
// nothing for MobileNetV2 (keras-applications builds it without regularisers; models/header.py:60-61 has none).
int ssd_net_regularization_loss(ssd_net* net, float* host_out) {
    SSD_CHECK_ARG(net && host_out, "ssd_net_regularization_loss: NULL argument");
    *host_out = 0.f;
    if (net->backbone != SSD_VGG16) return SSD_OK;
    std::vector<const Param*> ws;
    for (const auto& l : net->layers)
        if (l.kind == LK_CONV && !l.head_kind && l.p_kernel >= 0 && net->params[l.p_kernel].dev) ws.push_back(&net->params[l.p_kernel]);
    if (ws.empty()) return SSD_OK;
    constexpr int kBlocks = 64;
    float* scratch = nullptr;
    SSD_HIP(hipMalloc((void**)&scratch, (ws.size() * kBlocks + 1) * sizeof(float)));
    for (size_t i = 0; i < ws.size(); ++i)
        hipLaunchKernelGGL(sumsq_kernel, dim3(kBlocks), dim3(256), 0, nullptr, ws[i]->dev, (long)ws[i]->count, scratch + i * kBlocks);
    hipLaunchKernelGGL(reg_finalize_kernel, dim3(1), dim3(1), 0, nullptr, scratch, (int)(ws.size() * kBlocks), 5e-4f,
                       scratch + ws.size() * kBlocks);
    const hipError_t e = hipMemcpy(host_out, scratch + ws.size() * kBlocks, sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(scratch);
    SSD_HIP(e);
    return SSD_OK;
}

// One update of every trainable parameter from grads_flat_dev (e.g. after the host's RCCL all-reduce; grad_scale =
// 1 / world_size turns the reduced SUM into the global-batch mean).  One launch over the table; with a norm clip two
// launches in front of it fill one scale per variable.  Frozen ranges are in no segment: their var, m and v stay bitwise,
// and the slots of a layer that is unfrozen later continue from where they were (Keras rebuilds its optimizer at the
// compile() that follows a change of `trainable`; here there is no such call).
int ssd_net_optimizer_step(ssd_net* net, const float* grads_flat_dev, const ssd_optimizer* opt, float lr, float grad_scale,
                           void* stream) {
    SSD_CHECK_ARG(net && grads_flat_dev && opt, "ssd_net_optimizer_step: NULL argument");
    SSD_CHECK_ARG(opt->kind == SSD_OPT_ADAM || opt->kind == SSD_OPT_SGD, "ssd_net_optimizer_step: unknown optimizer kind %d", opt->kind);
    if (opt->kind == SSD_OPT_ADAM)
        SSD_CHECK_ARG(opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f,
                      "ssd_net_optimizer_step: Adam's beta1 %g / beta2 %g must lie in [0, 1)", opt->beta1, opt->beta2);
    else
        SSD_CHECK_ARG(opt->momentum >= 0.f && opt->momentum <= 1.f, "ssd_net_optimizer_step: momentum %g must lie in [0, 1]", opt->momentum);
    SSD_CHECK_ARG(!(opt->clipnorm > 0.f && opt->global_clipnorm > 0.f),
                  "ssd_net_optimizer_step: clipnorm and global_clipnorm exclude each other");
    if (!net->train) { set_error("ssd_net_optimizer_step: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    const int clip = (opt->clipnorm > 0.f ? kClipNorm : 0) | (opt->global_clipnorm > 0.f ? kClipGlobal : 0) |
                     (opt->clipvalue > 0.f ? kClipValue : 0);
    ssd_train_state& s = *net->train;
    const int rp = refresh_plan(net, s);
    if (rp) return rp;
    if (s.step > 0 && s.opt_kind >= 0 && s.opt_kind != opt->kind) {
        set_error("ssd_net_optimizer_step: the optimizer slots were written by %s steps (%ld so far): call ssd_net_optimizer_reset before a step of another kind",
                  s.opt_kind == SSD_OPT_SGD ? "SGD" : "Adam", s.step);
        return SSD_E_STATE;
    }
    const bool norms = clip & (kClipNorm | kClipGlobal);
    SSD_UNSUPPORTED_IF(norms && s.n_opt_vars > kOptMaxVars, "ssd_net_optimizer_step: norm clipping over %d variables (limit %d)", s.n_opt_vars, kOptMaxVars);
    s.opt_kind = opt->kind;
    s.step += 1;
    OptArgs a{};
    a.lr = lr;
    if (opt->kind == SSD_OPT_ADAM) {
        const double t = (double)s.step;
        a.lr = (float)((double)lr * std::sqrt(1.0 - std::pow((double)opt->beta2, t)) / (1.0 - std::pow((double)opt->beta1, t)));
        a.b1 = opt->beta1; a.b2 = opt->beta2; a.eps = opt->eps;
    }
    a.momentum = opt->momentum;
    a.grad_scale = grad_scale;
    a.clipnorm = opt->clipnorm;
    a.clipvalue = opt->clipvalue;
    hipStream_t st = (hipStream_t)stream;
    const int vec = ((uintptr_t)grads_flat_dev & 15) == 0;     // (var, m and v are allocations of their own)
    if (s.n_opt_segs) {
        const OptSeg* segs = reinterpret_cast<const OptSeg*>(s.opt_segs);
        if (norms) {
            hipLaunchKernelGGL(opt_sumsq_kernel, dim3(s.n_opt_segs < 16384 ? s.n_opt_segs : 16384), dim3(256), 0, st, grads_flat_dev,
                               segs, s.n_opt_segs, grad_scale, s.opt_partial, vec);
            hipLaunchKernelGGL(opt_norm_finish_kernel, dim3(1), dim3(1024), 0, st, s.opt_partial,
                               reinterpret_cast<const OptVar*>(s.opt_vars), s.n_opt_vars, s.opt_norm, opt->clipnorm,
                               opt->global_clipnorm);
        }
        if (opt->kind == SSD_OPT_ADAM) launch_opt_update<SSD_OPT_ADAM, false, true>(clip, s, grads_flat_dev, a, vec, st);
        else if (opt->momentum == 0.f) launch_opt_update<SSD_OPT_SGD, false, false>(clip, s, grads_flat_dev, a, vec, st);
        else if (opt->nesterov) launch_opt_update<SSD_OPT_SGD, true, true>(clip, s, grads_flat_dev, a, vec, st);
        else launch_opt_update<SSD_OPT_SGD, false, true>(clip, s, grads_flat_dev, a, vec, st);
    }
    SSD_LAUNCH_CHECK();
    net->finalized = false;
    net->drop_graphs();
    return SSD_OK;
}

// Adam without a clip, the step the reference's compile() describes: ssd_net_optimizer_step under another signature.
int ssd_net_adam_step(ssd_net* net, const float* grads_flat_dev, float lr, float beta1, float beta2, float eps,
                      float grad_scale, void* stream) {
    ssd_optimizer opt{};
    opt.kind = SSD_OPT_ADAM;
    opt.beta1 = beta1; opt.beta2 = beta2; opt.eps = eps;
    return ssd_net_optimizer_step(net, grads_flat_dev, &opt, lr, grad_scale, stream);
}

int ssd_net_optimizer_reset(ssd_net* net) {
    SSD_CHECK_ARG(net, "ssd_net_optimizer_reset: NULL argument");
    if (!net->train) return SSD_OK;
    ssd_train_state& s = *net->train;
    SSD_HIP(hipDeviceSynchronize());
    SSD_HIP(hipMemset(s.m, 0, s.P * sizeof(float)));
    SSD_HIP(hipMemset(s.v, 0, s.P * sizeof(float)));
    SSD_HIP(hipDeviceSynchronize());
    s.step = 0;
    s.opt_kind = -1;
    return SSD_OK;
}

static float* optimizer_slot(ssd_net* net, const char* slot) {
    const std::string w(slot);
    return w == "m" ? net->train->m : w == "v" ? net->train->v : nullptr;
}
static bool optimizer_slot_known(const char* slot) { return std::string(slot) == "m" || std::string(slot) == "v"; }

long ssd_net_optimizer_get_state(ssd_net* net, const char* slot, float* host_out, size_t cap) {
    SSD_CHECK_ARG(net && slot, "ssd_net_optimizer_get_state: NULL argument");
    SSD_CHECK_ARG(optimizer_slot_known(slot), "ssd_net_optimizer_get_state: unknown slot '%s' (\"m\" | \"v\")", slot);
    const size_t n = ssd_net_trainable_floats(net);
    if (!host_out) return (long)n;
    SSD_CHECK_ARG(cap >= n, "ssd_net_optimizer_get_state: room for %zu floats, the slot has %zu", cap, n);
    if (!net->train) { set_error("ssd_net_optimizer_get_state: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    SSD_HIP(hipDeviceSynchronize());
    SSD_HIP(hipMemcpy(host_out, optimizer_slot(net, slot), n * sizeof(float), hipMemcpyDeviceToHost));
    return (long)n;
}

int ssd_net_optimizer_set_state(ssd_net* net, const char* slot, const float* host_in, size_t count) {
    SSD_CHECK_ARG(net && slot && host_in, "ssd_net_optimizer_set_state: NULL argument");
    SSD_CHECK_ARG(optimizer_slot_known(slot), "ssd_net_optimizer_set_state: unknown slot '%s' (\"m\" | \"v\")", slot);
    SSD_CHECK_ARG(count == ssd_net_trainable_floats(net), "ssd_net_optimizer_set_state: %zu floats given, the slot has %zu", count,
                  ssd_net_trainable_floats(net));
    if (!net->train) { set_error("ssd_net_optimizer_set_state: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    SSD_HIP(hipDeviceSynchronize());
    SSD_HIP(hipMemcpy(optimizer_slot(net, slot), host_in, count * sizeof(float), hipMemcpyHostToDevice));
    return SSD_OK;
}

int ssd_net_train_set_steps(ssd_net* net, long steps) {
    SSD_CHECK_ARG(net && steps >= 0, "ssd_net_train_set_steps: bad arguments");
    if (!net->train) { set_error("ssd_net_train_set_steps: call ssd_net_train_begin() first"); return SSD_E_STATE; }
    net->train->step = steps;
    return SSD_OK;
}

long ssd_net_train_steps(const ssd_net* net) { return (net && net->train) ? net->train->step : 0; }

}  // extern "C"
