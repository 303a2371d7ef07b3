// Row-band inverted-residual kernel (see ssd_bandblock.hip and ssd_band_common.h) with the two 1x1 convolutions on the BF16
// matrix cores at FP32 accuracy (exact three-way bf16 split of both operands, six MFMAs per product: ssd_bf16x3.h).
// The network's results stay within the 1e-4 contract; they are not bit-identical to the fp32-MFMA kernels.
//
// What differs from ssd_bandblock.hip:
//   * X is split once per band into three bf16 planes (lane = pixel x 8 channels g4*8.., K padded to 32)
//   * expand: 16 expanded channels x K = 32 = ONE k-step: 6 MFMAs per pixel tile and chunk; weights pre-split at
//     finalize (split3_we_kernel)
//   * project: K = 32 = TWO consecutive 16-channel chunks: the depthwise output of the even chunk waits in registers,
//     after the odd chunk the lane's 8 values are split and 6 x NT MFMAs run (k-slot (g4, j): j < 4 -> even chunk channel
//     g4*4 + j, j >= 4 -> odd chunk; the pre-split project weights are packed in that order, split3_wp_kernel)
//   * the weight fragments reach LDS by LDS-DMA (two We stages, one Wp stage; 1 KB blocks of 16 rows x 32 bf16, quad-swizzled
//     through the per-lane source offset): waiting in registers one chunk ahead instead cost 36 - 60 registers and per-chunk
//     64-bit addresses and measured slower on every block

#include "ssd_band_common.h"
#include "ssd_bf16x3.h"

namespace ssd {

namespace {

// out[plane][row][32]: We (BatchNorm scale folded, packed [Ce][kpad]) split, K = Cin padded to 32
__global__ __launch_bounds__(256) void split3_we_kernel(const float* __restrict__ we, int Ce, int Cin, int kpad, short* __restrict__ out) {
    const long total = (long)Ce * 32;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int row = (int)(e >> 5), k = (int)(e & 31);
        const float v = k < Cin ? we[(long)row * kpad + k] : 0.f;
        short h, m, l;
        split1(v, h, m, l);
        out[e] = h;
        out[total + e] = m;
        out[2 * total + e] = l;
        out[3 * total + e] = rne1(v);        // plane 3: the bf16 rounding (precision-1 form of the kernel)
    }
}
// out[plane][row][pair][g4][8]: Wp (packed [npad][kpad], K = Ce) split, k-slots in chunk-pair order
__global__ __launch_bounds__(256) void split3_wp_kernel(const float* __restrict__ wp, int npad, int Ce, int kpad, int npairs,
                                                       short* __restrict__ out) {
    const long total = (long)npad * npairs * 32;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int j = (int)(e & 7), g4 = (int)((e >> 3) & 3);
        const long rp = e >> 5;
        const int pair = (int)(rp % npairs), row = (int)(rp / npairs);
        const int ch = (2 * pair + (j >> 2)) * 16 + g4 * 4 + (j & 3);
        const float v = ch < Ce ? wp[(long)row * kpad + ch] : 0.f;
        short h, m, l;
        split1(v, h, m, l);
        out[e] = h;
        out[total + e] = m;
        out[2 * total + e] = l;
        out[3 * total + e] = rne1(v);
    }
}

// NP = 3: fp32 results through the exact three-way split (six MFMAs per product); NP = 1: the net's bf16 mode (operands
// rounded once, one MFMA per product, plane 3 of the packed weights) -- a third of the plane registers, so blocks 1-2
// (T = 9 / 8 tiles per wave) fit as well
template <int CIN, int NT, int T, int TO, int S, int P, int NP>
__device__ __forceinline__ void band3_body(const FusedBlockParams& p, char* __restrict__ smem) {
    constexpr int WPL = NP == 1 ? 3 : 0;
    static_assert(CIN <= 32 && CIN % 8 == 0, "");
    constexpr int EBUF = band_ne(T) * kBandC * 4;

    char* Es = smem;
    float* Ps = reinterpret_cast<float*>(smem + 2 * EBUF);       // [11][Ce]

    SSD_BAND_GEOMETRY(p, S, P);
    const int npairs = (nchunk + 1) >> 1;
    const long plane_e = (long)Ce * 32, plane_p = (long)p.npad_p * npairs * 32;
    band_stage_params(p, tid, Es, EBUF, Ps);

    // ---- the wave's input tiles: X split once into three bf16 planes (lane = pixel x channels g4*8 .. g4*8 + 7)
    BP<NP> xs[T];
    unsigned realm = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        SSD_BAND_REAL_PIXEL(t, P);
        realm |= real ? (1u << t) : 0u;
        const bool have = real && g4 * 8 < CIN;
        const float* xp = p.x + SSD_BAND_XPIX * CIN + (g4 * 8 < CIN ? g4 * 8 : 0);
        const f32x4 a = have ? *reinterpret_cast<const f32x4*>(xp) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 b = have ? *reinterpret_cast<const f32x4*>(xp + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        xs[t] = splitN<NP>(a, b);
    }
    SSD_BAND_OUT_WINDOWS(p, TO, S, P)

    short* Wes = reinterpret_cast<short*>(Ps + 11 * Ce);         // [2][NP] blocks of 512 bf16
    short* Wps = Wes + 2 * NP * 512;                             // [NP][NT] blocks
    const int fslot = l15 * 32 + ((g4 ^ ((l15 >> 1) & 3)) * 8);  // the lane's fragment slot inside a block
    const int dr = lane >> 2, dq8 = ((lane & 3) ^ ((lane >> 3) & 3)) * 8;
    const __amdgpu_buffer_rsrc_t rs_e = __builtin_amdgcn_make_buffer_rsrc(const_cast<short*>(p.we3 + WPL * plane_e), 0, (int)(NP * plane_e * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<short*>(p.wp3 + WPL * plane_p), 0, (int)(NP * plane_p * 2), 0x00020000);
    const int voff_e = (dr * 32 + dq8) * 2, voff_p = (dr * npairs * 32 + dq8) * 2;
    auto dma_we = [&](int j, int stage) {
        for (int b = wave; b < NP; b += 8)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_e, (lds_dst_t)(Wes + (stage * NP + b) * 512), 16, voff_e,
                                                     (int)((b * plane_e + (long)j * kBandC * 32) * 2), 0, 0);
    };
    auto dma_wp = [&](int pair) {
        for (int b = wave; b < NP * NT; b += 8) {
            const int pl = b / NT, ni = b - pl * NT;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_p, (lds_dst_t)(Wps + b * 512), 16, voff_p,
                                                     (int)((pl * plane_p + ((long)ni * 16 * npairs + pair) * 32) * 2), 0, 0);
        }
    };
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    auto load_we = [&](int j) {
        BP<NP> w;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) w.p[pl] = *reinterpret_cast<const bf16x8*>(Wes + ((j & 1) * NP + pl) * 512 + fslot);
        return w;
    };
    dma_we(0, 0);
    if (nchunk > 1) dma_we(1, 1);
    dma_wp(0);
    dma_wait();
    __syncthreads();

    auto expand = [&](int j, const BP<NP>& wa) {
        const f32x4 sh = *reinterpret_cast<const f32x4*>(Ps + j * kBandC + g4 * 4);
        char* eb = Es + (j & 1) * EBUF + ew;
#pragma unroll
        for (int t0 = 0; t0 < T; t0 += 2) {
            if (t0 >= nti) break;
            const int t1 = t0 + 1 < T ? t0 + 1 : t0;
            f32x4 a0 = mmaN<NP>(wa, xs[t0], sh), a1 = sh;
            if (t0 + 1 < T) a1 = mmaN<NP>(wa, xs[t1], sh);
            const float hi0 = (realm >> t0) & 1u ? 6.0f : 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) a0[e] = __builtin_amdgcn_fmed3f(a0[e], 0.0f, hi0);
            *reinterpret_cast<f32x4*>(eb + t0 * 8192) = a0;
            if (t0 + 1 < T && t0 + 1 < nti) {
                const float hi1 = (realm >> t1) & 1u ? 6.0f : 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e) a1[e] = __builtin_amdgcn_fmed3f(a1[e], 0.0f, hi1);
                *reinterpret_cast<f32x4*>(eb + t1 * 8192) = a1;
            }
        }
    };

    f32x4 acc[TO][NT];
    f32x4 dprev[TO];
#pragma unroll
    for (int t = 0; t < TO; ++t) {
        dprev[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[t][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    expand(0, load_we(0));
    for (int i = 0; i < nchunk; ++i) {
        dma_wait();                 // the copies of an iteration ago have landed ...
        lds_barrier();              // ... and are visible; E(i) is complete; everyone is done reading E(i - 1)
        const bool odd = i & 1, last = i + 1 == nchunk;
        const bool flush = odd || last;                     // the project runs after every second chunk (and after a last odd one)
        if (i + 2 < nchunk) dma_we(i + 2, i & 1);           // the stage expand(i) read before this barrier
        if (!odd && i > 0) dma_wp(i >> 1);                  // everyone projected the pair before at iteration i - 1
        if (!odd && last && i > 0) {                        // a lone last chunk projects in the iteration its weights are issued in
            dma_wait();
            lds_barrier();
        }
        const char* eb = Es + (i & 1) * EBUF;
        f32x4 w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = band_param4(Ps, Ce, 1 + k, i, g4);
        const f32x4 dh = band_param4(Ps, Ce, 10, i, g4);
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            if (t >= nto) break;
            SSD_BAND_DW_TILE(d, eb, ea[t], w, dh, P);
            if (!flush) {
                dprev[t] = d;
            } else {
                const BP<NP> ds = odd ? splitN<NP>(dprev[t], d) : splitN<NP>(d, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                for (int ni = 0; ni < NT; ++ni) {
                    BP<NP> wpf;
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) wpf.p[pl] = *reinterpret_cast<const bf16x8*>(Wps + (pl * NT + ni) * 512 + fslot);
                    acc[t][ni] = mmaN<NP>(wpf, ds, acc[t][ni]);
                }
            }
        }
        if (i + 1 < nchunk) expand(i + 1, load_we(i + 1));
    }

    band_epilogue<TO, NT>(p, img, g4, opix, acc);
}

template <int CIN, int NT, int T, int TO, int S, int P, int NP>
__global__ __launch_bounds__(kBandThreads) void mbv2_band3_block_kernel(const FusedBlockParams p) {
    extern __shared__ __attribute__((aligned(1024))) char smem_b3[];
    band3_body<CIN, NT, T, TO, S, P, NP>(p, smem_b3);
}

// The split-bf16 form exists where the three X planes (12 registers per tile) fit: up to T = 7 tiles per wave.  Blocks
// 1-2 (T = 9 / 8) spilled (9 / 46 registers) and measured 149-158 / 162-172 us against 143 / 105 on the fp32 band kernel:
// those shapes exist in the bf16 form only.
constexpr bool band3_has_split(const BandShape& s) { return s.t <= 7; }
template <int CIN, int NT, int T, int TO, int S, int P>
constexpr band_kernel_t band3_split_fn() {
    if constexpr (band3_has_split(BandShape{CIN, NT, T, TO, S, P})) return mbv2_band3_block_kernel<CIN, NT, T, TO, S, P, 3>;
    else return nullptr;
}
#define BAND3_SPLIT_FN(CIN, NT, T, TO, S, P) band3_split_fn<CIN, NT, T, TO, S, P>(),
#define BAND3_BF16_FN(CIN, NT, T, TO, S, P) mbv2_band3_block_kernel<CIN, NT, T, TO, S, P, 1>,
const band_kernel_t kBand3Fn[2][kBandShapeCount] = {{SSD_BAND_SHAPES(BAND3_SPLIT_FN)}, {SSD_BAND_SHAPES(BAND3_BF16_FN)}};

// 1 KB blocks of the weight stages: per plane two We stages and one Wp stage of NT blocks
constexpr int band3_wblocks(const BandShape& s, int np) { return np * (2 + s.nt); }
static_assert(band_shapes_fit_lds([](const BandShape& s) { return band3_has_split(s) ? band3_wblocks(s, 3) : -1; }) &&
                  band_shapes_fit_lds([](const BandShape& s) { return band3_wblocks(s, 1); }),
              "every shape must fit the LDS with its weight stages");

int pick_band3(const FusedBlockParams& p) {
    const int i = pick_band_shape(p);
    return i >= 0 && kBand3Fn[p.bf16 != 0][i] ? i : -1;
}

size_t band3_lds(int i, const FusedBlockParams& p) {
    return band_lds_bytes(kBandShapes[i], p.Ce, band3_wblocks(kBandShapes[i], p.bf16 ? 1 : 3));
}

}  // namespace

bool band3_block_supported(const FusedBlockParams& p) {
    const int i = pick_band3(p);
    return i >= 0 && band3_lds(i, p) <= kBandLdsMax;
}

// bf16 planes of the two 1x1 weight matrices (shorts): sizes and the packing launches (run at finalize)
size_t band3_we_shorts(int Ce) { return (size_t)4 * Ce * 32; }
size_t band3_wp_shorts(int npad_p, int Ce) { return (size_t)4 * npad_p * (((Ce / kBandC) + 1) / 2) * 32; }
int launch_band3_pack(const float* we, int Ce, int Cin, int kpad_e, short* we3, const float* wp, int npad_p, int kpad_p,
                      short* wp3, hipStream_t st) {
    const int npairs = ((Ce / kBandC) + 1) / 2;
    hipLaunchKernelGGL(split3_we_kernel, dim3((Ce * 32 + 255) / 256), dim3(256), 0, st, we, Ce, Cin, kpad_e, we3);
    SSD_LAUNCH_CHECK();
    hipLaunchKernelGGL(split3_wp_kernel, dim3((npad_p * npairs * 32 + 255) / 256), dim3(256), 0, st, wp, npad_p, Ce, kpad_p, npairs, wp3);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

int launch_band3_block(FusedBlockParams p, hipStream_t st) {
    const int i = pick_band3(p);
    if (i < 0 || !p.we3 || !p.wp3) {
        set_error("band3 block: unsupported shape Cin=%d Ce=%d Cout=%d %dx%d stride=%d (or weights not split)", p.Cin, p.Ce, p.Cout,
                  p.H, p.W, p.stride);
        return SSD_E_UNSUPPORTED;
    }
    return launch_band_kernel(kBand3Fn[p.bf16 != 0][i], kBandShapes[i], band3_lds(i, p), p, st);
}

}  // namespace ssd
