// Row-band fused MobileNetV2 inverted-residual block for the HIGH-resolution stages (blocks 1-6 of
// SSD300: 150x150 / 75x75 / 38x38 maps, Cin 16 / 24 / 32):
//
//     y = project_BN( relu6(dw_BN( dw3x3( relu6(expand_BN( x * We )) ) )) * Wp ) [+ x]
//
// ([3P] keras-applications MobileNetV2 block_k_expand .. block_k_add, SURVEY.md Appendix A.)
// The whole-image kernel (ssd_imgblock.hip) showed what works on gfx950 -- no horizontal halo, the
// depthwise computed by each lane AS the project MFMA's B fragment (D never returns to LDS), one LDS
// barrier per 16-channel chunk, conflict-free E layout -- but needs the whole map in one workgroup.
// Here a workgroup owns a full-width BAND of R output rows of one image:
//
//   pixel space of the band's input rows: q = rb * P + c, pitch P >= W + 1 (the columns c >= W of a row are
//     the zero padding to the right of row rb AND to the left of row rb + 1), P a multiple of 8; 16
//     consecutive q = one MFMA pixel tile; tiles are dealt round-robin to the 8 waves (T per wave)
//   X   the wave's input tiles as MFMA B fragments, loaded ONCE from global into registers
//   per 16-channel chunk of the Ce expanded channels (E double-buffered in LDS, ONE barrier per chunk):
//     A  expand   E[q][16] = relu6(X[q][Cin] * We[Cin][16] + shift), 0 at pad positions / rows outside the
//                 image -> LDS row e = q + 8, 64-byte rows, 16-byte quad index XOR (e >> 1) & 3:
//                 conflict-free b128 tile writes and stride-1 fragment reads at any alignment
//     B  depthw.  each lane computes ITS output pixel x 4 channels from 9 ds_read_b128 (3 address
//                 registers per tile: the dy offsets are immediates because P % 8 == 0 keeps the swizzle)
//                 = exactly the B fragment of phase C
//     C  project  acc[qo][Cout] += D[qo][16] * Wp[16][Cout], accumulators in registers
//   the A fragments of We / Wp reach LDS by LDS-DMA (two stages each of the chunk's We rows and Wp rows; 1 KB
//   blocks of 16 rows x 16 floats, quad-swizzled through the per-lane source offset): waiting in registers one
//   chunk ahead instead cost 16-70 registers and per-chunk 64-bit addresses and measured slower on every block
//   epilogue    y = acc + shift (+ x), 16-byte stores
//
// Only the two (stride 1) or one (stride 2) halo rows between bands are expanded twice (1.2-1.3x of the
// expand, nothing of the depthwise / project) where the 8x8 tiles of ssd_fused.hip recompute 1.56x.

#include "ssd_band_common.h"

namespace ssd {

namespace {

template <int CIN, int NT, int T, int TO, int S, int P>
__device__ __forceinline__ void band_body(const FusedBlockParams& p, char* __restrict__ smem) {
    constexpr int KC = CIN / 16;                  // 16-wide k blocks of the expand
    constexpr bool TAIL = (CIN % 16) == 8;        // + one 8-wide k tail (Cin = 24): 2 MFMA k-steps
    constexpr int EBUF = band_ne(T) * kBandC * 4; // bytes per E buffer

    char* Es = smem;                                             // [2][NE][16] floats, swizzled
    float* Ps = reinterpret_cast<float*>(smem + 2 * EBUF);       // [11][Ce]: expand shift, taps [9], depthwise shift

    SSD_BAND_GEOMETRY(p, S, P);
    band_stage_params(p, tid, Es, EBUF, Ps);

    // ---- the wave's input tiles: B fragments of X in registers, loaded once
    f32x4 xb[T][KC];
    f32x2 xt[T];
    unsigned realm = 0;                           // bit t: this lane's pixel of tile t is a real image pixel
#pragma unroll
    for (int t = 0; t < T; ++t) {
        SSD_BAND_REAL_PIXEL(t, P);
        realm |= real ? (1u << t) : 0u;
        const float* xp = p.x + SSD_BAND_XPIX * CIN;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
            xb[t][kc] = real ? *reinterpret_cast<const f32x4*>(xp + kc * 16 + g4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (TAIL) xt[t] = real ? *reinterpret_cast<const f32x2*>(xp + KC * 16 + g4 * 2) : f32x2{0.f, 0.f};
    }
    SSD_BAND_OUT_WINDOWS(p, TO, S, P)

    // ---- A fragments of the weights through LDS
    constexpr int NBE = KC + (TAIL ? 1 : 0);      // 1 KB blocks of a We chunk (16 rows x 16 floats each)
    float* Wes = Ps + 11 * p.Ce;                  // [2][NBE] blocks of 256 floats
    float* Wps = Wes + 2 * NBE * 256;             // [2][NT] blocks
    const int fslot = l15 * 16 + ((g4 ^ ((l15 >> 1) & 3)) * 4);                  // the lane's 16-byte slot inside a block
    const int tslot = l15 * 16 + (((g4 >> 1) ^ ((l15 >> 1) & 3)) * 4) + (g4 & 1) * 2;   // ... its 8 bytes of the k tail
    const int dr = lane >> 2, dq4 = ((lane & 3) ^ ((lane >> 3) & 3)) * 4;
    const __amdgpu_buffer_rsrc_t rs_e = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.we), 0, (int)((long)p.Ce * p.kpad_e * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wp), 0, (int)((long)p.npad_p * p.kpad_p * 4), 0x00020000);
    const int voff_e = (dr * p.kpad_e + dq4) * 4, voff_p = (dr * p.kpad_p + dq4) * 4;
    auto dma_we = [&](int j, int stage) {
        for (int b = wave; b < NBE; b += 8)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_e, (lds_dst_t)(Wes + (stage * NBE + b) * 256), 16, voff_e,
                                                     (int)(((long)j * kBandC * p.kpad_e + b * 16) * 4), 0, 0);
    };
    auto dma_wp = [&](int j, int stage) {
        for (int b = wave; b < NT; b += 8)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_p, (lds_dst_t)(Wps + (stage * NT + b) * 256), 16, voff_p,
                                                     (int)(((long)b * 16 * p.kpad_p + j * kBandC) * 4), 0, 0);
    };
    auto dma_wait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
    f32x4 wa[KC], wp[NT];
    f32x2 wat;
    auto load_we = [&](f32x4 (&a)[KC], f32x2& at, int j) {
        const float* wb = Wes + (j & 1) * NBE * 256;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) a[kc] = *reinterpret_cast<const f32x4*>(wb + kc * 256 + fslot);
        if (TAIL) at = *reinterpret_cast<const f32x2*>(wb + KC * 256 + tslot);
    };
    auto load_wp = [&](f32x4 (&a)[NT], int j) {
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) a[ni] = *reinterpret_cast<const f32x4*>(Wps + ((j & 1) * NT + ni) * 256 + fslot);
    };
    dma_we(0, 0);
    if (nchunk > 1) dma_we(1, 1);
    dma_wp(0, 0);
    dma_wait();
    __syncthreads();                              // Ps, zero rows

    auto expand = [&](int j, const f32x4 (&a)[KC], const f32x2 at) {
        const f32x4 sh = *reinterpret_cast<const f32x4*>(Ps + j * kBandC + g4 * 4);
        char* eb = Es + (j & 1) * EBUF + ew;
        // two tiles at a time: independent accumulator chains (dependent fp32 MFMAs issue every 40 cycles, not 32)
#pragma unroll
        for (int t0 = 0; t0 < T; t0 += 2) {
            if (t0 >= nti) break;                 // scalar
            f32x4 acc0 = sh, acc1 = sh;
            const bool two = t0 + 1 < T;
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kc][s], xb[t0][kc][s], acc0, 0, 0, 0);
                    if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kc][s], xb[t0 + 1 < T ? t0 + 1 : t0][kc][s], acc1, 0, 0, 0);
                }
            if (TAIL) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s], xt[t0][s], acc0, 0, 0, 0);
                    if (two) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(at[s], xt[t0 + 1 < T ? t0 + 1 : t0][s], acc1, 0, 0, 0);
                }
            }
            const float hi0 = (realm >> t0) & 1u ? 6.0f : 0.0f;           // relu6 at real pixels, 0 at pad positions
#pragma unroll
            for (int e = 0; e < 4; ++e) acc0[e] = __builtin_amdgcn_fmed3f(acc0[e], 0.0f, hi0);
            *reinterpret_cast<f32x4*>(eb + t0 * 8192) = acc0;
            if (two && t0 + 1 < nti) {
                const float hi1 = (realm >> (t0 + 1)) & 1u ? 6.0f : 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc1[e] = __builtin_amdgcn_fmed3f(acc1[e], 0.0f, hi1);
                *reinterpret_cast<f32x4*>(eb + (t0 + 1) * 8192) = acc1;
            }
        }
    };

    f32x4 acc[TO][NT];
#pragma unroll
    for (int t = 0; t < TO; ++t)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) acc[t][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    // depthwise (this lane's pixel x 4 channels = the B fragment) + project MFMAs of chunk i, tile by tile
    auto dwproject = [&](int i, const f32x4 (&wpc)[NT]) {
        const char* eb = Es + (i & 1) * EBUF;
        f32x4 w[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) w[k] = band_param4(Ps, Ce, 1 + k, i, g4);
        const f32x4 dh = band_param4(Ps, Ce, 10, i, g4);
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            if (t >= nto) break;                // scalar
            SSD_BAND_DW_TILE(d, eb, ea[t], w, dh, P);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int ni = 0; ni < NT; ++ni)
                    acc[t][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(wpc[ni][s4], d[s4], acc[t][ni], 0, 0, 0);
        }
    };

    // (Running { expand (i + 1), depthwise + project (i) } in the opposite order on waves 4-7, so that SIMD
    // partners are never in the same phase, was measured: +-3 %, no gain -- the kernel is issue bound, not
    // latency bound.)
    load_we(wa, wat, 0);
    expand(0, wa, wat);
    for (int i = 0; i < nchunk; ++i) {
        dma_wait();                 // the copies of an iteration ago have landed ...
        lds_barrier();              // ... and are visible; E(i) is complete; everyone is done reading E(i - 1)
        if (i + 2 < nchunk) dma_we(i + 2, i & 1);           // the stage expand(i) read before this barrier
        if (i + 1 < nchunk) dma_wp(i + 1, (i + 1) & 1);     // the stage dwproject(i - 1) read before this barrier
        load_wp(wp, i);
        dwproject(i, wp);
        if (i + 1 < nchunk) {
            load_we(wa, wat, i + 1);
            expand(i + 1, wa, wat);
        }
    }

    band_epilogue<TO, NT>(p, img, g4, opix, acc);
}

template <int CIN, int NT, int T, int TO, int S, int P>
__global__ __launch_bounds__(kBandThreads) void mbv2_band_block_kernel(const FusedBlockParams p) {
    extern __shared__ __attribute__((aligned(1024))) char smem_band[];
    band_body<CIN, NT, T, TO, S, P>(p, smem_band);
}

#define BAND_FN(CIN, NT, T, TO, S, P) mbv2_band_block_kernel<CIN, NT, T, TO, S, P>,
const band_kernel_t kBandFn[kBandShapeCount] = {SSD_BAND_SHAPES(BAND_FN)};

// 1 KB blocks of the weight stages: two stages each of the We chunk (with its k tail) and of the Wp chunk
constexpr int band_wblocks(const BandShape& s) { return 2 * (s.cin / 16 + ((s.cin % 16) == 8 ? 1 : 0) + s.nt); }
static_assert(band_shapes_fit_lds(band_wblocks), "every shape must fit the LDS with its weight stages");

int pick_band(const FusedBlockParams& p) {
    if (p.kpad_e % 4 != 0 || p.kpad_p % 4 != 0) return -1;
    return pick_band_shape(p);
}

size_t band_lds(int i, const FusedBlockParams& p) { return band_lds_bytes(kBandShapes[i], p.Ce, band_wblocks(kBandShapes[i])); }

}  // namespace

bool band_block_supported(const FusedBlockParams& p) {
    const int i = pick_band(p);
    return i >= 0 && band_lds(i, p) <= kBandLdsMax;
}

int launch_band_block(FusedBlockParams p, hipStream_t st) {
    const int i = pick_band(p);
    if (i < 0) {
        set_error("band block: unsupported shape Cin=%d Ce=%d Cout=%d %dx%d stride=%d", p.Cin, p.Ce, p.Cout, p.H, p.W, p.stride);
        return SSD_E_UNSUPPORTED;
    }
    return launch_band_kernel(kBandFn[i], kBandShapes[i], band_lds(i, p), p, st);
}

}  // namespace ssd
