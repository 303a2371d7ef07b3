// What the two row-band block kernels share (ssd_bandblock.hip: fp32 MFMA; ssd_band3.hip: split-bf16 / bf16): the shape
// table and the launch on the host side; the band geometry, the parameter staging, the pixel addressing, the per-lane
// depthwise tile and the epilogue on the device side, each written once.  The organisation of a band is described at the top of
// ssd_bandblock.hip.  What stays in the two files is what differs between them: the X fragment format, the weight
// copies, the expand product and the project cadence.
#pragma once
#include "ssd_block_common.h"
#include "ssd_conv.h"

namespace ssd {

constexpr int kBandThreads = 512;
constexpr int kBandC = 16;                        // expanded channels per chunk
constexpr size_t kBandLdsMax = 160 * 1024;

// LDS rows of the E chunk for T input tiles per wave: 8 leading zero rows (q = -1 is read by the left
// tap of column 0 in band row 0) + every tile slot
constexpr int band_ne(int T) { return 8 + T * 8 * 16; }

// ---------------------------------------------------------------------------------------------------------- host side
// The compile-time shapes: Cin, NT 16-channel output tiles, T input / TO output pixel tiles per wave, stride, pixel
// pitch of a band row.  Each kernel file maps SSD_BAND_SHAPES to its own instantiations, in this order.
struct BandShape {
    int cin, nt, t, to, stride, pitch;
};
// (Block 1 of the 512x512 graph, 256x256, stays on the 8x8-tile kernel: a full-width band holds ONE output row -- 3 input
// rows of pitch 264 fill the 9 tile slots -- and measured 127 us against 116.)
#define SSD_BAND_SHAPES(X)                                                               \
    X(16, 2, 9, 2, 2, 152) /* block 1: 16 -> 96 -> 24, 150x150 -> 75x75 */               \
    X(24, 2, 8, 6, 1, 80)  /* block 2: 24 -> 144 -> 24 (+x) at 75x75 */                  \
    X(24, 2, 7, 2, 2, 80)  /* block 3: 24 -> 144 -> 32, 75x75 -> 38x38 */                \
    X(32, 2, 4, 4, 1, 40)  /* blocks 4-5: 32 -> 192 -> 32 (+x) at 38x38 */               \
    X(32, 4, 4, 1, 2, 40)  /* block 6: 32 -> 192 -> 64, 38x38 -> 19x19 */                \
    /* the 512x512 graph (BASELINE configs[4]): maps 128 / 64 wide */                    \
    X(24, 2, 8, 6, 1, 136) /* block 2 at 128x128 */                                      \
    X(24, 2, 7, 2, 2, 136) /* block 3: 128x128 -> 64x64 */                               \
    X(32, 2, 4, 4, 1, 72)  /* blocks 4-5 at 64x64 */                                     \
    X(32, 4, 4, 1, 2, 72)  /* block 6: 64x64 -> 32x32 */
#define SSD_BAND_SHAPE_ROW(CIN, NT, T, TO, S, P) {CIN, NT, T, TO, S, P},
constexpr BandShape kBandShapes[] = {SSD_BAND_SHAPES(SSD_BAND_SHAPE_ROW)};
constexpr int kBandShapeCount = sizeof(kBandShapes) / sizeof(kBandShapes[0]);

// The order of the table does not matter: a block matches a shape on (Cin, NT, stride) and W + 1 <= pitch <= W + 8, so two
// shapes that agree on the former and lie 8 or more apart in pitch can never both match.
constexpr bool band_shapes_disjoint() {
    for (int i = 0; i < kBandShapeCount; ++i)
        for (int j = i + 1; j < kBandShapeCount; ++j) {
            const BandShape &a = kBandShapes[i], &b = kBandShapes[j];
            const int dp = a.pitch > b.pitch ? a.pitch - b.pitch : b.pitch - a.pitch;
            if (a.cin == b.cin && a.nt == b.nt && a.stride == b.stride && dp < 8) return false;
        }
    return true;
}
static_assert(band_shapes_disjoint(), "no FusedBlockParams may match two shapes");

// LDS need: two E buffers, the 11 parameter rows and `wblocks` 1 KB blocks of LDS-DMA weight stages (the kernel's own count)
constexpr size_t band_lds_bytes(const BandShape& s, int Ce, int wblocks) {
    return (size_t)2 * band_ne(s.t) * kBandC * 4 + (size_t)11 * Ce * 4 + (size_t)wblocks * 1024;
}
// ... fits for every shape at the MobileNetV2 expansion Ce = 6 Cin (wblocks(shape) < 0: the kernel has no such form).  The
// weights have no other way into the kernels, so each kernel file asserts this for every form it instantiates.
template <class F>
constexpr bool band_shapes_fit_lds(F wblocks) {
    for (const BandShape& s : kBandShapes)
        if (wblocks(s) >= 0 && band_lds_bytes(s, 6 * s.cin, wblocks(s)) > kBandLdsMax) return false;
    return true;
}

// largest band (output rows) a shape can hold: input tiles and output tiles both have to fit
inline int band_max_rows(const BandShape& s, const FusedBlockParams& p) {
    const int hb = s.t * 8 * 16 / s.pitch;                       // band input rows that fit the tile slots
    int r = s.stride == 1 ? hb - 2 : (hb - 1) / 2;
    const int po = p.Wo + 1;
    while (r > 0 && (r * po + 15) / 16 > s.to * 8) --r;
    return r;
}

// index of the block's shape in kBandShapes, or -1 (the checks the two kernels share)
inline int pick_band_shape(const FusedBlockParams& p) {
    if (p.Ce % kBandC != 0 || p.Cout % 8 != 0) return -1;
    if (p.stride == 1 && (p.H != p.Ho || p.W != p.Wo || p.pad_t != 1 || p.pad_l != 1)) return -1;
    if (p.stride == 2 && (p.residual || p.Ho != (p.H + 1) / 2 || p.Wo != (p.W + 1) / 2 || p.pad_t > 1 || p.pad_l > 1 ||
                          p.pad_t < 0 || p.pad_l < 0))
        return -1;
    if (p.residual && p.Cin != p.Cout) return -1;
    if (p.e_out) return -1;
    for (int i = 0; i < kBandShapeCount; ++i) {
        const BandShape& s = kBandShapes[i];
        if (s.cin != p.Cin || s.stride != p.stride || (p.Cout + 15) / 16 != s.nt || p.npad_p < s.nt * 16) continue;
        if (p.W + 1 > s.pitch || p.W + 8 < s.pitch) continue;    // the shape's pitch is for this width
        // stride 2: the right-most tap column 2 (Wo - 1) - pad_l + 2 must be a pad column (or inside the map)
        if (p.stride == 2 && 2 * (p.Wo - 1) - p.pad_l + 2 >= s.pitch) continue;
        if (band_max_rows(s, p) < 1) continue;
        return i;
    }
    return -1;
}

typedef void (*band_kernel_t)(const FusedBlockParams);

// one workgroup per band: band b = output rows [b * Ho / bands, (b + 1) * Ho / bands)
inline int launch_band_kernel(band_kernel_t fn, const BandShape& s, size_t lds, FusedBlockParams p, hipStream_t st) {
    if (p.B == 0) return SSD_OK;
    SSD_UNSUPPORTED_IF(lds > kBandLdsMax, "band block: needs %zu B of LDS", lds);
    const int rmax = band_max_rows(s, p);
    p.bands = (p.Ho + rmax - 1) / rmax;
    if (lds > 64 * 1024) SSD_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)((long)p.B * p.bands)), dim3(kBandThreads), lds, st, p);
    SSD_LAUNCH_CHECK();
    return SSD_OK;
}

// -------------------------------------------------------------------------------------------------------- device side
// The blocks of declarations below are macros, not functions, on purpose.  hipcc simplifies every function once on its
// own (SROA, InstCombine) before it inlines even the forced ones, and a function that receives the lane's coordinates as
// arguments, or reads them back from a struct, is simplified without their value ranges: the address arithmetic of the
// kernels then comes out in another form, and with it the schedule and the unrolling of the chunk loop.  As text in the
// kernel body they compile to the instructions they always did (profiles/HISTORY.md, "One row-band skeleton").
//
// Where this workgroup and this lane stand.  Pixel space of the band's input rows: q = rb * P + c; tiles of 16 consecutive
// q are dealt round-robin to the 8 waves (tile = t * 8 + wave); the output rows have their own space qo = rol * Po + co.
// Declares: tid, lane, l15, g4, wave (scalar: the tile-count tests are s_cbranch, not exec masks); img; H, W, Ho, Wo, Ce;
// the band's output rows [ro0, ro0 + R); its first input row ri0 (may be -1) and row count HB; npt input and npo output
// pixel tiles, output pitch Po; nchunk; this wave's tile counts nti / nto.
// XCD-aware item order: hardware deals consecutive workgroup ids round-robin over the 8 XCDs (own L2 each); the bands of
// one image -- which share their halo rows of x -- get ids that land on the same XCD.
#define SSD_BAND_GEOMETRY(p, S, P)                                                                                          \
    static_assert(P % 8 == 0, "the dy tap offsets must keep the quad swizzle");                                             \
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;                                          \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                              \
    const int nb = p.bands;                                                                                                 \
    const int items = p.B * nb;                                                                                             \
    const int bid = (items & 7) == 0 ? (int)(blockIdx.x & 7) * (items >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;     \
    const int img = bid / nb, band = bid - img * nb;                                                                        \
    const int H = p.H, W = p.W, Ho = p.Ho, Wo = p.Wo, Ce = p.Ce;                                                            \
    const int ro0 = band * Ho / nb, R = (band + 1) * Ho / nb - ro0;                                                         \
    const int ri0 = S * ro0 - p.pad_t;                                                                                      \
    const int HB = S * (R - 1) + 3, QB = HB * P;                                                                            \
    const int npt = (QB + 15) >> 4;                                                                                         \
    const int Po = Wo + 1, npo = (R * Po + 15) >> 4;                                                                        \
    const int nchunk = Ce / kBandC;                                                                                         \
    const int nti = npt > wave ? (npt - wave + 7) >> 3 : 0;                                                                 \
    const int nto = npo > wave ? (npo - wave + 7) >> 3 : 0

// Is this lane's pixel of input tile t a real image pixel?  Declares `real` (and the pixel's band row rb, image row ri and
// column c); SSD_BAND_XPIX is then the pixel's index in x, pixel 0 of the image if it is not real, so that the address
// stays valid.
#define SSD_BAND_REAL_PIXEL(t, P)                                                                 \
    const int tile = t * 8 + wave;                                                                \
    const int q = tile * 16 + l15;                                                                \
    const int rb = q / P, c = q - rb * P;                                                         \
    const int ri = ri0 + rb;                                                                      \
    const bool real = tile < npt && rb < HB && c < W && (unsigned)ri < (unsigned)H
#define SSD_BAND_XPIX (((long)img * H + (real ? ri : 0)) * W + (real ? c : 0))

// The wave's output tiles.  Declares ew, the E write address of this lane inside a tile slot (tile t adds t * 8 tiles *
// 1 KiB: row 8 + l15, 16-byte quad index XOR (row >> 1) & 3); ea[TO][3], the window origins in E (3 addresses per tile: the
// dy offsets are immediates because P % 8 == 0 keeps the swizzle); and opix[TO], (ro0 + rol) * Wo + co of a real output
// pixel, else -1.  The window origin qor is that of tap dy = dx = 0; -1 is the zero row.
#define SSD_BAND_OUT_WINDOWS(p, TO, S, P)                                             \
    const int ew = (8 + wave * 16 + l15) * 64 + ((g4 ^ ((l15 >> 1) & 3)) << 4);       \
    int ea[TO][3];                                                                    \
    int opix[TO];                                                                     \
    _Pragma("unroll") for (int t = 0; t < TO; ++t) {                                  \
        const int tile = t * 8 + wave;                                                \
        const int qo = tile * 16 + l15;                                               \
        const int rol = qo / Po, co = qo - rol * Po;                                  \
        const bool realo = tile < npo && rol < R && co < Wo;                          \
        opix[t] = realo ? (ro0 + rol) * Wo + co : -1;                                 \
        const int qor = realo ? (S * rol) * P + S * co - p.pad_l : 0;                 \
        _Pragma("unroll") for (int dx = 0; dx < 3; ++dx) {                            \
            const int e = 8 + qor + dx;                                               \
            ea[t][dx] = e * 64 + ((g4 ^ ((e >> 1) & 3)) << 4);                        \
        }                                                                             \
    }

// per-channel parameters -> LDS rows Ps[11][Ce] (expand shift, taps [9], depthwise shift); leading zero rows of both E buffers
__device__ __forceinline__ void band_stage_params(const FusedBlockParams& p, int tid, char* Es, int ebuf, float* Ps) {
    const int Ce = p.Ce;
    for (int u = tid; u < 11 * (Ce / 4); u += kBandThreads) {
        const int row = u / (Ce / 4), c4 = (u - row * (Ce / 4)) * 4;
        const float* src = row == 0 ? p.eh : row == 10 ? p.dh : p.wd + (long)(row - 1) * Ce;
        *reinterpret_cast<f32x4*>(Ps + row * Ce + c4) = *reinterpret_cast<const f32x4*>(src + c4);
    }
    if (tid < 64) *reinterpret_cast<f32x4*>(Es + (tid >> 5) * ebuf + (tid & 31) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// this lane's 4 channels of chunk i in parameter row `row` (0 expand shift, 1 .. 9 depthwise taps, 10 depthwise shift)
__device__ __forceinline__ f32x4 band_param4(const float* Ps, int Ce, int row, int i, int g4) {
    return *reinterpret_cast<const f32x4*>(Ps + row * Ce + i * kBandC + g4 * 4);
}
// Depthwise of one output tile: declares d, this lane's output pixel x 4 channels from nine ds_read_b128 of the E buffer eb
// at the tile's three window addresses ea3, taps w[9] and shift dh = the B fragment of the project.  (A macro like the
// declarations above: as a function it changed four of the split-bf16 kernels.)
// Measured and not kept (each within the +-3 % run-to-run noise, at a cost in registers): requesting tile
// t + 1's nine E vectors before tile t's arithmetic (LDS latency is not what the time goes to), scalar
// v_fma_f32 instead of v_pk_fma_f32.
#define SSD_BAND_DW_TILE(d, eb, ea3, w, dh, P)                                                             \
    f32x4 d = dh;                                                                                          \
    _Pragma("unroll") for (int dy = 0; dy < 3; ++dy)                                                       \
        _Pragma("unroll") for (int dx = 0; dx < 3; ++dx)                                                   \
            d += *reinterpret_cast<const f32x4*>(eb + ea3[dx] + dy * P * 64) * w[dy * 3 + dx];             \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) d[e] = __builtin_amdgcn_fmed3f(d[e], 0.0f, 6.0f)

// epilogue: y = acc + shift (+ x); lane = 4 consecutive output channels of its pixel
template <int TO, int NT>
__device__ __forceinline__ void band_epilogue(const FusedBlockParams& p, int img, int g4, const int (&opix)[TO],
                                              const f32x4 (&acc)[TO][NT]) {
    const long img_o = (long)img * p.Ho * p.Wo;
#pragma unroll
    for (int t = 0; t < TO; ++t) {
        if (opix[t] < 0) continue;
        float* yp = p.y + (img_o + opix[t]) * p.Cout + g4 * 4;
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
            if (ni * 16 + g4 * 4 >= p.Cout) continue;          // Cout = 24: the second channel tile is half empty
            f32x4 v = acc[t][ni] + *reinterpret_cast<const f32x4*>(p.ph + ni * 16 + g4 * 4);
            if (p.residual)                                     // stride 1, Cin == Cout: same layout as y
                v = v + *reinterpret_cast<const f32x4*>(p.x + (img_o + opix[t]) * p.Cout + ni * 16 + g4 * 4);
            *reinterpret_cast<f32x4*>(yp + ni * 16) = v;
        }
    }
}

}  // namespace ssd
