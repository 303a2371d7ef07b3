// Internal interface between the conv kernels (ssd_conv.hip / ssd_ops.hip) and the graph
// runner (ssd_net.hip).
#pragma once
#include <cmath>
#include <cstring>

#include "common.h"

namespace ssd {

// Fully resolved launch parameters of one dense convolution (implicit GEMM view:
// out[M = B*Ho*Wo, N = Cout] = X[M, K = kh*kw*Cin] * W[K, N]).
struct ConvParams {
    const float* in;
    const float* w;        // packed [Npad][Kpad]
    const short* w3;       // the same as four bf16 planes [4][Npad][Kpad]: the exact split h, m, l and the bf16 rounding r (ssd_conv3.hip) or nullptr
    const float* scale;    // [Cout] or nullptr (== 1)
    const float* shift;    // [Cout] or nullptr (== 0)
    const float* residual; // dense [M][Cout] or nullptr
    float* out;            // nullptr with `op` set: a plane-only output, no fp32 store (dense [M][Cout], Cout % 4 == 0)
    int B, H, W, Cin, Ho, Wo, Cout;
    int kh, kw, stride, dil, pad_t, pad_l;
    int K, Kpad, Npad;
    long M;
    long out_batch_stride, out_pixel_stride;
    // optional second destination: output channels n >= n_split go to out2 (column n - n_split)
    // with their own strides -- the fused SSD label+box head conv of one level.
    int n_split;           // 0: single destination
    float* out2;
    long out2_batch_stride, out2_pixel_stride;
    int vec_store2;
    int act;
    int vec_store;         // 1: float4 stores are aligned
    int split_k;           // >1: partial sums to `partial` [split][M][Cout], epilogue deferred
    float* partial;
    const float* wino_w;   // Winograd F(2x2,3x3) weights U [16][Npad][Cin] (ssd_wino.hip) or nullptr
    int bf16;              // the net's precision-1 mode: the cost model (conv_pick_config) may take the bf16 tiles
    // LDS-DMA tiles (csrc/ssd_convdma.hip): the INPUT as bf16 planes [np][B*H*W*Cin] (np = 3: exact split h, m, l of the
    // fp32 activation; np = 1: its bf16 rounding; np = 2: the fp16 pair of 2^8 x), `xp_plane` elements between planes; nullptr = not available
    const short* xp;
    long xp_plane;
    int xp_np;
    // ... and the OUTPUT also written as planes by the epilogue (dense [M][Cout] outputs only; Cout % 4 == 0) for the
    // LDS-DMA tiles of this layer's consumers; nullptr = fp32 only
    short* op;
    long op_plane;
    int op_np;
    // the two-plane fp16 tiles ("dmah_*", ssd_bf16x3.h): the weights as fp16 planes [2][Kpad / 32][Npad][32] of 2^k w
    // (launch_pack_f16x2) or nullptr, and the exact power of two 2^-(8 + k) the tile multiplies its accumulators by
    // before anything else (split-K partials included); the input planes are then xp_np = 2
    const short* wh;
    float acc_scale;
    // "dmah_*" with one k-step per barrier: 0 the three-stage ring (tiles whose three stages fit the LDS), 1 the two-stage
    // loop (net option dma_ring 0; ssd_conv_desc::dma_two_stage)
    int dma_two_stage;
};
// ConvParams::vec_store of these destinations: float4 stores into `out` are aligned
inline int conv_vec_store(const ConvParams& p) {
    return (((uintptr_t)p.out & 15) == 0) && (p.out_pixel_stride % 4 == 0) && (p.out_batch_stride % 4 == 0);
}

// One fused MobileNetV2 inverted-residual block (csrc/ssd_fused.hip).
struct FusedBlockParams {
    const float* x;
    float* y;
    const float* we;            // expand weights, packed [Ce][kpad_e]
    const float *es, *eh;       // folded expand BN [Ce]
    const float* wd;            // depthwise weights [9][Ce]
    const float *ds, *dh;       // folded depthwise BN [Ce]
    const float* wp;            // project weights, packed [npad_p][kpad_p]
    const float *ps, *ph;       // folded project BN [Cout]
    int residual;               // y += x (stride 1, Cin == Cout)
    int B, H, W, Cin, Ce, Cout, Ho, Wo, stride, pad_t, pad_l;
    int kpad_e, kpad_p, npad_p;
    int tiles_y, tiles_x;       // filled by the launcher
    // whole-image kernel (csrc/ssd_imgblock.hip): expanded-channel groups per image and their meeting point
    int bf16;                   // the net's precision-1 mode: bf16 forms of the band / whole-image kernels (operands rounded once to bf16, one MFMA per product)
    int groups;                 // G >= 1 (ImagePlan::groups)
    const short* we3;           // split-bf16 band kernel (csrc/ssd_band3.hip): bf16 planes of we [4][Ce][32] (h, m, l, r) ...
    const short* wp3;           // ... and of wp [4][npad_p][pairs][4][8]
    int bands;                  // row-band kernels (csrc/ssd_band_common.h): bands per image (filled by the launcher)
    float* slabs;               // [G][B][Ho*Wo][Cout] partial sums (G > 1)
    unsigned* tickets;          // [B] arrival counters, zero between launches
    float* e_out;               // optional: the expanded map [B,H,W,Ce] is ALSO written to HBM (block 13: SSD feature map 1)
    // optional bf16 planes of the outputs for the LDS-DMA conv tiles that read them (csrc/ssd_convdma.hip): y (written by
    // the direct epilogue / the combine launch) and the expanded map e_out; planes_np = 3 exact split, 1 bf16 rounding
    short* y_planes;
    long y_plane;
    short* e_planes;
    long e_plane;
    int planes_np;
    int e_planes_np;            // ... of the expanded map's planes (its consumers may take another family than y's: 2 = the fp16 pair)
    int planes_only;            // whole-image kernel: bit 0 = y, bit 1 = the expanded map leave as planes ONLY (no fp32 store; every
                                // consumer reads the planes).  The pointers y / e_out stay set: they also say which shapes a kernel takes
    int form2;                  // unused (kept: the struct is the kernels' argument); ImagePlan::second says which form runs
    // whole-image kernel, second form, bf16 == 2 -- the two-plane fp16 form (fp32 results, three fp16 MFMAs per product in
    // BOTH 1x1 GEMMs; ssd_bf16x3.h): we3 / wp3 are then the fp16 pairs [2][Ce][kpad_e] of 2^ke we and [2][npad_p][kpad_p] of
    // 2^kp wp, and these three exact powers of two: x is split as the pair of f16_xs x = 2^s x (s from the static bound of
    // the block's input: ssd_f16x2_input_exp), the expand accumulators are multiplied by f16_es = 2^-(s + ke), the depthwise
    // output is split as the pair of 2^8 d and the project accumulators are multiplied by f16_ps = 2^-(8 + kp)
    float f16_xs, f16_es, f16_ps;
};
// Fused MobileNetV2 stem (Conv1 -> expanded_conv_depthwise -> expanded_conv_project).
struct StemParams {
    const float* x;             // image [B,H,W,3]
    float* y;                   // [B,H1,W1,16]
    const float* w1;            // Conv1 weights packed [32][kpad1]
    const float *s1, *h1;       // folded Conv1 BN [32]
    const float* wd;            // depthwise weights [9][32]
    const float *sd, *hd;
    const float* wp;            // project weights packed [16][kpadp]
    const float *sp, *hp;       // folded project BN [16]
    int B, H, W, H1, W1, pad_t, pad_l, kpad1, kpadp;
    int tiles_y, tiles_x;
    int bf16;                   // the net's precision: 1 = Conv1 / project operands rounded once to bf16
};
// Depthwise 3x3 + BN + ReLU6 -> project 1x1 + BN (+ residual) of one MobileNetV2 block
// (csrc/ssd_dwproj.hip); BN scales are folded into wd / wp by the caller.
struct DwProjParams {
    const float* e;             // expanded activations [B,H,W,Ce] (after expand BN + ReLU6)
    const float* wd;            // depthwise weights [9][Ce], BN scale folded in
    const float* dh;            // depthwise BN shift [Ce]
    const float* wp;            // project weights packed [npad_p][kpad_p], BN scale folded in
    const float* ph;            // project BN shift [Cout]
    const float* res;           // residual [B,Ho,Wo,Cout] or nullptr
    float* y;                   // [B,Ho,Wo,Cout]
    int B, H, W, Ce, Cout, Ho, Wo, stride, pad_t, pad_l;
    int kpad_p, npad_p;
    int tiles_y, tiles_x;       // filled by the launcher
    int bf16;                   // the net's precision-1 mode: project on the bf16 matrix cores (operands rounded once, fp32 accumulation)
};
bool dwproj_supported(const DwProjParams& p);
int launch_dwproj(DwProjParams p, hipStream_t st);
bool stem_supported(const StemParams& p);
int launch_stem(StemParams p, hipStream_t st);
bool fused_block_supported(const FusedBlockParams& p);
int launch_fused_block(FusedBlockParams p, hipStream_t st);
bool band3_block_supported(const FusedBlockParams& p);
size_t band3_we_shorts(int Ce);
size_t band3_wp_shorts(int npad_p, int Ce);
int launch_band3_pack(const float* we, int Ce, int Cin, int kpad_e, short* we3, const float* wp, int npad_p, int kpad_p,
                      short* wp3, hipStream_t st);
int launch_band3_block(FusedBlockParams p, hipStream_t st);
bool band_block_supported(const FusedBlockParams& p);
int launch_band_block(FusedBlockParams p, hipStream_t st);
// ---- whole-image kernel (ssd_imgblock.hip, ssd_imgblock2.hip): what the net asks for one block at one batch ...
struct ImageAsk {
    int precision;              // the net's: 0 fp32 results, 1 the bf16 mode
    bool split;                 // fp32 net: the split-bf16 form (table line `image 2`)
    bool second;                // option image_v2: the second code form where it has the block's geometry
    bool pairs;                 // option image_f16x2 and the block's fp16 weight pairs exist: the two-plane fp16 form
    bool ticket;                // option image_ticket: the groups combine inside the launch
    bool slabs;                 // the slab workspace exists (without it: one group)
    long lanes;                 // images in flight: B * lanes_hint
};
// ... and what runs: every choice between the kernels' forms is made by image_block_plan, nowhere else
struct ImagePlan {
    int form;                   // FusedBlockParams::bf16 as the kernel reads it: 0 fp32 MFMA, 1 bf16 mode, 2 fp16 pair, 3 split-bf16
    bool second;                // the second code form (ssd_imgblock2.hip)
    int groups;                 // expanded-channel groups per image
    size_t lds;                 // dynamic LDS bytes
    const void* fn;             // the kernel and its block size
    int threads;
    bool ticketed;              // groups > 1 meet at FusedBlockParams::tickets inside the launch ...
    bool combine;               // ... or in image_combine_kernel, a second launch
};
bool image_block_supported(const FusedBlockParams& shape);
int image_block_groups(const FusedBlockParams& shape, long lanes);
size_t image_block_slab_floats(const FusedBlockParams& shape, int B);
// `shape`: the block as fused_shape leaves it (bf16 = the net's precision).  SSD_E_UNSUPPORTED where no kernel takes it
int image_block_plan(const FusedBlockParams& shape, const ImageAsk& ask, ImagePlan* plan);
bool image_second_form(const FusedBlockParams& shape, int form, int groups, ImagePlan* plan);   // (image_block_plan's only)
// launches `plan` on parameters filled from it (bf16, groups, tickets, the form's weight planes): no choice, no fallback
int launch_image_block(const FusedBlockParams& p, const ImagePlan& plan, hipStream_t st);

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
inline int conv_kpad(int K) { return round_up(K, 32); }
inline int conv_npad(int Cout) { return round_up(Cout, 16); }

// ---- dense-conv tile families ----------------------------------------------------------------------------------------
// A config id names one tile of one FAMILY.  Each family lives in its own file and exports one `extern const ConvFamily`;
// ssd_conv.hip lists them in kFamilies[] (in ConvFamilyId order = config id order: a family's ids are one contiguous range,
// direct_valu is the last id) and every conv_* function below resolves `cfg` to (family, index in the family) through that
// list.  Adding a family = define its ConvFamily in its file + one ConvFamilyId + one kFamilies[] line.
enum ConvFamilyId { CF_NONE = -1, CF_MFMA, CF_WINO, CF_SKINNY, CF_MFMA3, CF_BF16, CF_DMA3, CF_DMAB, CF_DMAH, CF_DIRECT };
// ConvFamily::traits
enum : unsigned {
    // what the tiles read (conv_config_reads): the fp32 activation `in`, or the planes `xp` -- bf16 planes (xp_np = 3 / 1)
    // or the fp16 pair (xp_np = 2, weights `wh`)
    CONV_READS_FP32 = 0, CONV_READS_PLANES = 1, CONV_READS_F16X2 = 2, CONV_READS_MASK = 3,
    // which nets may choose the family (conv_config_allowed): fp32 nets never take the bf16 (one-product) tiles; bf16 nets take
    // them instead of the split-bf16 / Winograd tiles (the fp32-MFMA and skinny tiles serve the small tail layers in both
    // modes: more accurate than asked for)
    CONV_NET_FP32 = 4, CONV_NET_BF16 = 8,
    CONV_WRITES_PLANES = 16,     // the epilogue (conv_epilogue / splitk_reduce_kernel) honours ConvParams::op
    CONV_SPLITK_REDUCE = 32,     // split_k > 1: the tiles leave partial sums, launch_splitk_reduce follows
};
struct ConvFamily {
    ConvFamilyId id;
    int (*count)();
    const char* (*name)(int i);
    bool (*valid)(int i, const ConvParams& p);        // alignment / shape constraints
    long (*grid_blocks)(int i, const ConvParams& p);  // blocks of the un-split grid
    int (*k_tiles)(int i, const ConvParams& p);       // K tiles per block without split
    int (*launch)(const ConvParams& p, int i, hipStream_t st);   // the kernel only, of a config conv_launch found valid
    unsigned traits;
};
// (host data: a definition sits under #ifndef __HIP_DEVICE_COMPILE__, or the device pass would emit the constant with its
// pointers to host functions)
extern const ConvFamily kConvMfma, kConvDirect;              // ssd_conv.hip
extern const ConvFamily kConvWino;                           // ssd_wino.hip: Winograd F(2x2, 3x3)
extern const ConvFamily kConvSkinny;                         // ssd_skinny.hip: small-M / long-K convs, the K split inside the workgroup
extern const ConvFamily kConvMfma3, kConvBf16;               // ssd_conv3.hip: split-bf16 tiles and their bf16 (one-product) forms
extern const ConvFamily kConvDma3, kConvDmab, kConvDmah;     // ssd_convdma.hip: LDS-DMA tiles over activation planes (np = 3, 1, 2)

int conv_num_configs();
const char* conv_config_name(int cfg);
int conv_config_by_name(const char* name);                 // the config id a tuning table's word names; -1: none
ConvFamilyId conv_config_family(int cfg);                  // (CF_NONE: no config id)
// true if config `cfg` can run these parameters
bool conv_config_valid(int cfg, const ConvParams& p);
bool conv_config_allowed(int cfg, int precision);          // may a net of this precision (0 fp32, 1 bf16) choose it?
int conv_config_reads(int cfg);                            // CONV_READS_*
bool conv_config_is_dma(int cfg);                          // reads planes: any of the three LDS-DMA families
bool conv_config_is_dmah(int cfg);                         // ... the fp16 pair
int conv_dmah_twin(int cfg);                               // the "dma3_*" config of a "dmah_*" config's tile
bool conv_config_writes_planes(int cfg, const ConvParams& p);
int conv_pick_config(const ConvParams& p);                 // heuristic
long conv_grid_blocks(int cfg, const ConvParams& p);
int conv_k_tiles(int cfg, const ConvParams& p);
int conv_launch(const ConvParams& p, int cfg, hipStream_t st);

int fill_conv_params(const ssd_conv_desc* d, ConvParams* p);   // geometry + validation
int launch_splitk_reduce(const ConvParams& p, hipStream_t st);
// 1x1 stride-1 unpadded: the implicit GEMM is a plain one (the GEMM1X1 kernel forms)
inline bool conv_is_gemm1x1(const ConvParams& p) {
    return p.kh == 1 && p.kw == 1 && p.stride == 1 && p.pad_t == 0 && p.pad_l == 0 && p.Ho == p.H && p.Wo == p.W;
}

// what other files need of a family beyond its ConvFamily
bool wino_applicable(const ConvParams& p);
size_t wino_weight_floats(int Cin, int Cout);
int launch_wino_pack(const float* hwio, int Cin, int Cout, int Npad, int row_off, float* U, hipStream_t st);
void mfma3_tile(int i, int* BM, int* BN);      // the cost model (conv_pick_config)
// "dmah_*" config j: every dma_* tile with one 32-wide k-step per barrier, then ("..._ks2") the tiles whose two stages fit
// the LDS with two; the tile's index in the "dma3_*" family
int dmah_tile_index(int j);
// fp16 weight planes of a packed [Npad][Kpad] matrix: *absmax_bits_dev receives max |w| as fp32 bits (a non-finite weight:
// >= 0x7f800000), zeroed by the caller; then the planes of 2^k w
int launch_absmax_bits(const float* packed, int K, int Cout, unsigned* absmax_bits_dev, hipStream_t st);
int launch_pack_f16x2(const float* packed, int K, int Cout, int k, short* planes, hipStream_t st, bool row_major = false);
// the exponent k of a layer's weight scale from max |w| (as fp32 bits, finite): max |w| 2^k in [2^13, 2^14) -- headroom
// below fp16's 65504, the low plane's subnormal grid 2^-24 far below the high plane's ulp; all-zero weights: 0
inline int conv_f16x2_weight_exp(unsigned absmax_bits) {
    float wmax;
    std::memcpy(&wmax, &absmax_bits, sizeof(float));
    if (!(wmax > 0.f)) return 0;
    int e = 0;
    (void)std::frexp(wmax, &e);          // wmax = f 2^e, f in [0.5, 1)
    return 14 - e;
}
inline size_t conv_f16x2_plane_shorts(int K, int Cout) { return (size_t)2 * conv_kpad(K) * conv_npad(Cout); }
int launch_split_planes(const float* x, long n, int C, int np, short* planes, long plane, hipStream_t st);
int launch_join_planes(const short* planes, long n, int C, int np, long plane, float* x, hipStream_t st);

int launch_dwconv3x3(const float* in, int B, int H, int W, int C, int stride, int pad_t, int pad_l,
                     int Ho, int Wo, const float* w, const float* scale, const float* shift, int act,
                     float* out, hipStream_t st);
int launch_maxpool(const float* in, int B, int H, int W, int C, int k, int stride, int pad_t, int pad_l,
                   int Ho, int Wo, float* out, hipStream_t st, short* planes = nullptr, long plane = 0, int np = 0);
int launch_l2norm(const float* in, long pixels, int C, const float* gamma, float* out, hipStream_t st,
                  short* planes = nullptr, long plane = 0, int np = 0);
int launch_softmax(const float* in, long rows, int L, float* out, hipStream_t st);
// (csrc/ssd_decode.hip) the post-processor behind its call record (ssd_decode.h); `who`: the entry point's name in the NULL
// checks' messages.  With `logits` and `counts_clean`, `ws` is a workspace of ssd_decode_nms_workspace_bytes(ws_batch, ...)
// whose candidate counters are zero: zeroed once at allocation; whatever the config, every call leaves them zero again
struct NmsCall;
int decode_nms(const NmsCall& call, const char* who, hipStream_t st);
int launch_pack_weights(const float* hwio, int K, int Cout, int Kpad, int Npad, float* packed, hipStream_t st);
// packed fp32 weights + room for their four bf16 planes (conv_split_planes points at them)
inline size_t conv_packed_floats(int K, int Cout) {
    const size_t n = (size_t)conv_kpad(K) * conv_npad(Cout);
    return n + 2 * n;
}
inline const short* conv_split_planes(const float* packed, int K, int Cout) {
    return reinterpret_cast<const short*>(packed + (size_t)conv_kpad(K) * conv_npad(Cout));
}
// after ALL launch_pack_weights calls of a buffer; planes slice-major [Kpad / 32][Npad][32] for the conv tiles (ssd_bf16x3.h),
// row_major: plain [Npad][Kpad] (the whole-image block kernels' expand / project matrices)
int launch_pack_split(float* packed, int K, int Cout, hipStream_t st, bool row_major = false);
// out[r][c] = in[r][c] * scale[r] (rows >= nvalid copied unscaled); out[r][c] = in[r][c] * scale[c]
int launch_scale_rows(const float* in, const float* scale, int rows, int nvalid, int cols, float* out, hipStream_t st);
int launch_scale_cols(const float* in, const float* scale, int rows, int cols, float* out, hipStream_t st);
int launch_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                   int C, float* scale, float* shift, hipStream_t st);

}  // namespace ssd
