/*
 * ssd_hip.h -- C ABI of libssd_hip.so: the MI355X (gfx950) replacement for the SSD
 * forward + decode/NMS hot path of FurkanOM/tf-ssd.
 *
 * The reference has no FFI boundary (it is Python on TensorFlow); the de-facto operator
 * API is its Python surface.  Each entry point below names the reference
 * interface it replaces (file:line relative to the reference root).  The Python host in
 * tf-ssd_amd/ binds these with ctypes (tf-ssd_amd/ssd_hip.py) and keeps the reference's
 * function names and signatures.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - Every `const float* / float* / int*` named *_dev or documented "device" is a device
 *     pointer owned by the caller (e.g. torch.Tensor.data_ptr()).  The library never
 *     frees caller memory.  Scratch comes from a caller-provided workspace whose size is
 *     reported by the matching *_workspace_bytes() query.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All compute
 *     entry points are asynchronous on that stream.
 *   - Return value: 0 = ok, negative = error (SSD_E_*); text via ssd_last_error()
 *     (thread-local).  Nothing aborts or throws across the ABI.
 *   - Layouts: activations NHWC fp32; boxes [y1,x1,y2,x2] fp32; Keras weight layouts
 *     (Conv2D HWIO, DepthwiseConv2D [kh,kw,C,1]) at the set_param boundary.
 */
#ifndef SSD_HIP_H
#define SSD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_OK 0
#define SSD_E_INVALID (-1)     /* bad argument (Python shim raises ValueError)          */
#define SSD_E_HIP (-2)         /* a HIP runtime call failed                              */
#define SSD_E_UNSUPPORTED (-3) /* valid in the reference but outside this build's limits */
#define SSD_E_STATE (-4)       /* object used in the wrong state (e.g. not finalized)    */

/* ---- library ------------------------------------------------------------------- */
const char* ssd_version(void);
const char* ssd_last_error(void);
/* Select + probe the device (must be gfx950).  Replaces utils/io_utils.py:54-61
 * (handle_gpu_compatibility) as the one-off per-process device hook. */
int ssd_init(int device);
/* A stream for keeping several batches in flight (DecoderModel lanes): created
 * hipStreamNonBlocking, so work on it is NOT ordered against the legacy NULL stream -- an event recorded on the
 * NULL stream (what torch's wait_stream does when the caller sits on the default stream) completes without
 * waiting for the lanes, and two lanes really overlap.  (torch.cuda.Stream() objects are ordered against
 * the NULL stream on this stack: recording the per-step dependency there serialised the lanes, measured.)
 * high_priority != 0: the device's greatest stream priority.  Returns NULL on failure (ssd_last_error). */
void* ssd_stream_create(int high_priority);
/* ... restricted to the compute units whose bits are set in cu_mask[0 .. words) (hipExtStreamCreateWithCUMask): lanes on
 * DISJOINT sets of XCDs run truly concurrently, each with a whole number of workgroup rounds of its own. */
void* ssd_stream_create_masked(const unsigned* cu_mask, int words);
int ssd_stream_destroy(void* stream);

/* ---- prior boxes: utils/bbox_utils.py:115-176 (A1-A3) ------------------------------
 * fmaps[levels], n_ars[levels] and ars[levels][n_ars[l]] are HOST arrays; out_dev is
 * [N,4] with N = sum f^2 * (n_ars+1).  Bit-exact vs the NumPy restatement. */
int ssd_priors_count(const int* fmaps, const int* n_ars, int levels);
int ssd_priors(const int* fmaps, const float* const* ars, const int* n_ars, int levels,
               float* out_dev, void* stream);

/* ---- box decode: utils/bbox_utils.py:61-85 (D1) -------------------------------------
 * deltas [B,N,4] (device), priors [N,4] (device) -> out [B,N,4].  var (HOST, 4 floats)
 * may be NULL; when given, deltas are multiplied by it first (models/decoder.py:41). */
int ssd_decode_boxes(const float* priors_dev, const float* deltas_dev, const float* var,
                     int B, int N, float* out_dev, void* stream);

/* ---- SSDDecoder.call: models/decoder.py:36-55 + utils/bbox_utils.py:3-25 (D2,D3) ----
 * and the [3P] tf.image.combined_non_max_suppression semantics.
 * deltas [B,N,4], probs [B,N,L], priors [N,4] device; var HOST[4].
 * Outputs (device, fully overwritten incl. zero padding rows): boxes [B,T,4] clipped to
 * [0,1], labels [B,T] (float class id), scores [B,T], valid [B] (int32).  kept_idx_dev
 * (nullable) [B,T] int32 receives the anchor index behind each row (-1 on padding).
 * Tie rule (TF leaves it unspecified): equal scores -> lower anchor index, then lower
 * class index. */
size_t ssd_decode_nms_workspace_bytes(int B, int N, int L, int max_per_class);
int ssd_decode_nms(const float* deltas_dev, const float* probs_dev, const float* priors_dev,
                   const float* var, int B, int N, int L, int max_per_class, int max_total,
                   float iou_thr, float score_thr,
                   float* boxes_dev, float* labels_dev, float* scores_dev, int* valid_dev,
                   int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- bbox_utils.non_max_suppression: utils/bbox_utils.py:3-25 (D2) -------------------
 * Generic combined NMS on already-decoded boxes [B,N,1,4] (q == 1) and scores [B,N,C];
 * output order as TF returns it: boxes, scores, classes, valid.  clip_boxes as TF. */
int ssd_combined_nms(const float* boxes_dev, const float* scores_dev, int B, int N, int C,
                     int max_per_class, int max_total, float iou_thr, float score_thr,
                     int clip_boxes, float* boxes_out_dev, float* scores_out_dev,
                     float* classes_out_dev, int* valid_dev, int* kept_idx_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Soft-NMS and class-agnostic suppression: the same two post-processors behind one config -------------------------
 * Soft-NMS (Bodla et al. 2017) in the form of tf.image.non_max_suppression_with_scores (its V5 kernel: the Gaussian weight
 * exp(-0.5 / soft_nms_sigma * iou^2), strict '>' everywhere); class_agnostic pools the classes of an image into ONE list,
 * so an anchor's box suppresses (or decays) its own other classes and an overlapping box of any class.
 *
 * Candidates: (anchor i, class c, score s) with s > score_threshold (strict: a NaN score is never a candidate); in the decoder
 * form after the "argmax == 0 zeroes the row" mask, class 0 of an unmasked row being an ordinary class -- exactly the
 * candidates of ssd_decode_nms / ssd_combined_nms.  One list per (image, class), or one per image when class_agnostic.
 *
 *   limit = per class: min(max_per_class, N)      class-agnostic: min(max_per_class, max_total, candidates)
 *   while selected < limit and a candidate is alive:
 *       w = the alive candidate with the largest CURRENT score (ties: lower anchor index, then lower class index)
 *       emit (w, current score of w); w leaves the list
 *       for every alive j:                            o = IoU(box[j], box[w]), the helper of the hard NMS, boxes unclipped
 *           SSD_NMS_HARD:      if o > iou_threshold: j leaves
 *           SSD_NMS_LINEAR:    if o > iou_threshold: s[j] = s[j] * (1.0f - o)
 *           SSD_NMS_GAUSSIAN:  s[j] = s[j] * expf((scale * o) * o)          scale = -0.5f / sigma, one float division (host)
 *           LINEAR / GAUSSIAN: if !(s[j] > score_threshold): j leaves
 *
 * Every operation is fp32 and rounded on its own (no contraction, correctly rounded division, expf and not the fast
 * intrinsic); a candidate receives its decays in selection order, oldest first -- that order defines the bits.  The emitted
 * scores are the decayed ones, non-increasing within a list.  The per-image merge is ssd_decode_nms's: the emitted rows sorted
 * by (score desc, anchor asc, class asc), the first max_total kept, zero padding, valid and kept_idx as there (a class-agnostic
 * list already is in that order).  The decoder forms clip the boxes to [0,1] whatever clip_boxes says (SSDDecoder always
 * does); ssd_combined_nms_cfg honours it.
 *
 * SSD_NMS_HARD with class_agnostic == 0 IS ssd_decode_nms / ssd_combined_nms: the same launches, the same bits.  Everything
 * else runs the selection kernel (csrc/ssd_decode.hip soft_nms_kernel): lists of up to ssd_nms_lds_candidates() candidates are
 * held in LDS, longer ones in the workspace.  SSD_E_INVALID: an unknown method, SSD_NMS_GAUSSIAN with sigma not finite or
 * <= 0, iou_threshold NaN or outside [0,1], and the size checks of ssd_decode_nms; its LDS limit on max_per_class still
 * answers SSD_E_UNSUPPORTED. */
#define SSD_NMS_HARD 0
#define SSD_NMS_GAUSSIAN 1
#define SSD_NMS_LINEAR 2
typedef struct ssd_nms_config {
    int method;             /* SSD_NMS_* */
    int class_agnostic;     /* 0: one list per (image, class); otherwise one list per image */
    int max_per_class;
    int max_total;
    int clip_boxes;         /* ssd_combined_nms_cfg only */
    float iou_threshold;
    float score_threshold;
    float sigma;            /* SSD_NMS_GAUSSIAN: TF's soft_nms_sigma */
} ssd_nms_config;
size_t ssd_nms_config_bytes(void);          /* sizeof(ssd_nms_config) of this library (for mirrors of the struct) */
int ssd_nms_lds_candidates(void);           /* the longest list the selection kernel keeps wholly in LDS */
size_t ssd_decode_nms_cfg_workspace_bytes(int B, int N, int L, const ssd_nms_config* cfg);
int ssd_decode_nms_cfg(const float* deltas_dev, const float* probs_dev, const float* priors_dev, const float* var,
                       int B, int N, int L, const ssd_nms_config* cfg, float* boxes_dev, float* labels_dev,
                       float* scores_dev, int* valid_dev, int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream);
int ssd_combined_nms_cfg(const float* boxes_dev, const float* scores_dev, int B, int N, int C, const ssd_nms_config* cfg,
                         float* boxes_out_dev, float* scores_out_dev, float* classes_out_dev, int* valid_dev,
                         int* kept_idx_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- pairwise IoU: utils/bbox_utils.py:27-59 (M1) -----------------------------------
 * boxes [N,4] (boxes_batched == 0, shared across the batch) or [B,N,4]; gt [B,G,4];
 * out [B,N,G].  No epsilon: 0/0 -> NaN exactly like the reference. */
int ssd_iou_map(const float* boxes_dev, int boxes_batched, const float* gt_dev,
                int B, int N, int G, float* out_dev, void* stream);

/* ---- box encode: utils/bbox_utils.py:87-113 (M3): bboxes [N,4], gt [B,N,4] -> [B,N,4] */
int ssd_encode_deltas(const float* bboxes_dev, const float* gt_dev, int B, int N,
                      float* out_dev, void* stream);

/* ---- target assignment: utils/train_utils.py:90-127 (M2) ----------------------------
 * priors [N,4], gt_boxes [B,G,4], gt_labels [B,G] int32 (device); var HOST[4].
 * deltas_out [B,N,4]; label_idx_out [B,N] int32; match_idx_out [B,N] int32 (argmax over
 * G, first max wins) -- both bit-exact; onehot_out (nullable) [B,N,L] fp32. */
int ssd_match_encode(const float* priors_dev, const float* gt_boxes_dev,
                     const int* gt_labels_dev, const float* var, float iou_thr,
                     int B, int N, int G, int L, float* deltas_out_dev,
                     int* label_idx_out_dev, int* match_idx_out_dev, float* onehot_out_dev,
                     void* stream);

/* ---- target assignment behind a strategy (csrc/ssd_match.hip) ------------------------
 * Inputs and the four outputs are ssd_match_encode's.  A ground-truth row is VALID iff its label is > 0 (padding rows:
 * box 0, label -1, anywhere among the rows).  IoU bits are ssd_iou_map's; a NaN IoU never wins a maximum and never passes
 * a comparison.  A background prior holds label_idx 0, the one-hot of class 0 and the encoding of the all-zero box divided
 * by the variances; a positive prior of box g holds label[g], match_idx g and the deltas of box g.
 *
 * SSD_MATCH_MAX_IOU: ssd_match_encode itself -- the same launch, the same bits (iou_threshold is its iou_thr).
 *
 * SSD_MATCH_BIPARTITE (SSD paper section 2.2, Caffe MultiBoxLoss), per image: U = the valid boxes, T = {} taken priors.
 *   repeat: among the pairs (i, g), g in U, i not in T, IoU(i, g) > 0, take the one with the largest IoU (ties: the
 *   smaller g, then the smaller i); forced[i] = g, g leaves U, i joins T; stop when no such pair is left.
 *   A forced prior is positive for its box whatever its IoU.  Every other prior follows ssd_match_encode's rule over all G
 *   columns: first maximum, positive iff strictly > iou_threshold, match_idx = that arg-max.
 *
 * SSD_MATCH_ATSS (Zhang et al., CVPR 2020), per image: priors [level_start[l], level_start[l+1]) are level l,
 *   level_start[0] == 0, level_start[n_levels] == N, non-decreasing.  Centres, priors and boxes alike, in fp32:
 *   cy = (y1 + y2) * 0.5f, cx = (x1 + x2) * 0.5f; d2 = fl(fl(dy * dy) + fl(dx * dx)), nothing fused.  For each valid box g:
 *   per level the candidates are the min(topk, level size) priors with the smallest (d2, i), lexicographic, a NaN d2 last;
 *   the list is ordered by level, then rank, n entries; with v_k the candidates' IoUs widened to double,
 *   mean = (sum v_k) / n, var = (sum (v_k - mean)^2) / (n - 1) (0 when n == 1), both sums in list order, in double, nothing
 *   fused; thr = mean + sqrt(var); candidate k is positive for g iff v_k >= thr and y1 < cy < y2 and x1 < cx < x2 (its own
 *   centre, the box's corners).  A prior positive for several boxes takes the one with the largest IoU (ties: the smaller g).
 *   Everything else is background with match_idx -1.  iou_threshold is unused; topk in 1..SSD_MATCH_MAX_TOPK.
 *
 * workspace_dev: ssd_match_encode_cfg_workspace_bytes(B, N, G, cfg) bytes, 16-byte aligned (0 bytes: may be NULL); the
 * query answers 0 for a config the entry would refuse.  SSD_E_INVALID, nothing launched: a NULL or unknown config, ATSS
 * with topk or level_start out of range, NULL pointers, a workspace that is too small.  SSD_E_UNSUPPORTED: G beyond
 * ssd_match_encode's LDS limit, B > 65535.  B == 0 or N == 0 launches nothing.  Results do not depend on scheduling: ownership is
 * resolved by integer maxima only. */
#define SSD_MATCH_MAX_IOU 0   /* the reference rule; what ssd_match_encode does */
#define SSD_MATCH_BIPARTITE 1 /* SSD paper: bipartite stage, then the reference rule */
#define SSD_MATCH_ATSS 2      /* adaptive training sample selection */
#define SSD_MATCH_MAX_LEVELS 8
#define SSD_MATCH_MAX_TOPK 64
typedef struct ssd_match_config {
    int strategy;           /* SSD_MATCH_* */
    float iou_threshold;    /* MAX_IOU, BIPARTITE */
    int topk;               /* ATSS */
    int n_levels;           /* ATSS: 1..SSD_MATCH_MAX_LEVELS */
    int level_start[SSD_MATCH_MAX_LEVELS + 1];
} ssd_match_config;
size_t ssd_match_encode_cfg_workspace_bytes(int B, int N, int G, const ssd_match_config* cfg);
int ssd_match_encode_cfg(const float* priors_dev, const float* gt_boxes_dev, const int* gt_labels_dev, const float* var,
                         const ssd_match_config* cfg, int B, int N, int G, int L, float* deltas_out_dev,
                         int* label_idx_out_dev, int* match_idx_out_dev, float* onehot_out_dev, void* workspace_dev,
                         size_t workspace_bytes, void* stream);

/* ---- detection scoring: utils/eval_utils.py:20-50 (N2), the per-image part of update_stats ----
 * det_boxes [B,T,4], det_labels [B,T] (float class id, 0 = padding row), det_scores [B,T],
 * gt_boxes [B,G,4], gt_labels [B,G] int32 (-1 = padding), all device.  Per image: best IoU and
 * FIRST arg-max over the G boxes (running maximum from -inf, strict >: a NaN IoU never wins; the
 * IoU bits are ssd_iou_map's); detections visited in descending best IoU, equal keys by ascending
 * index; label-0 rows leave no record; a record is a true positive iff best IoU >= iou_thr, its
 * label equals the label of its best box and no earlier-visited record took that box.
 * Outputs (device, fully overwritten, rows at or after the count are zero): rec_class_out [B,T]
 * int32, rec_score_out [B,T], rec_tp_out [B,T] int32 (1 = TP, 0 = FP) in visit order;
 * rec_det_out (nullable) [B,T] int32 the detection index behind each record; rec_count_out [B]
 * int32 records per image.
 * Supported: 0 <= T <= 1024, 1 <= G <= 256 (one workgroup per image, all keys in LDS); anything
 * else returns SSD_E_UNSUPPORTED before any launch.  B == 0 is a no-op. */
int ssd_eval_match(const float* det_boxes_dev, const float* det_labels_dev,
                   const float* det_scores_dev, const float* gt_boxes_dev,
                   const int* gt_labels_dev, int B, int T, int G, float iou_thr,
                   int* rec_class_out, float* rec_score_out, int* rec_tp_out, int* rec_det_out,
                   int* rec_count_out, void* stream);

/* ---- detection scoring by the standard protocols: the per-image matching of VOCdevkit's
 * VOCevaldet.m (SSD_EVAL_RULE_VOC) and of pycocotools' cocoeval.evaluateImg without crowd boxes
 * and area ranges (SSD_EVAL_RULE_COCO).  Inputs as ssd_eval_match, plus gt_ignore [B,G] uint8
 * (nullable = nothing ignored; VOC "difficult") and NT IoU thresholds iou_thrs_host (HOST).
 * The IoU is taken on the normalised corner boxes the decoder emits, WITHOUT the devkit's
 * "+1 pixel" on widths and heights; its bits are ssd_iou_map's.  A NaN IoU never matches and
 * never wins a maximum.
 * Per image the records are the rows with a non-zero label in DESCENDING SCORE, equal scores by
 * ascending detection index (-0 == +0; NaN scores last).  They are walked in that order,
 * separately for every class c and every threshold t; taken[t][g] is private to the threshold.
 *   VOC:  ovmax = -inf; over the image's class-c boxes in index order, ignored and taken ones
 *         included: if iou > ovmax: ovmax = iou, jmax = g (first maximum).  No class-c box or
 *         ovmax < t: FP.  Else ignore[jmax]: ignored.  Else not taken[t][jmax]: TP, take it.
 *         Else FP (duplicate).
 *   COCO: candidates = the class-c boxes, non-ignored first, then ignored, index order within.
 *         best = t, m = -1; per candidate g: skip if taken[t][g]; stop if m >= 0, m not ignored
 *         and g ignored; skip if !(iou >= best); else best = iou, m = g (a later tie wins).
 *         m < 0: FP.  Else take m; ignored if ignore[m] (an ignored box absorbs one detection
 *         per threshold), else TP.
 * Outputs (device, fully overwritten, zeros at and after the count): rec_class_out [B,T] int32,
 * rec_score_out [B,T], rec_det_out (nullable) [B,T] int32, rec_state_out [B,NT,T] int8 (1 TP,
 * 0 FP, -1 ignored), rec_count_out [B] int32.  Deterministic: the same bits on every run.
 * Supported: 0 <= T <= 1024, 1 <= G <= 256, 1 <= NT <= 10 (one workgroup per image, everything
 * in LDS); anything else returns SSD_E_UNSUPPORTED before any launch.  B == 0 is a no-op. */
#define SSD_EVAL_RULE_VOC 0
#define SSD_EVAL_RULE_COCO 1
int ssd_eval_match_protocol(const float* det_boxes_dev, const float* det_labels_dev,
                            const float* det_scores_dev, const float* gt_boxes_dev,
                            const int* gt_labels_dev, const unsigned char* gt_ignore_dev,
                            int B, int T, int G, int rule, const float* iou_thrs_host, int NT,
                            int* rec_class_out, float* rec_score_out, int* rec_det_out,
                            signed char* rec_state_out, int* rec_count_out, void* stream);

/* ---- input pipeline: utils/data_utils.py:22-23 (N4) ---------------------------------------
 * tf.image.convert_image_dtype(uint8 -> float32, x 1/255) + tf.image.resize(bilinear, TF2
 * half-pixel centres, no antialias) in one kernel.  image_u8 [B,H,W,C] uint8 (device) ->
 * out [B,out_h,out_w,C] float32 in [0,1].  Images of different sizes go through
 * ssd_preprocess_ragged: one call per batch, bitwise the same values. */
int ssd_preprocess(const unsigned char* image_u8_dev, int B, int H, int W, int C, int out_h, int out_w,
                   float* out_dev, void* stream);

/* The ragged form: B uint8 [H_b,W_b,3] images of different sizes, packed in src_dev [src_bytes], to
 * out_dev [B,out_h,out_w,3] float32 in ONE launch; image b's result is bitwise what
 * ssd_preprocess(B = 1) writes for it.  desc_host and desc_dev are the same B descriptors in host
 * and in device memory (the host copy is checked before any launch; the kernel reads the device
 * copy).  No workspace; every output element is written once.
 * SSD_E_INVALID: NULL pointers, a src_offset that is negative or not a multiple of 16, an image
 * that does not lie inside [0, src_bytes).  SSD_E_UNSUPPORTED: C != 3, a side (H, W, out_h, out_w)
 * outside 1..16384, B > 65535.  B == 0 is a no-op. */
struct ssd_image_desc {
    long long src_offset; /* byte offset of the image in src_dev, a multiple of 16 */
    int H, W;
};
int ssd_preprocess_ragged(const unsigned char* src_dev, size_t src_bytes,
                          const struct ssd_image_desc* desc_host, const struct ssd_image_desc* desc_dev,
                          int B, int C, int out_h, int out_w, float* out_dev, void* stream);

/* ---- custom images: utils/data_utils.py:93-108 (PIL Image.resize(..., Image.LANCZOS) + convert_image_dtype) ----------
 * [3P] Pillow's 8-bit resampler (ImagingResample, 8bpc), reproduced bit for bit: a separable two-pass filter in 22-bit
 * fixed point.  Horizontal pass first (skipped when W == out_w), vertical pass second (skipped when H == out_h), each
 *     u8 = clamp((2^21 + sum_x px[xmin + x] * k[x]) >> 22, 0, 255),  x in [0, xmax)        (int32, arithmetic shift)
 * with a uint8 intermediate between them; then out = (float)u8 * (float)(1.0 / 255.0), what ssd_preprocess writes at
 * equal sizes.  The coefficients are the caller's (float64 on the host, as Pillow computes them:
 * utils/data_utils.lanczos_coefficients): per axis and (in, out) pair a table bounds [out][2] int32 = {xmin, xmax} and
 * k [out][ksize] int32, anywhere in tables_dev [tables_ints] int32.
 * One call resizes B images of DIFFERENT sizes (uint8 [H,W,3], packed at desc[b].src_offset of src_dev [src_bytes]) into
 * out_dev [B,out_h,out_w,3] float32 and, when out_u8_dev is not NULL, out_u8_dev [B,out_h,out_w,3] uint8.  desc_host and
 * desc_dev are the same B descriptors in host and in device memory (the host copy sizes the grids and is checked; the
 * kernels read the device copy).  h_* are ignored when W == out_w, v_* when H == out_h.  tmp_offset: where the image's
 * intermediate (H rows of ssd_resize_lanczos_pitch(out_w) bytes) lives in the workspace, a multiple of 16, images not
 * overlapping (ignored when W == out_w); ssd_resize_lanczos_workspace_bytes is the size when they are packed in order,
 * each rounded up to 16 bytes.
 * Supported: C == 3, every side (H, W, out_h, out_w) in 1..16384, B <= 65535; anything else returns SSD_E_UNSUPPORTED
 * before any launch.  B == 0 is a no-op.  Table rows are clipped to the image inside the kernels. */
struct ssd_resize_desc {
    long long src_offset; /* byte offset of the image in src_dev                                       */
    long long tmp_offset; /* byte offset of its intermediate in the workspace                          */
    int H, W;
    int h_bounds, h_k, h_ksize; /* int32 offsets into tables_dev of bounds [out_w][2], k [out_w][h_ksize] */
    int v_bounds, v_k, v_ksize; /* ... of bounds [out_h][2], k [out_h][v_ksize]                           */
};
int ssd_resize_lanczos_pitch(int out_w);
size_t ssd_resize_lanczos_workspace_bytes(const struct ssd_resize_desc* desc_host, int B, int out_h, int out_w);
int ssd_resize_lanczos(const unsigned char* src_dev, size_t src_bytes, const int* tables_dev, size_t tables_ints,
                       const struct ssd_resize_desc* desc_host, const struct ssd_resize_desc* desc_dev, int B, int C,
                       int out_h, int out_w, float* out_dev, unsigned char* out_u8_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);

/* ---- JPEG decoding: what PIL.Image.open(...).convert("RGB") does for the reference (utils/data_utils.py:93-108 and the
 * tfds VOC reader), for baseline files, split in two.  [3P] libjpeg-turbo's arithmetic (the decoder inside Pillow),
 * restated from its published algorithms; every stage is integer, so the bytes are Pillow's exactly.
 *
 * HOST HALF (ssd_jpeg_parse, ssd_jpeg_entropy_decode): marker parsing and Huffman decoding.  Plain C++: no HIP call, no
 * device needed, no global state, thread-safe (the error text is thread-local); callers may run them on many threads.
 * No byte outside [data, data + n) is read and none outside [coef_out, coef_out + coef_bytes) is written, whatever the
 * file holds.
 *   Supported: SOF0 (baseline, 8-bit), ONE interleaved scan, Huffman tables from any number of DHT segments (codes up to 16
 *   bits), byte stuffing, DRI / RSTn (the counter wraps past 7), APPn / COM segments (skipped); 1 component (grey) or 3
 *   components that libjpeg's rules call YCbCr (a JFIF marker; else Adobe transform != 0; else component ids other than
 *   'R','G','B'); chroma sampled 1x1 with luma 1x1, 2x1 or 2x2 (4:4:4, 4:2:2, 4:2:0); sides 1..16384.
 *   SSD_E_UNSUPPORTED (with a text): progressive, arithmetic, 12-bit, lossless and extended-sequential files, scans that
 *   do not hold all components in frame order, any other sampling (4:4:0, 4:1:1, ...), RGB / CMYK / YCCK files, table
 *   indices above 3, sides above 16384.
 *   SSD_E_INVALID: a truncated or damaged header, a table a component needs and the file does not define, a code that is
 *   not in its Huffman table, a coefficient index past 63, a missing or wrong restart marker, data that ends before the
 *   last MCU, an info that does not describe this stream, a coef_out that is too small.
 * Coefficient storage of one image: the components' planes one after the other (coef_offset[c], bytes), every plane
 * padded to whole MCUs: blocks_h[c] x blocks_w[c] blocks in raster order, 64 int16 per block in NATURAL (de-zigzagged)
 * order, still quantised.  Blocks the stream never reaches stay zero.  quant[c] is component c's quantisation table in the
 * same natural order.  A one-component file is laid out as 1x1-sampled whatever its frame header says.
 * coef_out may be pinned memory: the decode then lands in the staging buffer of the upload. */
struct ssd_jpeg_info {
    int width, height, components;              /* components: 1 or 3                                         */
    int h_samp[3], v_samp[3], quant_index[3];   /* per component: sampling factors, the file's table index    */
    int restart_interval;                       /* MCUs between RSTn markers, 0: none                         */
    int mcus_x, mcus_y;
    int blocks_w[3], blocks_h[3];               /* the padded plane of each component, in 8x8 blocks          */
    int reserved;
    long long coef_offset[3];                   /* byte offset of each component's plane in the storage       */
    long long coef_bytes;                       /* bytes of coefficient storage the image needs               */
    unsigned short quant[3][64];                /* per component, natural order                               */
};
int ssd_jpeg_parse(const unsigned char* data, size_t n, struct ssd_jpeg_info* out);
int ssd_jpeg_entropy_decode(const unsigned char* data, size_t n, const struct ssd_jpeg_info* info, short* coef_out,
                            size_t coef_bytes);

/* DEVICE HALF (ssd_jpeg_decode): coefficients -> uint8 [H_b,W_b,3] RGB for a ragged batch of B images, one call, two
 * launches, asynchronous on `stream`; the pixels never exist in host memory.  packed_dev [bytes] holds, per image, its
 * coefficient storage (kind SSD_JPEG_COEFFICIENTS: the layout above for components / h_samp x v_samp luma sampling, the
 * sizes derived from H, W and the sampling exactly as ssd_jpeg_parse derives them; quant_offset: 3 x 64 uint16, natural
 * order, one table per component) or its decoded pixels (kind SSD_JPEG_RAW: uint8 [H,W,3] at coef_offset -- an image
 * the host had to decode itself, copied through by the same call so a batch may mix both kinds).  The output images are
 * packed in rgb_dev [rgb_bytes] at out_desc[b].src_offset: a following ssd_preprocess_ragged / ssd_resize_lanczos reads
 * them in place.  desc_host / desc_dev and out_desc_host / out_desc_dev are the same descriptors in host and device
 * memory (the host copies are checked and size the grids; the kernels read the device copies).
 * Workspace: the uint8 component planes between the launches, (blocks of all components) x 64 bytes per coefficient image
 * at plane_offset; ssd_jpeg_decode_workspace_bytes is the size when they are packed in order, each rounded up to 16.
 * block_start / item_start: the running sums over the batch of 8x8 blocks (raw images: 0) and of ceil(H*W / 4) -- the
 * two kernels index ONE space each over the whole batch, so small and large images share a grid.
 * Arithmetic (int32 throughout):
 *   IDCT       JDCT_ISLOW: dequantise (coef * quant), column pass then row pass of the 8-point Loeffler-Ligtenberg-
 *              Moschytz flow graph with 13-bit constants (FIX_0_298631336 = 2446 ... FIX_3_072711026 = 25172), PASS1_BITS =
 *              2: pass 1 descales by 11 bits, pass 2 by 18, each (v + 2^(n-1)) >> n.
 *   range      sample = T[(v >> 18 after rounding) & 1023] with libjpeg's post-IDCT table as a function of the masked
 *              index i: i < 128 -> i + 128, i < 512 -> 255, i < 896 -> 0, else i - 896.  It WRAPS for values far out of
 *              range (reachable at quality 1 and 100); it is not a clamp.
 *   upsampling "fancy" triangle filters over the cw x ch = ceil(W*h/hmax) x ceil(H*v/vmax) REAL samples of a chroma plane.
 *              h2v1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2, out[0] = s[0],
 *              out[2cw-1] = s[cw-1].  h2v2: t[i] = 3 near[i] + far[i] with near = row y>>1 and far = the row above (even
 *              y) or below (odd y), the first and the last REAL row replicated past the edges; out[2i] = (3 t[i] + t[i-1]
 *              + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4, out[0] = (4 t[0] + 8) >> 4, out[2cw-1] = (4 t[cw-1] + 7)
 *              >> 4.  cw <= 2: plain replication, as the library chooses.
 *   colour     R = clamp(Y + ((91881 Cr' + 32768) >> 16)), B = clamp(Y + ((116130 Cb' + 32768) >> 16)),
 *              G = clamp(Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16)) with Cb' = Cb - 128, Cr' = Cr - 128; grey: R = G =
 *              B = Y, as convert("RGB") does.
 * SSD_E_INVALID, nothing launched: NULL pointers, packed_dev / rgb_dev / workspace_dev not 16-byte aligned, a kind other
 * than the two, offsets that are negative or no multiple of 16, regions outside their buffer, outputs or planes that
 * overlap or are out of order, an output descriptor of another size, wrong running sums.  SSD_E_UNSUPPORTED, nothing
 * launched: a side outside 1..16384, components / sampling other than above, B > 65535, more than 2^31 blocks or
 * items.  B == 0 is a no-op.  Never launched on coefficients the entropy decoder refused. */
#define SSD_JPEG_COEFFICIENTS 0
#define SSD_JPEG_RAW 1
struct ssd_jpeg_desc {
    long long coef_offset;  /* byte offset in packed_dev of the coefficient storage (or the raw pixels), a multiple of 16 */
    long long quant_offset; /* ... of the three quantisation tables, a multiple of 16 (ignored for raw pixels)           */
    long long plane_offset; /* byte offset in the workspace of the component planes, a multiple of 16 (ignored for raw)  */
    int kind;               /* SSD_JPEG_COEFFICIENTS or SSD_JPEG_RAW                                                      */
    int H, W, components;   /* components 1 or 3 (ignored for raw)                                                        */
    int h_samp, v_samp;     /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for one component)                                     */
    int block_start, item_start;
};
size_t ssd_jpeg_decode_workspace_bytes(const struct ssd_jpeg_desc* desc_host, int B);
int ssd_jpeg_decode(const unsigned char* packed_dev, size_t bytes, const struct ssd_jpeg_desc* desc_host,
                    const struct ssd_jpeg_desc* desc_dev, int B, unsigned char* rgb_dev, size_t rgb_bytes,
                    const struct ssd_image_desc* out_desc_host, const struct ssd_image_desc* out_desc_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- JPEG encoding: PIL.Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s) for uint8 [H,W,3] RGB, the mirror
 * image of the decoder above, split at the same place.  [3P] libjpeg-turbo's baseline encoder (the one inside Pillow),
 * restated from its published algorithms; every stage is integer, so the bytes are Pillow's exactly.
 *
 * DEVICE HALF (ssd_jpeg_forward): uint8 [H_b,W_b,3] RGB -> quantised int16 coefficients for a ragged batch of B images, one
 * call, two launches, asynchronous on `stream`.  Image b is read at src_offset of rgb_dev [rgb_bytes] (any alignment: the
 * [B,H,W,3] tensor ssd_draw_detections writes is the case src_offset = b*H*W*3) and written at coef_offset of coef_dev
 * [coef_bytes] in exactly the coefficient storage of struct ssd_jpeg_info for 3 components with h_samp x v_samp luma
 * sampling (every block of the padded planes is written; only the REAL blocks, ceil(cw/8) x ceil(ch/8) of a component of
 * cw x ch real samples, are specified, and the host half reads no other).  quant_offset: 2 x 64 uint16 in tables_dev
 * [tables_bytes], natural order, luma then the table Cb and Cr share.  desc_host / desc_dev are the same descriptors in
 * host and device memory (the host copy is checked and sizes the grids; the kernels read the device copy).
 * Workspace: the uint8 component planes between the launches, (blocks of all components) x 64 bytes per image at
 * plane_offset; ssd_jpeg_forward_workspace_bytes is the size when they are packed in order, each rounded up to 16.
 * block_start / item_start: the running sums over the batch of 8x8 blocks and of 16 x mcus_x x mcus_y (an item is four
 * chroma samples) -- the two kernels index ONE space each over the whole batch, so small and large images share a grid.
 * Arithmetic (int32 throughout), with FIX(x) = int(x * 65536 + 0.5):
 *   colour     Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16,
 *              Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16,
 *              Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16.
 *   edges      the last real column is replicated out to the MCU width BEFORE downsampling.  The last real row is
 *              replicated only up to a whole row group (a multiple of v_samp); after downsampling the last DOWNSAMPLED row
 *              is replicated to the MCU height (padding the input rows to the MCU height first gives other chroma whenever
 *              H is not a multiple of 8 v_samp).
 *   downsample h2v1: (a + b + bias) >> 1, bias 0, 1, 0, 1, ... by output column; h2v2: (a + b + c + d + bias) >> 2, bias
 *              1, 2, 1, 2, ...
 *   FDCT       samples - 128; JDCT_ISLOW forward: row pass then column pass of the 8-point Loeffler-Ligtenberg-Moschytz
 *              flow graph with the decoder's 13-bit constants, PASS1_BITS = 2: rows, DC terms << 2, the others descaled by
 *              11 bits; columns, DC terms (v + 2) >> 2, the others descaled by 15; each descale (v + 2^(n-1)) >> n.
 *   quantise   sign(d) * ((|d| + 4 q) / (8 q)), a true integer division.
 * SSD_E_INVALID, nothing launched: NULL pointers, tables_dev / coef_dev / workspace_dev not 16-byte aligned, offsets that
 * are negative or (coef, quant, plane) no multiple of 16, regions outside their buffer, coefficients or planes that
 * overlap or are out of order, wrong running sums.  SSD_E_UNSUPPORTED, nothing launched: a side outside 1..16384, a
 * sampling other than 1x1, 2x1, 2x2, B > 65535, more than 2^31 blocks or items.  B == 0 is a no-op. */
struct ssd_jpeg_enc_desc {
    long long src_offset;   /* byte offset of the image's pixels in rgb_dev                                              */
    long long coef_offset;  /* byte offset in coef_dev of its coefficient storage, a multiple of 16                      */
    long long quant_offset; /* byte offset in tables_dev of its two quantisation tables, a multiple of 16                */
    long long plane_offset; /* byte offset in the workspace of its component planes, a multiple of 16                    */
    int H, W;
    int h_samp, v_samp;     /* luma sampling: 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0)                                    */
    int block_start, item_start;
};
size_t ssd_jpeg_forward_workspace_bytes(const struct ssd_jpeg_enc_desc* desc_host, int B);
int ssd_jpeg_forward(const unsigned char* rgb_dev, size_t rgb_bytes, const unsigned char* tables_dev, size_t tables_bytes,
                     const struct ssd_jpeg_enc_desc* desc_host, const struct ssd_jpeg_enc_desc* desc_dev, int B,
                     short* coef_dev, size_t coef_bytes, void* workspace_dev, size_t workspace_bytes, void* stream);

/* HOST HALF: the header and the Huffman coding.  Plain C++ under the rules of the decoder's host half: no HIP call, no
 * device needed, no global state, thread-safe (the error text is thread-local).
 * ssd_jpeg_quality_tables: jpeg_set_quality(quality, force_baseline) -- quality clamped to 1..100, scale = 5000 / q below
 *   50, else 200 - 2 q, every entry clamp((base * scale + 50) / 100, 1, 255) on the Annex K tables; out: 2 x 64 uint16,
 *   natural order, luma then chroma.
 * ssd_jpeg_encode_info: the ssd_jpeg_info of a width x height image with h_samp x v_samp luma sampling and these two
 *   tables -- what ssd_jpeg_parse returns for the stream ssd_jpeg_entropy_encode then writes.  SSD_E_UNSUPPORTED: a side
 *   outside 1..16384, another sampling; SSD_E_INVALID: a table entry outside 1..255.
 * ssd_jpeg_encode_bound: the size no stream of this info exceeds (0: an inconsistent info).
 * ssd_jpeg_entropy_encode: coef (the coefficient storage; only real blocks are read) -> the whole stream in out: SOI, the
 *   18-byte JFIF 1.01 APP0 (units 0, density 1:1), two DQT segments (zigzag order), SOF0 (component ids 1, 2, 3, tables 0,
 *   1, 1), four DHT segments (DC0, AC0, DC1, AC1: the Annex K tables), one interleaved SOS without restart markers, the
 *   entropy-coded data (0xFF stuffed, the last byte padded with 1-bits), EOI; *written = its size.  An MCU block beyond a
 *   component's real blocks is synthesised: all AC zero, the DC of the block emitted just before it in the same MCU.
 *   Nothing outside [out, out + out_bytes) is written.  SSD_E_INVALID: an info that is not what ssd_jpeg_encode_info fills
 *   in, an out that is too small for the stream (any size that holds it is enough), a DC difference beyond category 11
 *   or an AC coefficient beyond category 10 (outside baseline range). */
int ssd_jpeg_quality_tables(int quality, unsigned short* out);
int ssd_jpeg_encode_info(int width, int height, int h_samp, int v_samp, const unsigned short* tables, struct ssd_jpeg_info* out);
size_t ssd_jpeg_encode_bound(const struct ssd_jpeg_info* info);
int ssd_jpeg_entropy_encode(const short* coef, const struct ssd_jpeg_info* info, unsigned char* out, size_t out_bytes,
                            size_t* written);
/* ssd_jpeg_encode_header: everything ssd_jpeg_entropy_encode writes before the entropy-coded data (SOI through SOS, the
 *   same bytes: it is the function the coder itself calls); *written = SSD_JPEG_HEADER_BYTES, whatever the image.
 *   SSD_E_INVALID: NULL pointers, an inconsistent info, out_bytes below SSD_JPEG_HEADER_BYTES (nothing is written). */
#define SSD_JPEG_HEADER_BYTES 623
int ssd_jpeg_encode_header(const struct ssd_jpeg_info* info, unsigned char* out, size_t out_bytes, size_t* written);

/* DEVICE ENTROPY CODER (ssd_jpeg_pack): the coefficient storage of a ragged batch, exactly as ssd_jpeg_forward writes it
 * (three components, 1x1 / 2x1 / 2x2 luma sampling; only REAL blocks are read), -> the complete JPEG streams of the
 * batch, back to back in out_dev: stream b is out_dev[offsets_dev[b] : offsets_dev[b + 1]] (int32 [B + 1], offsets[0] =
 * 0), and its bytes are ssd_jpeg_entropy_encode's bit for bit: the header (copied from header_offset of packed_dev
 * [packed_bytes], SSD_JPEG_HEADER_BYTES bytes that ssd_jpeg_encode_header wrote), the stuffed Huffman data of one
 * interleaved scan with the Annex K tables, the last byte padded with 1-bits (a 0xFF made by the padding is stuffed),
 * EOI.  Dummy blocks of the last MCU column / row are synthesised (AC zero, a DC difference of zero).  One call, a fixed
 * number of launches (six kernels and two fills, whatever B and the sizes), asynchronous on `stream`; no workgroup waits
 * on another, every prefix sum is reduce-then-scan in separate launches, so the bytes do not depend on scheduling.
 *   blocks     ONE index space of emitted blocks over the batch (block_start: the running sum of mcus_x * mcus_y *
 *              (h_samp * v_samp + 2), the same number ssd_jpeg_forward counts).  Kernel 1 gives every block its bit
 *              length (the DC predictor is the DC of the block emitted before it in the same component, always a real
 *              block's value; ZRL for runs above 15; EOB only when zeros trail) and every 256 blocks their sum; kernel 2
 *              (one workgroup) scans the sums (64-bit: a batch may hold more than 2^32 bits) and finds every image's
 *              first bit; kernel 3 re-derives the codes and ORs them, as big-endian 32-bit words with atomic ORs (blocks
 *              share words; OR commutes), into the image's zeroed unstuffed stream.
 *   stuffing   the unstuffed stream of image b lives at 224 * block_start of the workspace (224 bytes hold the longest
 *              block, 1660 bits, and the padding).  Kernel 4 counts the 0xFF bytes of every 224-byte slot (the same index
 *              space), kernel 5 (one workgroup) scans them, sizes every stream (header + data + stuffing + EOI) and scans
 *              the sizes into offsets_dev; kernel 6 scatters every slot's bytes to their final place -- which already
 *              includes the batch-level offsets, so the output is compact without a host round trip -- and copies the
 *              header and the EOI.
 * status_dev (int32 [B]): 0, or for an image with a DC difference beyond category 11 (bit 0) or an AC coefficient beyond
 *   category 10 (bit 1) -- what ssd_jpeg_entropy_encode refuses -- nonzero; the content of that image's region is then
 *   unspecified (its size is still within its bound), and every other image of the batch is exact.
 * Workspace: ssd_jpeg_pack_workspace_bytes(desc_host, B) bytes (bit lengths, scan partials, the unstuffed streams at their
 *   worst case; 0 for an unusable batch); the call itself zeroes it on `stream`.
 * Nothing outside [out_dev, out_dev + out_bytes) is written; the bytes past offsets_dev[B] are left as they were.
 * SSD_E_INVALID, nothing launched: NULL pointers, coef_dev / packed_dev / out_dev / workspace_dev not 16-byte aligned,
 *   offsets_dev / status_dev not 4-byte aligned, offsets that are negative or no multiple of 16, regions outside their
 *   buffer, coefficients that overlap or are out of order, wrong running sums, a workspace that is too small, out_bytes
 *   below the sum of ssd_jpeg_encode_bound of the images, each rounded up to 16 (which rules out overflow by construction).
 * SSD_E_UNSUPPORTED, nothing launched: a side outside 1..16384, a sampling other than 1x1, 2x1, 2x2, B > 65535, a bound
 *   sum above 2^31 - 1 bytes (byte offsets are int32).  B == 0 is a no-op. */
struct ssd_jpeg_pack_desc {
    long long coef_offset;   /* byte offset in coef_dev of the image's coefficient storage, a multiple of 16             */
    long long header_offset; /* byte offset in packed_dev of its SSD_JPEG_HEADER_BYTES header bytes, a multiple of 16     */
    int H, W;
    int h_samp, v_samp;      /* luma sampling: 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0)                                   */
    int block_start;         /* running sum over the batch of the image's 8x8 blocks                                     */
    int reserved;            /* 0                                                                                        */
};
size_t ssd_jpeg_pack_workspace_bytes(const struct ssd_jpeg_pack_desc* desc_host, int B);
int ssd_jpeg_pack(const short* coef_dev, size_t coef_bytes, const unsigned char* packed_dev, size_t packed_bytes,
                  const struct ssd_jpeg_pack_desc* desc_host, const struct ssd_jpeg_pack_desc* desc_dev, int B,
                  unsigned char* out_dev, size_t out_bytes, int* offsets_dev, int* status_dev, void* workspace_dev,
                  size_t workspace_bytes, void* stream);

/* PNG ENCODER (ssd_png_encode): uint8 RGB images of a ragged batch, on the device, -> their finished PNG files, back to
 * back in out_dev: file b is out_dev[offsets_dev[b] : offsets_dev[b + 1]] (int32 [B + 1], offsets[0] = 0).  PNG is
 * lossless, so the contract is not another encoder's bytes: every decoder returns the input pixels, the stream is strictly
 * valid, and ssd_png_encode_host -- plain C++ from the same step functions (csrc/ssd_png_common.h) -- writes the same bytes.
 * A file is the 8-byte signature, IHDR (W, H, depth 8, colour type 2, compression 0, filter 0, interlace 0), one IDAT chunk
 * per segment, IEND; no ancillary chunks.
 *   filtered   F is H rows of 1 + 3 W bytes: the filter type, then the filtered bytes (bpp 3, zeros above row 0).  filter
 *              0..4 forces None / Sub / Up / Average / Paeth on every row; 5 (adaptive) takes per row the type whose
 *              filtered bytes have the least sum of min(v, 256 - v), ties to the lowest type.  Paeth: a on pa <= pb &&
 *              pa <= pc, else b on pb <= pc, else c.
 *   segments   F is cut every SSD_PNG_SEGMENT_BYTES bytes, whatever the rows; seg_start is the running sum over the batch
 *              of ssd_png_segments, row_start that of H: the kernels index ONE space of segments (and of rows).
 *   tokens     inside a segment a maximal run of n equal bytes is one literal, then the other n - 1 bytes in pieces of
 *              min(258, rest): a piece of 3 or more is a match of that length at distance 1, a piece of 1 or 2 that many
 *              literals.  Runs begin anew at a segment's first byte.
 *   block      one deflate block per segment: dynamic Huffman, or stored where that is not longer in whole bytes (ties go
 *              to stored).  A dynamic block that is not the image's last is followed by an empty stored block (000, zeros
 *              to the byte, 00 00 FF FF), which counts in the comparison, so every segment begins and ends on a byte; the
 *              image's last block has BFINAL and is padded with zeros.  HLIT = 29, HDIST = 0, HCLEN = 15 always.  Literal /
 *              length code: Huffman over the symbols that occur and 256, lengths <= 15.  Distance code: code 0 with length
 *              1.  Code-length code: lengths <= 7 over the sequence of the 286 + 1 lengths, in which a run of z zeros is
 *              symbol 18 (up to 138) while 11 or more are left, then 17 for 3..10, single zeros for 1..2; symbol 16 is not
 *              used.  Huffman: the two lightest of (weight, leaves before internal nodes, sorted by (weight, symbol));
 *              where the depth exceeds the limit, the counts per length are shortened as ITU-T T.81 K.3 does and handed
 *              out longest first to the rarest symbols (Kraft sum exactly 1; lengths that fit are left as they are).
 *   framing    the first segment's chunk data begins 78 9C, the last one's ends with the big-endian Adler-32 of F; every
 *              chunk carries the CRC-32 of its type and data.
 * One call, four launches whatever B and the sizes (filter, segment, scan, scatter), asynchronous on `stream`; no workgroup
 * waits on another, the prefix sums are a launch of their own, bits are ORed into zeroed words and histograms are integer
 * LDS atomics, so the bytes do not depend on scheduling.  Every RGB image is encodable: there is no per-image status.
 * ssd_png_segments / ssd_png_encode_bound: the IDAT chunks of an H x W image, and the size no file of it exceeds: signature,
 *   IHDR and IEND (45), per segment the chunk framing and a stored header (17), the bytes of F, and 6 (78 9C, Adler-32); 0
 *   for a side outside 1..16384.
 * Workspace: ssd_png_encode_workspace_bytes(desc_host, B) bytes (F, the finished chunk data per segment, sizes; 0 for an
 *   unusable batch).
 * Nothing outside [out_dev, out_dev + out_bytes) is written; the bytes past offsets_dev[B] are left as they were.
 * SSD_E_INVALID, nothing launched: NULL pointers, workspace_dev not 16-byte aligned, offsets_dev not 4-byte aligned, pixels
 *   outside rgb_dev, wrong running sums, a workspace that is too small, out_bytes below the sum of ssd_png_encode_bound.
 * SSD_E_UNSUPPORTED, nothing launched: a side outside 1..16384, B > 65535, a filter outside 0..5, a bound sum above
 *   2^31 - 1 bytes (byte offsets are int32).  B == 0 is a no-op.
 * ssd_png_encode_host: one image on the host (no HIP call, no global state, thread-safe), the same bytes; *written = the
 *   file's size.  SSD_E_INVALID: NULL pointers, out_bytes below the file's size (nothing is written; any size that holds
 *   the file is enough); SSD_E_UNSUPPORTED as above. */
#define SSD_PNG_SEGMENT_BYTES 16384
struct ssd_png_desc {
    long long src_offset;   /* byte offset of the image's pixels in rgb_dev, any alignment                                */
    int H, W;
    int filter;             /* 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth, 5 adaptive                                       */
    int seg_start;          /* running sum over the batch of ssd_png_segments                                            */
    int row_start;          /* running sum over the batch of H                                                           */
    int reserved;           /* 0                                                                                         */
};
int ssd_png_segments(int H, int W);
size_t ssd_png_encode_bound(int H, int W);
size_t ssd_png_encode_workspace_bytes(const struct ssd_png_desc* desc_host, int B);
int ssd_png_encode(const unsigned char* rgb_dev, size_t rgb_bytes, const struct ssd_png_desc* desc_host,
                   const struct ssd_png_desc* desc_dev, int B, unsigned char* out_dev, size_t out_bytes, int* offsets_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);
int ssd_png_encode_host(const unsigned char* rgb, int H, int W, int filter, unsigned char* out, size_t out_bytes, size_t* written);

/* PNG DECODER (ssd_png_parse, ssd_png_idat, ssd_png_decode): PNG files -> uint8 RGB pixels on the device, behind a host
 * inflate.  The contract is Pillow's: for every file ssd_png_parse accepts, whose zlib stream inflates to exactly
 * H * (1 + row_bytes) bytes and whose filter bytes are 0..4, the pixels equal PIL.Image.open(f).convert("RGB") bit for bit.
 * The format (colour type, depths -> RGB):
 *   2 RGB           8       the samples            |  16     the HIGH byte of each sample
 *   6 RGBA          8, 16   as RGB, alpha dropped
 *   0 grey          8       replicated to three channels  |  1, 2, 4   sample x 255, x 85, x 17, replicated
 *   4 grey + alpha  8, 16   (the high byte of) grey replicated, alpha dropped
 *   3 palette       1, 2, 4, 8   PLTE[index]; an index past the end of a short PLTE gives (0, 0, 0)
 * Ancillary chunks (tRNS, gAMA, text, ...) change nothing.  Refused, for the caller's other decoder: grey at 16 bits, Adam7
 * interlace, a side above 16384, animated files, unknown critical chunks, PLTE in a grey image (SSD_E_UNSUPPORTED); a bad
 * signature, chunk order, chunk length or CRC, a file that ends early, a missing PLTE for type 3, IDAT chunks that are not
 * consecutive, a missing IEND (SSD_E_INVALID).
 * HOST HALF.  Plain C++: no HIP call, no global state, thread-safe.
 *   ssd_png_parse walks the chunks, verifies every CRC and fills ssd_png_info: row_bytes = ceil(W * channels * depth / 8),
 *     filter_distance = max(1, channels * depth / 8), stream_bytes = H * (1 + row_bytes) (what inflate must return), the
 *     palette zero-padded to 256 entries, and where the zlib stream lies: idat_count consecutive IDAT chunks from byte
 *     first_idat of the file on, idat_bytes of payload in all.
 *   ssd_png_idat copies that payload, joined, to `out` (out_bytes >= idat_bytes).  Inflating it is the caller's business
 *     (zlib is no dependency of this library), and so is refusing a stream of another length or a filter byte above 4.
 *   ssd_png_decode_host: one image's inflated stream -> H * W * 3 bytes, the same arithmetic as the device in plain loops.
 *     SSD_E_INVALID: NULL pointers, filtered_bytes other than stream_bytes, a filter byte above 4, rgb_bytes too small.
 * DEVICE.  ssd_png_decode: one call per ragged batch, two launches whatever the batch (un-filter: Sub / Up / Average / Paeth
 * modulo 256, one wavefront per chain of dependent rows; convert: the table above), asynchronous on `stream`.  packed_dev
 * holds, each part at a multiple of 16 bytes, per image its filtered scanlines (src_offset; the images in ascending order,
 * not overlapping), for colour type 3 its 768-byte palette (palette_offset) and its chain list (chain_offset: int32 rows,
 * ascending, at which a chain begins: row 0 and every row whose filter byte is 0 or 1; rows outside 0..H are clamped, so a
 * wrong list gives wrong pixels, never an access outside the image).  Image b's H * W * 3 bytes go to rgb_dev + dst_offset (a
 * multiple of 16, ascending, not overlapping: the src_offset of the ssd_image_desc that ssd_preprocess_ragged and
 * ssd_resize_lanczos take); nothing else in rgb_dev is written.  chain_start / row_start / raw_offset: running sums over the
 * batch of chains, H and round16(H * row_bytes).  Workspace: ssd_png_decode_workspace_bytes(desc_host, B) (the unfiltered
 * rows; 0 for an unusable batch).
 * SSD_E_INVALID, nothing launched: NULL pointers, packed_dev / rgb_dev / workspace_dev not 16-byte aligned, a side below 1, a
 *   (colour type, depth) outside the table, offsets that are misaligned, outside their buffer or overlapping, chains outside
 *   1..H, wrong running sums, a workspace that is too small.  SSD_E_UNSUPPORTED, nothing launched: a side above 16384,
 *   B > 65535.  B == 0 is a no-op. */
struct ssd_png_info {
    int width, height, depth, color_type, channels, filter_distance, palette_entries, idat_count;
    long long row_bytes, stream_bytes, idat_bytes, first_idat;
    unsigned char palette[768];
};
struct ssd_png_dec_desc {
    long long src_offset;       /* the filtered scanlines in packed_dev: H rows of 1 + row_bytes bytes                  */
    long long palette_offset;   /* 768 bytes in packed_dev (colour type 3 only)                                          */
    long long chain_offset;     /* int32 [chains] in packed_dev                                                          */
    long long dst_offset;       /* the image's H * W * 3 bytes in rgb_dev                                                */
    long long raw_offset;       /* running sum over the batch of round16(H * row_bytes): its place in the workspace      */
    int H, W, depth, color_type;
    int chains;                 /* 1..H                                                                                  */
    int chain_start;            /* running sum over the batch of chains                                                  */
    int row_start;              /* running sum over the batch of H                                                       */
    int reserved;               /* 0                                                                                     */
};
int ssd_png_parse(const unsigned char* data, size_t n, struct ssd_png_info* out);
int ssd_png_idat(const unsigned char* data, size_t n, const struct ssd_png_info* info, unsigned char* out, size_t out_bytes);
int ssd_png_decode_host(const struct ssd_png_info* info, const unsigned char* filtered, size_t filtered_bytes, unsigned char* rgb,
                        size_t rgb_bytes);
size_t ssd_png_decode_workspace_bytes(const struct ssd_png_dec_desc* desc_host, int B);
int ssd_png_decode(const unsigned char* packed_dev, size_t packed_bytes, const struct ssd_png_dec_desc* desc_host,
                   const struct ssd_png_dec_desc* desc_dev, int B, unsigned char* rgb_dev, size_t rgb_bytes, void* workspace_dev,
                   size_t workspace_bytes, void* stream);

/* PNG INFLATE (ssd_png_inflate, ssd_png_inflate_host): the inflate in front of ssd_png_decode, on the device, for a ragged
 * batch.  The contract is the host inflater's: STATUS 0 IMPLIES that zlib, asked for one byte more than the image has
 * (Python: zlib.decompressobj().decompress(s, n + 1)), returns exactly the same n = H * (1 + row_bytes) bytes with the
 * stream at its end and no input left over, and that every filter byte is 0..4.  Any other status means "ask the host":
 * the image's bytes are then unspecified (inside its own regions).
 * The format: a zlib stream (RFC 1950: CM = 8, CINFO <= 7, FCHECK, no FDICT) of stored, fixed-Huffman and dynamic-Huffman
 * blocks (RFC 1951) in any mix, and its Adler-32.
 * ssd_png_inflate: one call per batch, two launches whatever the batch, asynchronous on `stream`, no workspace.
 *   1 inflate  one wavefront per stream.  The decode state is wave-uniform; a dynamic block's code tables are built in LDS
 *              by the whole wavefront; the 32 KB window is an LDS ring, so a back-reference is an LDS read (never a read of
 *              global memory this kernel wrote); a match of length L at distance D is copied by the lanes as
 *              out[p + l] = out[p - D + l % D]; each finished 16 KB half of the ring leaves in 16-byte stores and is folded
 *              into the Adler-32 in parallel.  status_dev[b] is written (0 or ONE bit below: the first cause met).
 *   2 chains   one workgroup per image reads the H filter bytes: one above 4 sets SSD_PNG_INFLATE_FILTER (only where kernel 1
 *              left 0); the rows 0 and those of type 0 or 1 go, ascending, to the first slots of the image's chain list and H
 *              goes to EVERY REMAINING ONE of its H slots, so an ssd_png_dec_desc with chains = H, the same chain_offset and
 *              src_offset = dst_offset decodes the image (a padded slot is the empty chain H..H).
 *   packed_dev holds, per image, each at a multiple of 16 bytes and none overlapping another: the joined IDAT payload
 *   (zlib_offset, zlib_bytes; read only, and no byte outside it is read), the H * (1 + row_bytes) bytes to write (dst_offset)
 *   and the int32[H] chain list to write (chain_offset).  Nothing else but status_dev[0..B) is written.
 * Stricter than zlib (refused here, accepted there; the host road then decides): a distance beyond the window the header
 *   declares (zlib checks only against the bytes produced); input left behind the Adler-32 (zlib reports it as unused data).
 * ssd_png_inflate_host: one stream in plain C++ from the same step functions: no HIP call, no global state, thread-safe; the
 *   same bytes in out[0..out_bytes) and the same status word as the device (filter bit included; out_bytes = H * (1 +
 *   row_bytes)).  Nothing outside out[0..out_bytes) is written.  SSD_E_INVALID: NULL pointers, row_bytes < 1, out_bytes no
 *   positive multiple of 1 + row_bytes.
 * SSD_E_INVALID, nothing launched: NULL pointers, packed_dev not 16-byte aligned, desc_dev not 8-byte or status_dev not
 *   4-byte aligned, H < 1, row_bytes < 1, zlib_bytes < 0, a region that is misaligned, outside packed_dev or overlapping
 *   another region of the batch, reserved != 0.  SSD_E_UNSUPPORTED, nothing launched: B > 65535; H * (1 + row_bytes) above
 *   SSD_PNG_INFLATE_MAX_STREAM.  B == 0 is a no-op.
 * The cap: one wavefront inflates a stream alone, and it is slow: 3.0 MB of output per second, measured on an MI355X on
 *   Pillow-written 500x375 photographs, smooth and noise alike (tests/bench_png_inflate.py leg (f): 189 ms for 562 875 bytes;
 *   DESIGN.md section 7, "PNG inflate on the device").  SSD_PNG_INFLATE_MAX_STREAM = 1 MiB keeps a stream at that rate to
 *   0.35 s, and leaves a stream of nothing but long codes room to be slower; a larger image is the host road's. */
#define SSD_PNG_INFLATE_HEADER         0x0001   /* CM, CINFO, FCHECK or FDICT                                             */
#define SSD_PNG_INFLATE_BLOCK_TYPE     0x0002   /* block type 3                                                           */
#define SSD_PNG_INFLATE_STORED         0x0004   /* a stored block whose LEN and NLEN disagree                             */
#define SSD_PNG_INFLATE_SYMBOLS        0x0008   /* HLIT > 286 or HDIST > 30                                               */
#define SSD_PNG_INFLATE_REPEAT         0x0010   /* a code-length repeat with nothing before it, or running past the lengths */
#define SSD_PNG_INFLATE_OVERSUBSCRIBED 0x0020   /* an over-subscribed code                                                */
#define SSD_PNG_INFLATE_INCOMPLETE     0x0040   /* an incomplete code other than one 1-bit code or (distances) none       */
#define SSD_PNG_INFLATE_NO_END         0x0080   /* no end-of-block code                                                   */
#define SSD_PNG_INFLATE_SYMBOL         0x0100   /* length symbol 286 / 287, distance symbol 30 / 31, a code no symbol has */
#define SSD_PNG_INFLATE_DISTANCE       0x0200   /* a distance beyond the bytes produced so far, or beyond the window      */
#define SSD_PNG_INFLATE_INPUT          0x0400   /* input exhausted                                                        */
#define SSD_PNG_INFLATE_OUTPUT         0x0800   /* more or fewer bytes than H * (1 + row_bytes)                           */
#define SSD_PNG_INFLATE_ADLER          0x1000   /* Adler-32 mismatch                                                      */
#define SSD_PNG_INFLATE_TRAILING       0x2000   /* input bytes behind the trailer                                         */
#define SSD_PNG_INFLATE_FILTER         0x4000   /* a filter byte above 4                                                  */
#define SSD_PNG_INFLATE_MAX_STREAM     (1ll << 20)
struct ssd_png_inflate_desc {
    long long zlib_offset;      /* the joined IDAT payload in packed_dev                                                 */
    long long zlib_bytes;
    long long dst_offset;       /* H * (1 + row_bytes) bytes in packed_dev: the src_offset of the image's ssd_png_dec_desc */
    long long chain_offset;     /* int32 [H] in packed_dev: the chain_offset of the image's ssd_png_dec_desc (chains = H)  */
    long long row_bytes;
    int H;
    int reserved;               /* 0                                                                                     */
};
int ssd_png_inflate(unsigned char* packed_dev, size_t packed_bytes, const struct ssd_png_inflate_desc* desc_host,
                    const struct ssd_png_inflate_desc* desc_dev, int B, int* status_dev, void* stream);
int ssd_png_inflate_host(const unsigned char* zlib, size_t n, unsigned char* out, size_t out_bytes, long long row_bytes, int* status);

/* DEVICE ENTROPY DECODER (ssd_jpeg_scan_plan, ssd_jpeg_unpack): the Huffman decoding of ssd_jpeg_entropy_decode on the
 * device, for a ragged batch, bit for bit.  A Huffman stream is bit-granular, but JPEG's self-synchronises: a decoder
 * started at a wrong bit falls into step with the true one after a few dozen codes.  Each SEGMENT of a scan (one restart
 * interval, or the whole scan) is cut into subsequences of subseq_bits bits; every subsequence but the first starts from
 * the guess "a DC code of MCU block 0 begins at my first bit", and the entry states are swept until none changes.  The
 * first state is known, so the fixed point is the true decode: exact, not heuristic.
 *
 * HOST (plain C++ under the rules of the host half above: no HIP call, no global state, thread-safe, nothing read outside
 * [data, data + n)):
 * ssd_jpeg_scan_plan: what the device needs beyond struct ssd_jpeg_info, WITHOUT decoding a code: the byte range
 *   [data_begin, data_end) of the entropy-coded data, each component's DC and AC table in the form the decoder indexes
 *   (huff[2 c] DC, huff[2 c + 1] AC), and the segments: info's restart_interval ? ceil(mcus / restart_interval) : 1 of
 *   them, each with its first byte (from data_begin), its byte length and its first MCU.  A segment ends where the host
 *   decoder's reader stops: at the first 0xFF not followed by 0x00, or at an 0xFF that is the last byte; fill bytes 0xFF
 *   before a marker are skipped; the k-th restart must be 0xD0 + (k & 7).  SSD_E_INVALID: what ssd_jpeg_parse refuses, an
 *   info that does not describe the stream, a wrong or missing restart marker, fewer segments than the frame needs,
 *   seg_capacity below the number of segments.  SSD_E_UNSUPPORTED: what ssd_jpeg_parse calls so, entropy-coded data of
 *   SSD_JPEG_UNPACK_MAX_SCAN_BYTES or more.
 * ssd_jpeg_entropy_decode_subseq: ssd_jpeg_entropy_decode's contract (return codes, nothing written outside coef_out)
 *   computed by the device's algorithm: the same decode core (csrc/ssd_jpeg_huff.h) through the same phases, as loops over
 *   "threads".  SSD_OK implies that ssd_jpeg_entropy_decode returns SSD_OK with the same coefficients; it refuses
 *   (SSD_E_INVALID) whatever the host decoder refuses.  subseq_bits as below.
 *
 * DEVICE (ssd_jpeg_unpack): packed_dev [packed_bytes] holds descriptors | Huffman tables | segment tables | the stuffed
 * scan bytes [data_begin, data_end) of every image, each part at a multiple of 16.  Image b's coefficients go to
 * coef_offset of coef_dev [coef_bytes] in exactly the storage of struct ssd_jpeg_info -- natural order, padded planes,
 * DC terms predicted -- so a following ssd_jpeg_decode reads that buffer as its packed_dev unchanged, and no coefficient
 * ever exists in host memory.  One call, a fixed number of launches (four kernels and two fills), asynchronous on
 * `stream`; no workgroup waits on another.
 *   zero    every image's region of coef_dev (blocks the stream never reaches stay zero), nothing between the regions
 *   sync    one workgroup per image walks its subsequences in chunks of 256 and carries the settled exit state of a chunk
 *           into the next; the sweeps are a barrier loop ended by a workgroup-wide vote, capped at 256 (the worst case of a
 *           chunk: each sweep settles at least one more state).  Every thread counts the blocks it completes; the running
 *           sum of the counts gives every subsequence the ordinal of the block it starts in.
 *   write   one thread per subsequence decodes once more from its settled state: AC values to their natural index, the DC
 *           DIFFERENCE to index 0 (a block that straddles two subsequences is written by two threads at disjoint
 *           indices); every store is guarded by the frame's MCU count.  Blocks beyond the frame and data after the last
 *           MCU are ignored, as on the host.
 *   dc      per component and segment an inclusive scan of the differences in scan order (MCU order).
 * status_dev (int32 [B]): 0, or nonzero when the settled pass meets what the host decoder refuses: a code outside its
 *   table or an index past 63 (bit 0), bits that run out before the segment's last MCU (bit 1), a restart interval whose
 *   last code does not end inside its segment's last byte (bit 2: the condition under which the host decoder finds the
 *   marker where it looks -- the device is at least as strict), tables no plan produces (bit 3).  status[b] == 0 implies
 *   that ssd_jpeg_entropy_decode returns SSD_OK with the same coefficients.  A flagged image's region may hold anything
 *   inside its own bounds; every other image is exact.
 * subseq_bits: 0 = SSD_JPEG_UNPACK_SUBSEQ_BITS; else a multiple of 32, at least 128 (a step spans at most 80 stuffed
 *   bits, so a state leaves a subsequence into the next one).
 * block_start / seg_start / sub_start: the running sums over the batch of the images' 8x8 blocks, of segments + 1, and
 *   of ssd_jpeg_unpack_slots(scan_bytes, segments, subseq_bits) (a multiple of 256 that bounds the image's subsequences).
 * Workspace: ssd_jpeg_unpack_workspace_bytes(desc_host, B, subseq_bits) bytes (0 for an unusable batch).  Its first B
 *   int32 are a debug counter: the sweeps the sync phase took for image b (the most over its chunks).
 * SSD_E_INVALID, nothing launched: NULL pointers, packed_dev / coef_dev / workspace_dev not 16-byte aligned, status_dev
 *   not 4-byte aligned, offsets that are negative or no multiple of 16, regions outside their buffer, coefficient regions
 *   that overlap or are out of order, coef_dev overlapping packed_dev, a segment count that is not the frame's, wrong
 *   running sums, a workspace that is too small.  SSD_E_UNSUPPORTED, nothing launched: a subseq_bits that is no multiple
 *   of 32 or below 128 (and not 0) or above SSD_JPEG_UNPACK_MAX_SUBSEQ_BITS, a side outside 1..16384, components /
 *   sampling other than the decoder's, scan_bytes of SSD_JPEG_UNPACK_MAX_SCAN_BYTES or more, B > 65535, 2^31 blocks or
 *   subsequence slots or more.  B == 0 is a no-op. */
#define SSD_JPEG_UNPACK_SUBSEQ_BITS 1024
#define SSD_JPEG_UNPACK_MAX_SUBSEQ_BITS 65536
#define SSD_JPEG_UNPACK_MAX_SCAN_BYTES (1LL << 28)
struct ssd_jpeg_huff {              /* one Huffman table as the decoder indexes it, 912 bytes                             */
    unsigned short look[256];       /* (length << 8) | symbol for codes of at most 8 bits, 0: longer                      */
    int maxcode[17];                /* largest code of each length, -1: none                                              */
    int valoff[17];                 /* index of the first symbol of that length minus its first code                      */
    unsigned char vals[256];
    unsigned char reserved[8];
};
struct ssd_jpeg_segment {
    unsigned first_byte;            /* from data_begin                                                                    */
    unsigned bytes;                 /* stuffed bytes, without the marker that ends it                                     */
    int first_mcu;
    int reserved;
};
struct ssd_jpeg_scan_plan {
    long long data_begin, data_end; /* the entropy-coded data: the first segment's first byte .. the last segment's end   */
    int segments;
    int reserved;
    struct ssd_jpeg_huff huff[6];   /* component c: huff[2 c] DC, huff[2 c + 1] AC (a grey image: the first two)          */
};
int ssd_jpeg_scan_plan(const unsigned char* data, size_t n, const struct ssd_jpeg_info* info, struct ssd_jpeg_scan_plan* plan,
                       struct ssd_jpeg_segment* segments, size_t seg_capacity);
int ssd_jpeg_entropy_decode_subseq(const unsigned char* data, size_t n, const struct ssd_jpeg_info* info, short* coef_out,
                                   size_t coef_bytes, int subseq_bits);
struct ssd_jpeg_unpack_desc {
    long long scan_offset;  /* byte offset in packed_dev of the image's stuffed scan bytes, a multiple of 16              */
    long long scan_bytes;   /* data_end - data_begin                                                                      */
    long long huff_offset;  /* ... of its 6 struct ssd_jpeg_huff, a multiple of 16                                        */
    long long seg_offset;   /* ... of its `segments` struct ssd_jpeg_segment, a multiple of 16                            */
    long long coef_offset;  /* byte offset in coef_dev of its coefficient storage, a multiple of 16                       */
    int H, W, components;   /* components 1 or 3                                                                          */
    int h_samp, v_samp;     /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for one component)                                     */
    int restart_interval, segments;
    int block_start, seg_start, sub_start;
};
int ssd_jpeg_unpack_slots(long long scan_bytes, int segments, int subseq_bits);
size_t ssd_jpeg_unpack_workspace_bytes(const struct ssd_jpeg_unpack_desc* desc_host, int B, int subseq_bits);
int ssd_jpeg_unpack(const unsigned char* packed_dev, size_t packed_bytes, const struct ssd_jpeg_unpack_desc* desc_host,
                    const struct ssd_jpeg_unpack_desc* desc_dev, int B, int subseq_bits, unsigned char* coef_dev,
                    size_t coef_bytes, int* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- augmentation: augmentation.py:4-183 (used at trainer.py:42), the deterministic pieces; the random draws of the
 * reference's tf.random.uniform / sample_distorted_bounding_box calls are INPUTS (host side: tf-ssd_amd/augmentation.py).
 * Images float32 [B,H,W,C] in [0,1] (the reference augments after convert + resize).
 * ssd_image_mean: mean_out[b][c] = mean over H, W of (img + add[b]) (add NULL = 0): expand_image's fill colour
 *   (augmentation.py:142) and adjust_contrast's pivot.
 * ssd_augment_geometry: params [B][10] int32 = {canvas_h, canvas_w, pad_top, pad_left, crop_y, crop_x, crop_h, crop_w,
 *   flip, use_crop}: expand_image (:123-151) as a virtual canvas filled with fill[b][c], patch's tf.slice + tf.image.resize
 *   to out_h x out_w (:176-177, bilinear, half-pixel centres), flip_horizontally (:106) -- one gather kernel, out != img;
 *   use_crop 0 (flip only) needs out_h x out_w == H x W; the whole canvas as the window at its own size materialises it.
 * ssd_augment_color (C = 3, in place): params [B][4] = {brightness delta, contrast factor, hue delta, saturation factor},
 *   flags [B] bits 0..3 = which run (:51-93, reference order), mean [B][3] = contrast's pivot; ends with clip [0,1] (:27). */
int ssd_image_mean(const float* img_dev, int B, int H, int W, int C, const float* add_dev, float* mean_out_dev, void* stream);
int ssd_augment_geometry(const float* img_dev, int B, int H, int W, int C, int out_h, int out_w, const int* params_dev,
                         const float* fill_dev, float* out_dev, void* stream);
int ssd_augment_color(float* img_dev, int B, int H, int W, const float* params_dev, const int* flags_dev,
                      const float* mean_dev, void* stream);

/* ---- augmentation, the random plan drawn on the device (opt-in; the host draws of augmentation.py stay as they are) ----
 * ssd_augment_plan: the decisions of augmentation.apply (:19-25: patch [expand, min overlap, window], flip, brightness,
 *   contrast, hue, saturation) for B images of H x W in one launch, one wavefront per image, written in the layouts the
 *   three kernels above read; the ground-truth boxes are transformed along (expand_boxes, renormalize to the window,
 *   flip_boxes).  No atomics, no workspace, no host synchronisation, no allocation.
 *   gt_boxes [B,G,4] (y1, x1, y2, x2 normalised); gt_labels [B,G]: a row is valid iff label > 0 (NULL: valid iff the sum
 *   of its |coordinates| > 0).  Rows that are not valid are copied through unchanged.  An image with no valid row gets NO
 *   patch (the host sampler raises there, like TF; a kernel cannot).  boxes_out may be gt_boxes (in place).
 *   geom_out [B,10] = ssd_augment_geometry's params (no patch: {H, W, 0, 0, 0, 0, H, W, flip, 0}); color_out [B,4] and
 *   flags_out [B] = ssd_augment_color's params and flags (an operation that does not run: 0 / 1 / 0 / 1); add_out [B] =
 *   the brightness delta or 0 (ssd_image_mean's add for contrast's pivot); info_out [B,4] = {accepted sampler attempt:
 *   -1 no patch, 0..99, 100 every attempt failed and the window is the whole canvas (the host sampler's fallback);
 *   the min-overlap index drawn (0..4 -> 0.1, 0.3, 0.5, 0.7, 0.9; drawn whether or not a patch runs); 1 iff the patch
 *   expands; 0}.
 *   Random stream: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), key =
 *   (seed & 0xffffffff, seed >> 32), counter = (id & 0xffffffff, id >> 32, slot, 0) with id = sample_ids[b]: the plan is
 *   a pure function of (seed, id, H, W, the image's ground truth) -- not of B, the position in the batch or other images.
 *   A float draw is u = (word >> 8) * 2^-24 in [0, 1); a boolean is u > 0.5f (augmentation.py:33); uniform(lo, hi) =
 *   lo + u * (hi - lo) in fp32, each operation rounded on its own; an integer in [0, n) is (uint64(word) * n) >> 32.
 *   Slots (fixed, never conditional: a draw's value does not depend on which branches ran):
 *     slot 0        patch?                     expand?              flip?              brightness?
 *     slot 1        contrast?                  hue?                 saturation?        min-overlap index (n = 5)
 *     slot 2        expansion ratio U[1,4)     u_left               u_top              --
 *     slot 3        brightness U[-.12,.12)     contrast U[.5,1.5)   hue U[-.08,.08)    saturation U[.5,1.5)
 *     slot 16 + a   aspect ratio U[.5,2)       height draw          y draw             x draw          (attempt a = 0..99)
 *   Arithmetic: fp32 throughout (the TF kernel the host sampler restates computes in float; the host sampler itself uses
 *   float64 for its window), rintf = round half to even, pixel rectangles = the truncated fp32 product, areas in 64-bit
 *   integers.  Attempt a: aspect; min_h / max_h = rintf(sqrtf({0.05, 1} * canvas area / aspect)); if rintf(max_h * aspect)
 *   > canvas_w: max_h = (int)((canvas_w + 0.5f - 1e-7f) / aspect), one less if its rounded width still does not fit;
 *   max_h = min(max_h, canvas_h); min_h = min(min_h, max_h); h = min_h + integer draw in [0, max_h - min_h + 1) when
 *   min_h < max_h; w = rintf(h * aspect); h + 1 if w * h < min area, h - 1 if w * h > max area (w recomputed); rejected
 *   outside the area range or the canvas; y, x = integer draws in [0, canvas_h - h), [0, canvas_w - w) (0 when the side is
 *   full); accepted iff some valid box of >= 1 pixel has (float)intersection / (float)area >= the min overlap.  The
 *   window is the LOWEST accepted attempt (lane l evaluates attempts l and l + 64; a wave ballot picks it): the law of
 *   the sequential "first one that satisfies".
 *   SSD_E_UNSUPPORTED (nothing is launched): G > 512, or a canvas side 4 * H / 4 * W beyond 16384. */
int ssd_augment_plan(const float* gt_boxes_dev, const int* gt_labels_dev, const long long* sample_ids_dev, int B, int G, int H,
                     int W, unsigned long long seed, int* geom_out_dev, float* color_out_dev, int* flags_out_dev,
                     float* add_out_dev, int* info_out_dev, float* boxes_out_dev, void* stream);

/* ---- augmentation, mosaic (opt-in; not in the reference): four images of the batch tiled around a random centre ----------
 * ssd_augment_mosaic_plan draws the plan of every output image and merges the ground truth; ssd_augment_mosaic_pixels
 * writes the images.  No atomics, no workspace, no host synchronisation, no allocation.  Both read other images of the
 * batch: no output may overlap an input (SSD_E_INVALID).
 *   Inputs: images [B,H,W,3] float32 (already resized); gt_boxes [B,G,4] (y1, x1, y2, x2 normalised), 16-byte aligned;
 *   gt_labels [B,G] int32, REQUIRED (they are merged): a row is valid iff its label > 0; sample_ids [B]; seed; p = the
 *   probability that an output image is a mosaic; (s_min, s_max) = the scale range; G_out = rows of the output ground
 *   truth; pad_label = the label of a padding row (data_utils.get_padding_values()[2] = -1).
 *   Random stream: ssd_augment_plan's Philox4x32-10 with its key, counter layout and draw conventions (u, uniform(lo, hi),
 *   integer below n: above), on slots that kernel does not touch (it uses 0..3 and 16..115), so the same (seed, id) may feed
 *   both and the draws are independent:
 *     slot 128      mosaic?                    partner 1            partner 2          partner 3
 *     slot 129      centre y draw              centre x draw        --                 --
 *     slot 130      scale of tile 0            tile 1               tile 2             tile 3
 *   The plan of output image b (every value is computed and written whether or not b is a mosaic):
 *     mosaic iff u < p (p = 0: never, p = 1: always).
 *     tile 0 (top-left) shows image b itself; tiles 1, 2, 3 (top-right, bottom-left, bottom-right) show the images
 *       integer(word_t) below B of THIS batch, drawn with replacement (a partner may be b, partners may repeat).
 *     centre: yc = clamp((int)(H * (0.25f + 0.5f * u)), 1, H - 1), xc the same with W and its own draw.
 *     tile t: s_t = uniform(s_min, s_max); hs_t = max(1, rintf(H * s_t)), ws_t = max(1, rintf(W * s_t)).  The source image
 *       is resized as a whole to hs_t x ws_t (bilinear, half-pixel centres: ssd_augment_geometry's arithmetic with the
 *       whole image as the window and hs_t x ws_t as the output size) and placed with one corner on the centre:
 *         tile 0 rows [yc - hs, yc) columns [xc - ws, xc);    tile 1 rows [yc - hs, yc) columns [xc, xc + ws);
 *         tile 2 rows [yc, yc + hs) columns [xc - ws, xc);    tile 3 rows [yc, yc + hs) columns [xc, xc + ws).
 *     plan_out [B,16] int32 = {mosaic, yc, xc, 0, then for t = 0..3 {source, hs_t, ws_t}}.
 *   Pixels: output pixel (oy, ox) belongs to the tile (oy < yc ? top : bottom, ox < xc ? left : right); inside that tile's
 *     placed image it is the resized image's pixel, outside it fill[c] (fill: 3 floats on the HOST).  An image that is not
 *     a mosaic is copied through.  The plan is device data: a tile whose row names no image of the batch, a centre outside
 *     [0, H] x [0, W] or a size outside 1..8192 (what the plan kernel can write) shows the fill colour.
 *   Ground truth of a mosaic image: for t = 0..3 in this order and the VALID rows of tile t's source in row order, in fp32
 *   with every operation rounded on its own (top / left = the first row / column of the placed image, as floats):
 *     Y1 = top + y1 * hs, Y2 = top + y2 * hs, X1 = left + x1 * ws, X2 = left + x2 * ws                       (pixels)
 *     (cy1, cy2) = Y1, Y2 clipped to the tile's rows [0, yc] or [yc, H]; (cx1, cx2) = X1, X2 clipped to its columns [0, xc]
 *       or [xc, W]   (v < lo ? lo : v > hi ? hi : v)
 *     h = cy2 - cy1, w = cx2 - cx1, h0 = Y2 - Y1, w0 = X2 - X1; the row is KEPT iff
 *       h >= 2 && w >= 2 && w * h >= 0.1f * (w0 * h0) && w < 100 * h && h < 100 * w
 *     a kept row is written as (cy1 / H, cx1 / W, cy2 / H, cx2 / W) with its source's label at the next free output row;
 *     kept rows beyond G_out are dropped; the remaining rows are padding: all-zero box, pad_label.
 *   Ground truth of an image that is not a mosaic: its G rows copied to rows 0..G-1 as they are, valid or not; the rest
 *     is padding.
 *   info_out [B,4] = {mosaic, rows kept by the rule, rows written, valid source rows seen}; not a mosaic: {0, 0, G, 0}.
 *   The plan kernel runs one wavefront per output image: lanes take a source's rows 64 at a time, a wave ballot and a
 *   prefix popcount give every kept row its output index -- the law of the sequential order above.
 *   SSD_E_UNSUPPORTED (nothing is launched) outside 2 <= H, W <= 4096, 1 <= G <= 512, G <= G_out <= 2048, B <= 65535.
 *   SSD_E_INVALID (nothing is launched): p outside [0, 1]; a scale range outside 0.1 <= s_min <= s_max <= 2; a NULL
 *   pointer; an output that overlaps an input or another output.  B == 0 is a no-op. */
int ssd_augment_mosaic_plan(const float* gt_boxes_dev, const int* gt_labels_dev, const long long* sample_ids_dev, int B, int G,
                            int H, int W, unsigned long long seed, float p, float s_min, float s_max, int G_out, int pad_label,
                            int* plan_out_dev, float* boxes_out_dev, int* labels_out_dev, int* info_out_dev, void* stream);
int ssd_augment_mosaic_pixels(const float* img_dev, int B, int H, int W, const int* plan_dev, const float* fill /* host, 3 */,
                              float* out_dev, void* stream);

/* ---- drawing: utils/drawing_utils.py:6-85 (draw_grid_map, draw_bboxes, draw_bboxes_with_labels) ---------------------
 * ssd_image_minmax: minmax_out [B][2] = {min, max} over H, W, C of each image of img_dev [B,H,W,3] float32: the two numbers
 *   of [3P] Keras array_to_img(scale=True).  NaN pixels are ignored.  workspace: ssd_image_minmax_workspace_bytes(B) bytes,
 *   4-byte aligned (partial results; two launches, no atomics).
 * ssd_draw_detections: out_dev [B,H,W,3] uint8 = array_to_img of every image, then the reference's PIL loop on it -- for
 *   each box in index order ImageDraw.text((x1 + 4, y1 + 2), text) in the legacy bitmap font and
 *   ImageDraw.rectangle((x1, y1, x2, y2), outline, width) -- reproduced to the byte ([3P] Pillow, pinned by
 *   tests/golden/drawing.npz) in one pass that writes each output byte once: a pixel takes the colour of the LAST box
 *   whose frame or text inks it.
 *     array_to_img, every step a separately rounded fp32 op: v = x - min; if (max - min != 0) v = v / (max - min);
 *       v = v * 255; uint8(v) truncates.  minmax_dev NULL: no scaling, out = uint8(x) saturated to 0..255 (float images
 *       that already hold bytes: draw_grid_map).
 *     boxes_dev [B,T,4] int32 = (y1, x1, y2, x2) in pixels, corners inclusive, 16-byte aligned; they may lie partly or
 *       wholly outside the image.  A box with x2 - x1 <= 0 or y2 - y1 <= 0 is skipped (drawing_utils.py:63), and so is a
 *       box whose label is outside [0, L).  Boxes thinner than 2 * outline_width paint outside their rectangle exactly
 *       as Pillow's strokes do.
 *     labels_dev [B,T] int32 index colors_dev [L][3] uint8.  text_dev [B,T,maxlen] bytes with text_len_dev [B,T] (clamped
 *       to 0..maxlen); bytes outside 32..126 draw nothing (the Python surface raises ValueError for them).  atlas_dev
 *       [96][4] uint32: per glyph (95 printable ASCII, then a blank) 11 row bytes, bit k = column k - 1 of the 6-wide
 *       cell, byte 11 unused, then a word {first box row, end box row << 8, has column -1 << 16}
 *       (utils/drawing_utils.glyph_atlas builds it from Pillow's font).
 *     fill != 0: boxes are filled rectangles instead (ImageDraw.rectangle(fill=): draw_grid_map), drawn down to one
 *       pixel (only x2 < x1 or y2 < y1 is skipped); no text.  text_dev / text_len_dev / atlas_dev may be NULL then and
 *       when maxlen == 0.
 *   B == 0 is a no-op; T == 0 writes the plain converted images.
 * ssd_draw_bounding_boxes: [3P] tf.image.draw_bounding_boxes (TF 2.0 DrawBoundingBoxesOp restated; unpinned): img_dev /
 *   out_dev [B,H,W,3] float32 (out != img), boxes_dev [B,T,4] float32 normalised (y1, x1, y2, x2), colors_dev [L][3]
 *   float32 cycled by box index.  Corners are int64(float(coord) * (size - 1)); an inverted box and a box entirely
 *   outside are skipped; each 1-pixel edge is drawn only when that edge lies inside; later boxes overwrite earlier ones.
 * Supported: C == 3, H and W in 1..16384, B <= 65535, T <= 4096 (ssd_draw_detections) / 1024 (ssd_draw_bounding_boxes),
 *   maxlen <= 64; anything else returns SSD_E_UNSUPPORTED before any launch and leaves the output untouched.
 *   outline_width outside 1..64 and NULL pointers are SSD_E_INVALID. */
size_t ssd_image_minmax_workspace_bytes(int B);
int ssd_image_minmax(const float* img_dev, int B, int H, int W, int C, float* minmax_out_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
int ssd_draw_detections(const float* img_dev, const float* minmax_dev, int B, int H, int W, int C, const int* boxes_dev,
                        const int* labels_dev, const unsigned char* text_dev, const int* text_len_dev, int T, int maxlen,
                        const unsigned char* colors_dev, int L, const unsigned* atlas_dev, int outline_width, int fill,
                        unsigned char* out_dev, void* stream);
int ssd_draw_bounding_boxes(const float* img_dev, int B, int H, int W, int C, const float* boxes_dev, int T,
                            const float* colors_dev, int L, float* out_dev, void* stream);

/* ---- training loss: ssd_loss.py:8-65 (N1) ----------------------------------------------
 * CustomLoss.loc_loss_fn + conf_loss_fn in one kernel per image.
 *   actual_deltas / pred_deltas [B,N,4]; actual_labels (one-hot) / pred_labels (probabilities)
 *   [B,N,L] (device).  Either pair may be NULL to evaluate only the other term.
 *   loc_loss [B]  = alpha * sum_pos Huber_{delta=1}(pred - actual summed over 4) / max(#pos, 1),
 *                   positives = anchors with any non-zero actual delta           (ssd_loss.py:18-33)
 *   conf_loss [B] = sum_n (pos + neg)_n * CE_n / max(#pos, 1); CE on probabilities renormalised
 *                   by their sum and clipped to [1e-7, 1-1e-7] ([3P] Keras categorical_crossentropy
 *                   on a non-Softmax-op tensor); pos = any one-hot column 1.. set; neg = rank of
 *                   CE*y0 in descending order (ties: lower anchor index) < int(#pos * ratio)
 *                                                                                  (ssd_loss.py:45-63)
 * Optional outputs: ce_out [B,N], mask_out [B,N] (pos + neg, the reference's final_mask; 2 where a
 * positive also ranks as negative), and the gradients of grad_scale * (loc_loss[b] + conf_loss[b])
 * w.r.t. pred_deltas (grad_deltas [B,N,4]) and w.r.t. the LOGITS behind pred_labels = softmax(z)
 * (grad_logits [B,N,L]); grad_scale = 1/batch gives the Keras batch-mean objective. */
size_t ssd_loss_workspace_bytes(int B, int N);
int ssd_loss(const float* actual_deltas_dev, const float* pred_deltas_dev,
             const float* actual_labels_dev, const float* pred_labels_dev, int B, int N, int L,
             float neg_pos_ratio, float loc_loss_alpha, float* loc_loss_dev, float* conf_loss_dev,
             float* ce_out_dev, float* mask_out_dev, float* grad_deltas_dev, float* grad_logits_dev,
             float grad_scale, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- focal confidence loss: Keras CategoricalFocalCrossentropy(alpha, gamma) ---------------------
 * The same tensors as ssd_loss; the localisation term is ssd_loss's, the confidence term replaces the hard-negative
 * mining: every anchor counts.  Per anchor, with q the predicted probabilities and y the target row, in fp32, every
 * operation rounded on its own (no contraction), sums in class order:
 *   s   = sum_c q_c
 *   r_c = clip(q_c / s, 1e-7, 1 - 1e-7)                                 (ssd_loss's renormalise-and-clip)
 *   f   = sum_c (alpha * (1 - r_c)^gamma) * -(y_c * log r_c)            (a class with y_c == 0 adds exactly 0)
 * Per image: pos = #{anchors with any y[1:] != 0};  conf_loss[b] = (sum over ALL anchors of f) / (pos == 0 ? 1 : pos),
 * the sum taken per tile of ssd_focal_loss_tile(L) anchors by a fixed tree, then over the tiles in order by a fixed tree.
 * ce_out [B,N] <- f; mask_out [B,N] <- 1 (no mining: the final mask is all ones).
 * Gradients of grad_scale * (loc_loss[b] + conf_loss[b]) w.r.t. pred_deltas and the LOGITS behind pred_labels:
 *   df/dr_c = (y_c * alpha) * (gamma * ((1 - r)^gamma / (1 - r)) * log r - (1 - r)^gamma / r),  r = q_c / s,
 *             where r lies in [1e-7, 1 - 1e-7] (bounds included), 0 elsewhere (ssd_loss's rule);
 *   then through r = q / s and the softmax backward exactly as ssd_loss does with g_c = df/dr_c and
 *   gce = grad_scale / (pos == 0 ? 1 : pos).
 *   gamma == 0: the modulating factor is exactly 1 and the first term exactly 0 (no powf is evaluated).
 * An anchor's bits depend on its own rows and the image's two positive counts, not on the grid; no atomics.
 * Rows of L <= 119 floats are staged through LDS (coalesced 16-byte accesses); longer rows are read directly.
 * SSD_E_INVALID, nothing launched: bad sizes, alpha <= 0, gamma < 0, either not finite, neither term given, a gradient
 * without its target, a workspace below ssd_focal_loss_workspace_bytes(B, N, L), delta tensors not 16-byte aligned.
 * ssd_focal_loss_tile: anchors per workgroup for this L (*staged_out, nullable: 1 when the rows go through LDS). */
int ssd_focal_loss_tile(int L, int* staged_out);
size_t ssd_focal_loss_workspace_bytes(int B, int N, int L);
int ssd_focal_loss(const float* actual_deltas_dev, const float* pred_deltas_dev,
                   const float* actual_labels_dev, const float* pred_labels_dev, int B, int N, int L,
                   float loc_loss_alpha, float focal_alpha, float focal_gamma, float* loc_loss_dev,
                   float* conf_loss_dev, float* ce_out_dev, float* mask_out_dev, float* grad_deltas_dev,
                   float* grad_logits_dev, float grad_scale, void* workspace_dev, size_t workspace_bytes,
                   void* stream);

/* ---- IoU-family localisation losses: IoU / GIoU / DIoU / CIoU on the decoded boxes ----------------
 * The delta tensors of ssd_loss, plus priors [N,4] (y1,x1,y2,x2) on the device and variances[4] on the host; replaces
 * only the localisation term.  Per anchor, t is the box decoded from actual_deltas and b the box decoded from
 * pred_deltas, both by ssd_decode_boxes' arithmetic with `var` (utils/bbox_utils.py:61-85 on deltas * variances):
 *   h = exp(dh*vh)*ph,  cy = dy*vy*ph + pcy,  y1 = cy - 0.5h,  y2 = h + y1,  likewise for x; nothing is clamped.
 * In fp32, every operation rounded on its own (no contraction), eps = 1e-7:
 *   inter = max(min(y2,ty2) - max(y1,ty1), 0) * max(min(x2,tx2) - max(x1,tx1), 0)
 *   union = ((y2-y1)(x2-x1) + (ty2-ty1)(tx2-tx1)) - inter;           iou = inter / (union + eps)
 *   ch = max(y2,ty2) - min(y1,ty1), cw likewise, ac = ch*cw          (the enclosing box)
 *   rho2 = ((y1+y2)/2 - (ty1+ty2)/2)^2 + ((x1+x2)/2 - (tx1+tx2)/2)^2;   c2 = (ch*ch + cw*cw) + eps
 *   v = (4/pi^2) * (atan(tw/th) - atan(w/h))^2  with w = x2-x1, h = y2-y1;   a = v / (((1 - iou) + v) + eps)
 *   SSD_LOC_IOU   l = 1 - iou
 *   SSD_LOC_GIOU  l = 1 - (iou - (ac - union) / (ac + eps))
 *   SSD_LOC_DIOU  l = (1 - iou) + rho2/c2
 *   SSD_LOC_CIOU  l = ((1 - iou) + rho2/c2) + a*v
 * (torchvision.ops' generalized_ / distance_ / complete_box_iou_loss with the boxes in (y1,x1,y2,x2) order.)
 * Per image: positives are the anchors with any non-zero actual delta (ssd_loss's rule);
 *   loc_loss[b] = (sum over the positives of l) / (pos == 0 ? 1 : pos) * loc_loss_alpha,
 * the sum taken per tile of ssd_iou_loc_loss_tile() anchors by a fixed tree, then over the tiles in order by a fixed tree.
 * per_anchor_out [B,N] (nullable) <- l for a positive, 0 for every other anchor.
 * grad_deltas [B,N,4] (nullable) <- the analytic gradient of grad_scale * loc_loss[b] w.r.t. pred_deltas, through the box
 * terms and the decode (exp and the variances included); exactly 0.0f for every anchor that is not positive.
 * Subgradients: min(p, q) / max(p, q) with p the prediction's coordinate pass the gradient to p at a tie (p == q), so a
 * prediction equal to its target gets a finite one-sided gradient; max(x, 0) passes it where x > 0; CIoU's `a` is a
 * constant in the backward (the usual stop-gradient).
 * An anchor's bits depend on its own rows and the image's positive count, not on the grid; no atomics.
 * SSD_E_INVALID, nothing launched: bad sizes, a mode outside SSD_LOC_IOU .. SSD_LOC_CIOU, variances NULL, not finite or
 * <= 0, priors NULL, a gradient without the target, actual_deltas or pred_deltas NULL, a workspace below
 * ssd_iou_loc_loss_workspace_bytes(B, N), priors or delta tensors not 16-byte aligned.  B == 0: SSD_OK, nothing written. */
#define SSD_LOC_HUBER 0            /* the reference's Huber loss on the encoded deltas (ssd_loss / ssd_focal_loss) */
#define SSD_LOC_IOU 1
#define SSD_LOC_GIOU 2
#define SSD_LOC_DIOU 3
#define SSD_LOC_CIOU 4
int ssd_iou_loc_loss_tile(void);
size_t ssd_iou_loc_loss_workspace_bytes(int B, int N);
int ssd_iou_loc_loss(const float* priors_dev, const float* variances, const float* actual_deltas_dev,
                     const float* pred_deltas_dev, int B, int N, int mode, float loc_loss_alpha,
                     float* loc_loss_dev, float* per_anchor_out_dev, float* grad_deltas_dev, float grad_scale,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* The loss of a training step (ssd_net_train_forward_backward_cfg). */
#define SSD_LOSS_HARD_NEGATIVE 0   /* ssd_loss: the reference's mining; neg_pos_ratio, loc_loss_alpha          */
#define SSD_LOSS_FOCAL 1           /* ssd_focal_loss: loc_loss_alpha, focal_alpha (> 0), focal_gamma (>= 0)   */
typedef struct ssd_loss_config {
    int kind;
    float neg_pos_ratio, loc_loss_alpha, focal_alpha, focal_gamma;
    /* the localisation term (SSD_LOC_*); a zero-filled tail is SSD_LOC_HUBER, the term of `kind`'s own kernel.  Another
     * value: the confidence term alone comes from `kind`'s kernel and ssd_iou_loc_loss(priors_dev [num_priors,4],
     * variances, mode = loc_kind) writes the localisation loss and its gradient. */
    int loc_kind;
    const float* priors_dev;
    float variances[4];
} ssd_loss_config;
size_t ssd_loss_config_bytes(void);      /* sizeof(ssd_loss_config) of this library (for mirrors of the struct) */

/* =====================================================================================
 * Conv family (the TF/Keras ops the models dispatch: SURVEY.md 2.3 K1-K7).
 * All tensors NHWC fp32 on the device.
 * ================================================================================== */

enum ssd_act { SSD_ACT_NONE = 0, SSD_ACT_RELU = 1, SSD_ACT_RELU6 = 2 };

/* Geometry of one convolution.  pad_* are explicit (TF SAME / ZeroPadding2D asymmetry is
 * resolved by the caller; ssd_same_pads() below restates the TF rule). */
typedef struct ssd_conv_desc {
    int B, H, W, Cin;          /* input  [B,H,W,Cin]                       */
    int Cout, kh, kw;          /* kernel [kh,kw,Cin,Cout] (Keras HWIO)     */
    int stride, dilation;
    int pad_t, pad_l, pad_b, pad_r;
    int act;                   /* enum ssd_act, applied after scale/shift  */
    int has_residual;          /* add residual [B,Ho,Wo,Cout] before store */
    int dma_two_stage;         /* ssd_conv2d_planes_f16x2, "dmah_*" configs with one k-step per barrier: 0 (a zero-filled
                                * tail) the three-stage LDS ring, non-zero the two-stage loop (the net option dma_ring 0);
                                * the same bits either way.  Every other kernel ignores it */
} ssd_conv_desc;

/* TF SAME rule: out=ceil(in/s), p=max((out-1)*s+(k-1)*d+1-in,0),
 * before=p/2, after=p-before.  Returns out size. */
int ssd_same_pads(int in, int k, int stride, int dilation, int* before, int* after);
int ssd_conv_out_size(int in, int k, int stride, int dilation, int pad_before, int pad_after);

/* Packed dense-conv weights: [Npad][Kpad] fp32, K = (ky*kw+kx)*Cin+ci, zero padded (device), followed by four
 * bf16 planes [4][Npad][Kpad] of the same matrix: h, m, l = its EXACT three-way split (x = h + m + l; the "mfma3_*"
 * tile configs run every product as six bf16 MFMAs at fp32 accuracy, csrc/ssd_bf16x3.h) and r = its bf16 rounding
 * (round to nearest even; the "bf16_*" tile configs of the net's precision-1 mode run ONE bf16 MFMA per product of
 * once-rounded operands).  ssd_conv_packed_weight_floats() covers all of it.  scale/shift [Cout] are the folded
 * BatchNorm (or 1/bias) epilogue vectors. */
size_t ssd_conv_packed_weight_floats(int kh, int kw, int Cin, int Cout);
int ssd_conv_pack_weights(const float* hwio_dev, int kh, int kw, int Cin, int Cout,
                          float* packed_dev, void* stream);

/* Conv2D (+BatchNorm +activation +residual): the MFMA implicit-GEMM kernel (K1,K3).
 * Replaces keras Conv2D / BatchNormalization / ReLU call sites
 * (models/ssd_mobilenet_v2.py:16-32, models/ssd_vgg16.py:52-91, models/header.py:60-61).
 * out address of pixel (b, p=oy*Wo+ox), channel n:
 *     out_dev + b*out_batch_stride + p*out_pixel_stride + n
 * (pass 0 for the strides to get the dense [B,Ho,Wo,Cout] default), which is how the
 * head convs write straight into the concatenated [B,N,K] buffers (models/header.py:34-41). */
int ssd_conv2d(const ssd_conv_desc* d, const float* in_dev, const float* packed_w_dev,
               const float* scale_dev, const float* shift_dev, const float* residual_dev,
               float* out_dev, long out_batch_stride, long out_pixel_stride, void* stream);

/* Tuning / test hooks of the same kernel family: explicit tile configuration (-1 = cost
 * model), optional deterministic split-K (split_k > 1 needs split_k*M*Cout floats). */
int ssd_conv_num_configs(void);
const char* ssd_conv_config_name(int config);
int ssd_conv2d_ex(const ssd_conv_desc* d, const float* in_dev, const float* packed_w_dev,
                  const float* scale_dev, const float* shift_dev, const float* residual_dev,
                  float* out_dev, long out_batch_stride, long out_pixel_stride, int config,
                  int split_k, float* splitk_ws_dev, void* stream);

/* The same op on the LDS-DMA tiles ("dma3_*" / "dmab_*" configs, csrc/ssd_convdma.hip): the INPUT is handed over as
 * bf16 planes [planes][n] (planes = 3: the exact split x = h + m + l of the fp32 activation, fp32 results as above;
 * planes = 1: its bf16 rounding -- the bf16 mode's storage format), `in_plane_stride` ELEMENTS between planes; both
 * operands then reach LDS by `buffer_load ... lds` without passing through registers.  Inside a plane the NHWC tensor
 * of `channels` channels (a multiple of 32) and P = n / channels pixels is stored SLICE-MAJOR, [channels / 32][P][32]:
 * element (pixel, c) at ((c / 32) * P + pixel) * 32 + c % 32 -- the 16 rows x 64 bytes of one copy instruction are then
 * 1 KB of contiguous memory.  ssd_split_planes writes such
 * planes from an fp32 tensor (n % 4 == 0), ssd_join_planes restores fp32 (exactly, for planes = 3); the conv can write
 * its own output as planes too (out_planes_dev != NULL: dense outputs with Cout % 32 == 0) for the next layer. */
int ssd_split_planes(const float* x_dev, long n, int channels, int planes, void* planes_dev, long plane_stride, void* stream);
int ssd_join_planes(const void* planes_dev, long n, int channels, int planes, long plane_stride, float* x_dev, void* stream);
int ssd_conv2d_planes(const ssd_conv_desc* d, const void* in_planes_dev, int planes, long in_plane_stride,
                      const float* packed_w_dev, const float* scale_dev, const float* shift_dev,
                      const float* residual_dev, float* out_dev, long out_batch_stride, long out_pixel_stride,
                      void* out_planes_dev, long out_plane_stride, int config, int split_k,
                      float* splitk_ws_dev, void* stream);

/* The two-plane fp16 form of the LDS-DMA tiles ("dmah_*" configs; "dmah_*_ks2": two 32-wide k-steps per barrier).
 * planes = 2 in ssd_split_planes / ssd_join_planes: the activation x as the fp16 pair h = fp16(256 x),
 * l = fp16(256 x - h), both rounded to nearest even, in the slice-major layout above (2 bytes per element).
 * RANGE CONTRACT: the form is made for ReLU6 outputs.  |x| <= 255 is represented within
 *     |join(split(x)) - x| <= 2^-22 |x| + 2^-33;
 * |x| above ~255.9 becomes inf and joins to a non-finite value -- nothing is silently made finite.  The weights are
 * two fp16 planes of 2^k w, [2][Kpad / 32][Npad][32] (ssd_conv_f16x2_weight_bytes of device memory, 16-byte aligned),
 * written by ssd_conv_pack_weights_f16x2 from the packed fp32 weights of ssd_conv_pack_weights (whose buffer keeps its
 * size and layout); it chooses k so that max |w| 2^k lies in [2^13, 2^14) (all-zero weights: k = 0), returns it in
 * *k_out, synchronises the stream, and answers SSD_E_UNSUPPORTED for a non-finite weight.  Each fp32 product is three
 * v_mfma_f32_16x16x32_f16 (wl xh, wh xl, wh xh; the dropped wl xl is ~2^-22 relative) into one fp32 accumulator,
 * multiplied by the exact 2^-(8 + k) before the epilogue and before split-K partials are written.  An output requested
 * as planes is written in the same two-plane form (so it obeys the same range contract).
 * ssd_conv2d_planes_f16x2 takes only "dmah_*" configs and these take only this entry point: bf16 planes, the fp32
 * entry points and Cin % 32 != 0 answer SSD_E_UNSUPPORTED. */
size_t ssd_conv_f16x2_weight_bytes(int kh, int kw, int Cin, int Cout);
int ssd_conv_pack_weights_f16x2(const float* packed_w_dev, int kh, int kw, int Cin, int Cout, void* w_planes_dev,
                                int* k_out, void* stream);
int ssd_conv2d_planes_f16x2(const ssd_conv_desc* d, const void* in_planes_dev, long in_plane_stride,
                            const float* packed_w_dev, const void* w_planes_dev, int w_exp, const float* scale_dev,
                            const float* shift_dev, const float* residual_dev, float* out_dev,
                            long out_batch_stride, long out_pixel_stride, void* out_planes_dev,
                            long out_plane_stride, int config, int split_k, float* splitk_ws_dev, void* stream);

/* Winograd F(2x2,3x3) variant of the same op for 3x3 stride-1 dilation-1 convs with Cin % 16 == 0
 * (the SSD head convs, models/header.py:60-61, and VGG16's 3x3 backbone, models/ssd_vgg16.py:52-72):
 * 2.25x fewer multiplications on the same fp32 MFMA, fused input / output transforms.  Weights are
 * transformed once ([16][Npad][Cin] floats).  The graph runner's autotune picks it per layer.
 * Any other convolution answers SSD_E_UNSUPPORTED with "cannot run" in ssd_last_error(), as every tile family of
 * ssd_conv2d_ex / ssd_conv2d_planes does for a shape outside its constraints (the refusal contract on non-square
 * geometry: tests/conv_geometry_cases.py REFUSALS). */
size_t ssd_conv_wino_weight_floats(int Cin, int Cout);
int ssd_conv_wino_pack_weights(const float* hwio_dev, int Cin, int Cout, float* wino_w_dev, void* stream);
int ssd_conv_wino_num_configs(void);
int ssd_conv2d_wino(const ssd_conv_desc* d, const float* in_dev, const float* wino_w_dev,
                    const float* scale_dev, const float* shift_dev, float* out_dev,
                    long out_batch_stride, long out_pixel_stride, int wino_config, int split_k,
                    float* splitk_ws_dev, void* stream);

/* DepthwiseConv2D 3x3 (+BN +act): weights [3,3,C] (Keras [3,3,C,1]) device (K2). */
int ssd_dwconv3x3(const float* in_dev, int B, int H, int W, int C, int stride,
                  int pad_t, int pad_l, int pad_b, int pad_r,
                  const float* w_dev, const float* scale_dev, const float* shift_dev,
                  int act, float* out_dev, void* stream);

/* MaxPool2D with TF SAME semantics (padded cells ignored): models/ssd_vgg16.py:54-73 (K4) */
int ssd_maxpool2d(const float* in_dev, int B, int H, int W, int C, int k, int stride,
                  int pad_t, int pad_l, int pad_b, int pad_r, float* out_dev, void* stream);

/* L2Normalization: models/ssd_vgg16.py:7-31 (K5): x * rsqrt(max(sum_c x^2, 1e-12)) * gamma_c */
int ssd_l2norm(const float* in_dev, long pixels, int C, const float* gamma_dev,
               float* out_dev, void* stream);

/* softmax over the last dim (models/header.py:64) (K7); in-place allowed. */
int ssd_softmax(const float* in_dev, long rows, int L, float* out_dev, void* stream);

/* =====================================================================================
 * Graph runner: models/ssd_mobilenet_v2.py:7-35 (F3) / models/ssd_vgg16.py:33-97 (F6)
 * + models/header.py:43-67 (F1,F2) [+ models/decoder.py:57-69 (D4)].
 * A net owns its packed weights, activation arena and (optionally) a captured hipGraph.
 * ================================================================================== */
typedef struct ssd_net ssd_net;

enum ssd_backbone { SSD_MOBILENET_V2 = 0, SSD_VGG16 = 1 };

/* n_ars[levels] = len(aspect_ratios[l]) (anchors per cell = n_ars+1), total_labels = L. */
ssd_net* ssd_net_create(int backbone, int img_size, int levels, const int* n_ars,
                        int total_labels);
void ssd_net_destroy(ssd_net* net);

/* Parameter table in Keras order / names (e.g. "Conv1/kernel", "bn_Conv1/gamma",
 * "block_1_expand/kernel", "extra1_1/bias", "1_conv_label_output/kernel" ...). */
int ssd_net_num_params(const ssd_net* net);
const char* ssd_net_param_name(const ssd_net* net, int i);
int ssd_net_param_rank(const ssd_net* net, int i);
const int* ssd_net_param_shape(const ssd_net* net, int i);
/* Copy one parameter from HOST memory in its Keras layout (count = product of shape). */
int ssd_net_set_param(ssd_net* net, const char* name, const float* host_data, size_t count);
/* Read a parameter back (HOST), Keras layout. */
int ssd_net_get_param(const ssd_net* net, const char* name, float* host_out, size_t count);
/* Fold BN, pack weights for the MFMA kernels, size the arena for `max_batch`. */
int ssd_net_finalize(ssd_net* net, int max_batch);
/* Tile-configuration table chosen by finalize's on-device autotune, as text (one
 * "layer config split_k" line per conv).  get returns the length (buf may be NULL);
 * set installs a table that the next finalize uses instead of re-tuning (if complete/valid). */
long ssd_net_get_tuning(const ssd_net* net, char* buf, size_t cap);
int ssd_net_set_tuning(ssd_net* net, const char* text);
/* How the last finalize chose its kernels: *from_table = conv layers taken from preset lines,
 * *timed = choices timed on the device (conv layers + whole-image blocks + launch mode).  timed == 0
 * means the table was complete: nothing depends on timing noise, results are reproducible bit for bit
 * across processes.  (The reference's Keras graph is deterministic in which kernels it runs; this is
 * the counterpart guarantee -- models/ssd_mobilenet_v2.py:7-35.) */
int ssd_net_tuning_stats(const ssd_net* net, int* from_table, int* timed);
/* Device memory a finalized net holds, bytes: out[0] activation arena (one fp32 slot per tensor x max_batch), out[1] bf16
 * planes of the activations its CHOSEN LDS-DMA conv tiles read (allocated for the finalize-time race, freed again where
 * no chosen tile reads them), out[2] partial-sum slabs of the whole-image block kernel, out[3] split-K slabs.  A lane
 * replica (models/decoder.py) holds the same again. */
int ssd_net_memory_bytes(const ssd_net* net, size_t out[4]);
/* ... and, on top of those, the fp16 weight planes of the whole-image blocks (option "image_f16x2"; 0 with the option off). */
size_t ssd_net_image_f16x2_bytes(const ssd_net* net);
/* Static bound of a named tensor of a finalized net: max |x| over EVERY input, computed at finalize from the weights alone
 * for the tensors a project conv behind a ReLU6 depthwise writes (alone or inside a fused block), a residual adding its
 * source's interval; < 0: no bound is known (other tensors, non-finite weights).  Recomputed by every finalize. */
float ssd_net_tensor_bound(const ssd_net* net, const char* tensor);
/* The interval arithmetic behind it, on the host (no device): output channel r of y = W' d + shift (+ residual) with d in
 * [0, 6]^k lies in [6 sum min(w', 0) + shift + res_lo, 6 sum max(w', 0) + shift + res_hi], w' = w[r * ld + c] * scale[r]
 * (scale / shift / res_lo + res_hi may be NULL: 1 / 0 / no residual).  Returns 1, or 0 if anything is not finite (no bound),
 * or a negative SSD_E_* code. */
int ssd_block_output_interval(const float* w, int n, int k, int ld, const float* scale, const float* shift, const double* res_lo,
                              const double* res_hi, double* lo, double* hi);
/* Exponent s = floor(log2(2^15 / bound)) of the input scale 2^s of the two-plane fp16 form of the whole-image blocks:
 * |2^s x| <= 2^15 for |x| <= bound.  Returns 1, or 0 (no fp16 form) for an unknown (< 0), zero or non-finite bound or |s| > 12. */
int ssd_f16x2_input_exp(float bound, int* s);
/* sha256 (first 16 hex digits) of the kernel sources this library was built from (csrc/build.sh);
 * shipped tuning tables record the build they were measured on. */
const char* ssd_build_id(void);
int ssd_net_num_priors(const ssd_net* net);
int ssd_net_feature_map_size(const ssd_net* net, int level);

/* image [B,S,S,3] fp32 in [0,1] (device) -> pred_deltas [B,N,4], pred_labels [B,N,L]
 * (softmax probabilities), exactly the pair the reference model outputs. */
int ssd_net_forward(ssd_net* net, const float* image_dev, int B, float* deltas_out_dev,
                    float* probs_out_dev, void* stream);

/* Forward + SSDDecoder (get_decoder_model(...).predict on one batch): priors [N,4] dev. */
int ssd_net_predict(ssd_net* net, const float* image_dev, int B, const float* priors_dev,
                    const float* var, int max_total, float iou_thr, float score_thr,
                    float* boxes_dev, float* labels_dev, float* scores_dev, int* valid_dev,
                    void* stream);
/* ... with the decoder of ssd_decode_nms_cfg (cfg->max_per_class and cfg->max_total are both honoured; ssd_net_predict is
 * max_per_class == max_total == max_total, SSD_NMS_HARD, per class).  Calls with different configs may alternate on one net. */
int ssd_net_predict_cfg(ssd_net* net, const float* image_dev, int B, const float* priors_dev, const float* var,
                        const ssd_nms_config* cfg, float* boxes_dev, float* labels_dev, float* scores_dev,
                        int* valid_dev, void* stream);

/* Debug/test hook: copy the activation of a named layer of the LAST forward to the host.
 * Returns the element count (or negative error); host_out may be NULL to query size. */
long ssd_net_fetch_activation(ssd_net* net, const char* layer, float* host_out, size_t cap);
/* ... and the same activation as the bf16 planes the LDS-DMA conv tiles read (csrc/ssd_convdma.hip), joined back to
 * fp32: *planes_out = 3 (exact split: equals the fp32 activation bit for bit) or 1 (its bf16 rounding); returns 0 when
 * no running layer asked for this tensor's planes in the last forward. */
long ssd_net_fetch_planes(ssd_net* net, const char* layer, float* host_out, size_t cap, int* planes_out);

/* Per-layer algorithmic work of one forward at batch B (for roofline accounting). */
int ssd_net_num_layers(const ssd_net* net);
const char* ssd_net_layer_name(const ssd_net* net, int i);
const char* ssd_net_layer_kind(const ssd_net* net, int i);   /* "conv","dw","pool",... */
const char* ssd_net_layer_config(const ssd_net* net, int i); /* autotuned conv tile config */
/* Which form of the whole-image block kernel runs layer i at batch B: -1 the layer is not routed to it, 0 fp32 MFMA,
 * 1 the bf16 mode, 3 the split-bf16 form, 2 the two-plane fp16 form (option "image_f16x2", a statically bounded input). */
int ssd_net_layer_image_form(const ssd_net* net, int i, int B);
double ssd_net_layer_flops(const ssd_net* net, int i, int B); /* 2*MACs                  */
double ssd_net_layer_bytes(const ssd_net* net, int i, int B); /* in + out + weights      */
/* FLOPs the chosen kernel issues: = layer_flops except Winograd layers (x 16/36, whole border tiles) */
double ssd_net_layer_executed_flops(const ssd_net* net, int i, int B);
/* Options: "use_graph" replays each forward/predict step as one captured hipGraph (keyed by the
 * pointers/sizes of the call; the NULL stream is served through an internal stream) -- by default
 * ssd_net_finalize races replay against direct launches on the device at max_batch and uses replay only
 * where it is more than 1 % ahead; setting the option pins the mode;
 * "fuse_blocks" (default 1) runs eligible MobileNetV2 inverted-residual blocks
 * (expand -> depthwise -> project) as one fused kernel; 0 runs them as three layers (then
 * every intermediate activation is inspectable); "fuse_dwproj" (default 1, needs fuse_blocks)
 * runs depthwise -> project of the remaining blocks (7-16) as one kernel behind the expand
 * GEMM; "fuse_image" (default 1, needs fuse_blocks) lets the whole-image block kernel (blocks
 * 7-12 / 14-16: expand -> depthwise -> project with the expanded map kept on the CU) replace expand
 * GEMM + depthwise/project where it won finalize's on-device race, 2 forces it wherever it applies,
 * 0 disables it; "image_split" (default 1; fp32 nets) also lets that kernel's split-bf16 form (fp32 results from six bf16
 * matrix products per product, weights staged through LDS) into the race -- table line "<block> image 2" --, 0 leaves
 * it out; "image_ticket" (default 0) makes that kernel combine its channel-group partial sums
 * inside the launch (arrival ticket, last arriver) instead of by a second launch; "overlap_heads" (default 1) runs the SSD head convs on side streams ("tail_on_side", default 0,
 * swaps the roles: big head convs on the caller's stream, the small tail layers on the side streams -- measured slower); "use_wino" (default 1)
 * offers the Winograd F(2x2,3x3) kernels to finalize's autotune for the 3x3 stride-1 convs;
 * "precision" (default 0 = fp32, the reference's arithmetic: trainer.py:50-54 has no mixed precision; 1 = bf16, this
 * build's extension for BASELINE.json configs[3] / [4]): every matrix operand of the dense / 1x1 convolutions is rounded
 * once to bf16 (nearest even), each product is one bf16 MFMA with fp32 accumulation ("bf16_*" tiles, the bf16 forms of
 * the stem, row-band and whole-image block kernels); BatchNorm shifts, activations, residual adds, depthwise taps, softmax and
 * the box math stay fp32, activations stay fp32 in HBM; the training step then runs its forward / backward-data convs
 * on the bf16 tiles (fp32 master weights, weight gradients and Adam).  Takes effect at the next finalize. */
int ssd_net_set_option(ssd_net* net, const char* name, int value);
/* Live per-layer hipEvent timing of ssd_net_forward / ssd_net_predict on their stream.
 * read_timing sums the durations (ms) of the forwards recorded since the last read into
 * ms_sum_out[num_layers + 1] (last entry: decode+NMS of predict) and reports their count. */
int ssd_net_set_timing(ssd_net* net, int enabled);
int ssd_net_read_timing(ssd_net* net, float* ms_sum_out, int* forwards_out);
/* Time every layer with hipEvents on `stream` (reps forwards); ms_out[num_layers]. */
int ssd_net_profile_layers(ssd_net* net, const float* image_dev, int B, int reps,
                           float* ms_out, void* stream);

/* =====================================================================================
 * Training step: what Keras runs for the reference's
 * `ssd_model.compile(optimizer=Adam(1e-3), loss=[loc_loss_fn, conf_loss_fn])` +
 * `ssd_model.fit(...)` (trainer.py:50-76), one call per phase so that the host can all-reduce
 * the flat gradient vector over RCCL between backward and the optimiser.
 * MobileNetV2 graph (BASELINE configs[3]); training-mode BatchNorm (batch statistics, moving
 * averages updated with momentum 0.999 / eps 1e-3 of keras-applications MobileNetV2).
 * ================================================================================== */
/* Plan the training buffers for `batch` images per step; moves the trainable parameters into
 * one flat vector (parameter-table order, Keras layouts; moving_mean / moving_variance are not
 * trainable).  Keeps the Adam state when re-planned for a larger batch. */
int ssd_net_train_begin(ssd_net* net, int batch);
size_t ssd_net_trainable_floats(const ssd_net* net);
/* Offset of a parameter inside the flat trainable vector (-1: unknown / not trainable). */
long ssd_net_trainable_offset(const ssd_net* net, const char* name);
/* Training-mode forward + ssd_loss + backward on one batch (device pointers):
 * image [B,S,S,3], actual_deltas [B,N,4], actual_labels [B,N,L] (calculate_actual_outputs).
 * grads_flat [ssd_net_trainable_floats] <- d mean_b(loc_b + conf_b) / d parameter (caller-owned);
 * loc_loss / conf_loss [B] <- per-image loss terms (nullable). */
int ssd_net_train_forward_backward(ssd_net* net, const float* image_dev, int B,
                                   const float* actual_deltas_dev, const float* actual_labels_dev,
                                   float neg_pos_ratio, float loc_loss_alpha, float* grads_flat_dev,
                                   float* loc_loss_dev, float* conf_loss_dev, void* stream);
/* The same step with the loss chosen by `loss` (SSD_LOSS_*): ssd_net_train_forward_backward is this call with kind
 * SSD_LOSS_HARD_NEGATIVE and its two numbers, and issues exactly the same launches.  The training state's loss workspace
 * is planned for the largest of the losses.  SSD_E_INVALID before any launch: a NULL `loss`, an unknown kind, a focal
 * alpha <= 0 or gamma < 0, a loc_kind outside SSD_LOC_HUBER .. SSD_LOC_CIOU, and beside a loc_kind other than
 * SSD_LOC_HUBER NULL or misaligned priors or variances that are not finite and > 0.  With loc_kind == SSD_LOC_HUBER the
 * launches are exactly those of the struct's first five fields. */
int ssd_net_train_forward_backward_cfg(ssd_net* net, const float* image_dev, int B,
                                       const float* actual_deltas_dev, const float* actual_labels_dev,
                                       const ssd_loss_config* loss, float* grads_flat_dev,
                                       float* loc_loss_dev, float* conf_loss_dev, void* stream);
/* Gradient buckets for the batch data-parallel step (the reference trains on one device, trainer.py:50-76; the
 * RCCL exchange is this build's SURVEY.md 8e row 2): bucket k = flat offsets [lo[k], lo[k + 1]), lo ascending
 * from 0.  The backward finishes the flat gradient vector from its end (heads first, stem last) and records an
 * event per bucket when it is final; ssd_net_train_wait_bucket(net, k, stream) orders `stream` -- the one the
 * all-reduce of bucket k is issued on -- behind that point, so the exchange overlaps the rest of the backward. */
int ssd_net_train_set_buckets(ssd_net* net, int n, const long* lo);
int ssd_net_train_wait_bucket(ssd_net* net, int k, void* stream);
/* Adam (Keras defaults beta1 0.9, beta2 0.999, eps 1e-7; TF ApplyAdam form) on every trainable
 * parameter; grads are multiplied by grad_scale first (1/world_size after a SUM all-reduce).
 * This is ssd_net_optimizer_step (below) with kind = SSD_OPT_ADAM and every clip off, under an older signature: the
 * same launch, the same checks in the same order, the same return codes.  So a beta1 or beta2 outside [0, 1) is
 * refused with SSD_E_INVALID (it used to go through and give a NaN step length).
 * The update's roundings are fixed in the source: g = grad * grad_scale is rounded before g - m, and
 * m + (g - m)(1 - beta1) takes three roundings.  With grad_scale == 1 and nothing frozen or clipped these are the bits
 * this call always gave; with grad_scale != 1 (the data-parallel step), frozen layers or a clip, m and var can differ
 * in the last bit from what earlier builds gave, which fused some of these operations depending on the kernel. */
int ssd_net_adam_step(ssd_net* net, const float* grads_flat_dev, float lr, float beta1, float beta2,
                      float eps, float grad_scale, void* stream);
long ssd_net_train_steps(const ssd_net* net);
/* The optimizers of the reference's trainer (`from tensorflow.keras.optimizers import SGD, Adam`) with the Keras
 * gradient-clipping arguments, TF 2.x semantics on fp32 state.  g = grads_flat * grad_scale (the averaged gradient;
 * clipping acts on g):
 *   SGD (training_ops ApplyKerasMomentum): accum = momentum * accum - lr * g; var += accum, with nesterov
 *     var += momentum * accum - lr * g; momentum == 0: var -= lr * g, no accumulator is read or written.  The
 *     accumulator is the slot "m"; "v" is left alone.
 *   Adam (training_ops ApplyAdam): m += (g - m)(1 - beta1); v += (g * g - v)(1 - beta2);
 *     var -= lr * sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps), t the step counter after this step.
 *   clipnorm c (tf.clip_by_norm per Keras variable = entry of the parameter table; the label and the box kernel of a
 *     fused head conv are two): s = sum(g * g), norm = s > 0 ? sqrt(s) : s, g = (g * c) / max(norm, c).
 *   global_clipnorm c (tf.clip_by_global_norm over all trainable variables): gn = sqrt(sum of all s),
 *     g *= c * min(1 / gn, 1 / c).  Excludes clipnorm.
 *   clipvalue c: g = min(max(g, -c), c), after the norm clip when both are set.
 * Frozen variables (ssd_net_set_trainable) are not read, not written and not counted in any norm.
 * Launches: one (the update over the table of trainable segments) without norm clipping, three with it (per-segment
 * sums of squares in a fixed tree, per-variable sums of those in table order in double, the update); no atomics, the
 * same inputs give the same bits in every run.  Every setting is an instantiation of the one update kernel over the one
 * table, Adam with every clip off (ssd_net_adam_step) included: what a step does to an element does not depend on what
 * else is trainable.
 * The state remembers which kind wrote the slots: a step of another kind (ssd_net_adam_step included) while the step
 * counter is non-zero returns SSD_E_STATE -- call ssd_net_optimizer_reset (slots = 0, step counter = 0; a no-op before
 * ssd_net_train_begin).  SSD_E_INVALID, nothing launched: NULL pointers, an unknown kind, momentum outside [0, 1], a
 * beta outside [0, 1), clipnorm and global_clipnorm both > 0, an unknown slot, a wrong count.
 * The slots ("m" | "v") are flat vectors in ssd_net_trainable_offset order; get returns the count (host_out NULL:
 * query).  ssd_net_train_set_steps sets the step counter (restoring a saved state). */
#define SSD_OPT_ADAM 0
#define SSD_OPT_SGD 1
typedef struct ssd_optimizer {
    int kind;
    float beta1, beta2, eps;                     /* Adam */
    float momentum;
    int nesterov;                                /* SGD  */
    float clipnorm, clipvalue, global_clipnorm;  /* <= 0: off */
} ssd_optimizer;
int ssd_net_optimizer_step(ssd_net* net, const float* grads_flat_dev, const ssd_optimizer* opt, float lr,
                           float grad_scale, void* stream);
int ssd_net_optimizer_reset(ssd_net* net);
long ssd_net_optimizer_get_state(ssd_net* net, const char* slot, float* host_out, size_t cap);
int ssd_net_optimizer_set_state(ssd_net* net, const char* slot, const float* host_in, size_t count);
int ssd_net_train_set_steps(ssd_net* net, long steps);
/* Measurement: matrix-core FLOPs the last ssd_net_train_forward_backward issued, per instruction family --
 * out3[0] conv forward + backward-data on fp32-MFMA tiles, out3[1] the same on split-bf16 tiles (six bf16 MFMAs per
 * fp32 product), out3[2] weight gradients (fp32 MFMA).  bench.py --train prices each family at its own peak. */
int ssd_net_train_matrix_flops(const ssd_net* net, double* out3);
/* Sum of the layers' regularisation losses at the current weights: 5e-4 * sum(kernel^2) over VGG16's
 * backbone / extra convs (reference models/ssd_vgg16.py:44-45), 0 for MobileNetV2.  Keras adds this term to
 * the `loss` and `val_loss` that fit() logs and ModelCheckpoint(save_best_only) monitors (trainer.py:56-63).
 * Synchronous (legacy stream, one float copied to the host). */
int ssd_net_regularization_loss(ssd_net* net, float* host_out);
/* Fine-tuning: Keras' `layer.trainable = False`, by KERAS LAYER NAME -- a parameter name up to its last '/':
 * "Conv1", "bn_Conv1", "block_3_depthwise_BN", "extra2_1", "4_conv_boxes_output", "l2_normalization".  A conv and its
 * BatchNorm are two Keras layers and freeze independently, as do the label and the box conv of one head level.  By
 * default every layer is trainable and the step is the one it always was (same bits).  Both calls work
 * before and after ssd_net_train_begin, need no device, and take effect at the next ssd_net_train_forward_backward /
 * ssd_net_adam_step.  Unknown name: SSD_E_INVALID (get: too).
 *   frozen kernel / bias / L2-norm scale: no gradient is computed, its range of grads_flat holds exactly 0.0f after
 *     ssd_net_train_forward_backward (the flat vector keeps its size, order and offsets; so do the gradient buckets);
 *   frozen BatchNorm: TF 2.0 semantics -- inference mode.  It normalises with moving_mean / moving_variance (eps 1e-3),
 *     makes no statistics pass, leaves the moving statistics bitwise alone and produces no dgamma / dbeta;
 *   pruning: a tensor needs a gradient only if a trainable parameter lies upstream of it; no data gradient and no
 *     residual add go into a tensor that needs none, a layer without trainable parameters whose inputs need none is
 *     left out of the backward altogether (ssd_net_train_plan);
 *   the optimizer step leaves var, m and v of frozen ranges bitwise untouched (they are in no segment of its table: the
 *     same launches, the same bits for every element that stays trainable); the step counter stays global.  Unlike
 *     Keras -- which rebuilds the optimizer at the compile() that must follow a change of `trainable` -- the moments
 *     of a layer that is unfrozen later continue from where they were.
 * ssd_net_regularization_loss is unchanged: Keras keeps the regularisation term of frozen kernels in `loss`. */
int ssd_net_set_trainable(ssd_net* net, const char* keras_layer, int trainable);
int ssd_net_get_trainable(const ssd_net* net, const char* keras_layer);   /* 1 / 0, SSD_E_INVALID: unknown name */
/* The backward plan of layer `layer` (index of ssd_net_layer_name) under the current flags, from the graph and the
 * flags alone (no device, no ssd_net_train_begin): *flags = OR of SSD_PLAN_*.  0 for a layer the training step does not
 * run (the fused-block and softmax entries of the layer list). */
#define SSD_PLAN_WGRAD 1       /* gradient of the kernel (+ bias) / of the L2-norm scale                          */
#define SSD_PLAN_WGRAD2 2      /* head conv: gradient of the box kernel (+ bias); SSD_PLAN_WGRAD is the label one   */
#define SSD_PLAN_DGRAD 4       /* data gradient into the layer's input                                             */
#define SSD_PLAN_RESGRAD 8     /* the output gradient is handed to the residual tensor                             */
#define SSD_PLAN_BN_BATCH 16   /* BatchNorm on batch statistics (moving averages updated)                          */
#define SSD_PLAN_BN_PARAMS 32  /* dgamma / dbeta                                                                   */
#define SSD_PLAN_SKIP 64       /* nothing trainable, no input needs a gradient: not in the backward at all         */
int ssd_net_train_plan(const ssd_net* net, int layer, int* flags);
/* Debug / parity hook: copy a buffer of the last training forward/backward (batch B) to the host:
 * "probs", "deltas", "grad_logits", "grad_deltas", "<tensor>", "grad:<tensor>", "pre:<layer>",
 * "mean:<layer>", "var:<layer>".  Returns the element count (host_out NULL: query). */
long ssd_net_train_fetch(ssd_net* net, const char* what, int B, float* host_out, size_t cap);

/* Test / bench hooks of the training backward kernels on caller-owned memory (the kernels and launch plans of
 * ssd_net_train_forward_backward, outside a net).
 *
 * Weight gradient of a dense conv: dW [kh,kw,Cin,N] (Keras HWIO) = im2col(x)^T * g, x [B,H,W,Cin] the forward input
 * of geometry `d` (d->Cout, act and has_residual are not used), g [B*Ho*Wo][ldg] the gradient of the conv output of
 * which the first N columns are taken (ldg >= N: a head conv's padded dY; g_dev may point at a column offset).
 * `config` selects one of ssd_conv_wgrad_num_configs() MFMA tile shapes, -1 the padded-area heuristic.  The M chunks'
 * partial sums need ssd_conv_wgrad_workspace_floats(d, N) floats of workspace (enough for every config; more than
 * kh*kw*Cin*N floats means more than one chunk).  SSD_E_INVALID, nothing launched: NULL pointers, bad geometry, a
 * config out of range, ldg < N, a workspace that is too small. */
int ssd_conv_wgrad_num_configs(void);
size_t ssd_conv_wgrad_workspace_floats(const ssd_conv_desc* d, int N);
int ssd_conv2d_wgrad_ex(const ssd_conv_desc* d, const float* x_dev, const float* g_dev, int ldg, int N, int config,
                        float* dW_dev, float* workspace_dev, size_t workspace_floats, void* stream);
/* Backward of the 3x3 depthwise conv (pads after = 1, as TF SAME and keras correct_pad give for k = 3:
 * Ho = (H + pad_t + 1 - 3) / stride + 1): dw [3,3,C] from x [B,H,W,C] and g [B,Ho,Wo,C]; dx [B,H,W,C] = (accumulate ?
 * dx : 0) + the data gradient under w [3,3,C].  C % 4 == 0, stride 1 or 2, pads 0 or 1, 16-byte aligned tensors;
 * 9 * C * ceil(B*Ho*Wo / 64) floats of workspace always suffice.  Anything else is SSD_E_INVALID, nothing launched. */
int ssd_dwconv3x3_backward(const float* x_dev, const float* g_dev, const float* w_dev, int B, int H, int W, int C, int stride,
                           int pad_t, int pad_l, int accumulate, float* dx_dev, float* dw_dev, float* workspace_dev,
                           size_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_H */
