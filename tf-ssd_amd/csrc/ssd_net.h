// Shared definitions of the graph runner (ssd_net.hip) and the training step (ssd_train.hip):
// parameter table, activation tensors, layer list and the net object behind `ssd_net*`.
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "ssd_conv.h"

struct ssd_train_state;      // csrc/ssd_train.h
void ssd_train_state_free(ssd_train_state*);

namespace ssd {

enum LayerKind { LK_CONV = 0, LK_DW, LK_POOL, LK_L2NORM, LK_SOFTMAX, LK_FUSED };
static const char* kKindName[] = {"conv", "dw", "pool", "l2norm", "softmax", "fused"};

// Which kernel runs a layer.  RT_OFF: none (a fused layer that is switched off or whose shape no fused kernel takes; a
// member of a fused layer that runs).  RT_LAYER: the layer's own kernel (conv / dw / pool / l2norm / softmax).  The
// rest are the kernel families of an LK_FUSED layer; the precision suffix of their names follows ssd_net::precision.
enum Route { RT_OFF = 0, RT_LAYER, RT_STEM, RT_DWPROJ, RT_TILE, RT_BAND, RT_BAND3, RT_IMAGE, RT_IMAGE_SPLIT };
inline bool route_is_image(Route r) { return r == RT_IMAGE || r == RT_IMAGE_SPLIT; }     // the whole-image kernel, any form

// Who writes the planes of a layer's output while they are live (plane_writer, ssd_storage.hip).  PW_NONE: nobody, they
// are not live.  PW_KERNEL: the layer's own kernel, from registers.  PW_PASS: a split pass over the fp32 copy behind it.
enum PlaneWriter { PW_NONE = 0, PW_KERNEL, PW_PASS };
enum PlaneOutput { PO_OUT = 0, PO_E_OUT };     // Layer::out / Layer::e_out

struct Param {
    std::string name;
    std::vector<int> shape;
    size_t count = 0;
    float* dev = nullptr;
    bool set = false;
    bool in_flat = false;     // dev points into the training step's flat parameter buffer (not freed per param)
};

struct Tensor {
    std::string name;
    int H = 0, W = 0, C = 0;
    size_t per_image = 0;     // floats
    float* dev = nullptr;     // arena slot, max_batch images
    // the same activation as bf16 planes [planes_np][plane_stride] for the LDS-DMA conv tiles of its consumers
    // (csrc/ssd_convdma.hip): allocated at finalize for every tensor a dense conv with Cin % 32 == 0 reads (option
    // "conv_dma", finalize_planes), kept where a chosen tile reads them (finalize_free_unread_planes), WRITTEN -- by the
    // producer's kernel or by a split pass, Layer::w_out -- only while a running consumer's chosen configuration is an
    // LDS-DMA tile: planes_live.  planes_live and plane_only are written by resolve_storage (ssd_storage.hip) alone
    short* planes = nullptr;
    long plane_stride = 0;    // elements between planes
    int planes_np = 0;        // 3: exact split h, m, l (fp32 nets); 1: bf16 rounding (the bf16 mode); 2: the fp16 pair of 2^8 x (fp32 nets, a
                              // ReLU6-bounded tensor whose plane readers all chose "dmah_*" tiles: finalize_resolve_f16x2, ssd_storage.hip)
    int planes_cap = 0;       // planes the allocation holds (planes_np <= planes_cap)
    bool planes_live = false;
    // the planes ARE the tensor: its producer skips the fp32 store into `dev` (the arena slot stays, unwritten).  Decided by
    // plan_storage (ssd_storage.hip): planes live, every running reader a dense conv on an LDS-DMA tile, the producer a
    // kernel whose plane store needs no fp32 copy (PW_KERNEL), option "plane_only" 1.  Inference only: the training step
    // keeps activations of its own.  ssd_net_fetch_activation joins the planes (h + m + l is exact)
    bool plane_only = false;
    // static bound of the tensor, from the weights alone (finalize_tensor_bounds, ssd_net.hip): every value any input can
    // produce lies in [blo[c], bhi[c]] for channel c; bound = max |.| over the channels, < 0: no bound is known
    std::vector<double> blo, bhi;
    float bound = -1.f;
};

struct Layer {
    std::string name;
    LayerKind kind = LK_CONV;
    int in = -1, out = -1, res = -1;          // tensor ids (out == -1: head conv -> net outputs)
    int H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, Cout = 0;
    int kh = 1, kw = 1, stride = 1, dil = 1, pt = 0, pl = 0, pb = 0, pr = 0, act = 0;
    int p_kernel = -1, p_bias = -1, p_bn = -1;  // p_bn: index of gamma (beta, mean, var follow)
    int p_kernel2 = -1, p_bias2 = -1, Cout1 = 0; // fused head conv: second (boxes) kernel/bias, label width
    int p_gamma = -1;                           // l2norm scale
    // head routing (floats): level offset, batch stride, pixel stride for the label part
    // (head_*) and the box part (head2_*); head_kind 3 = fused label+box head conv of one level
    int head_kind = 0;
    long head_off = 0, head_bs = 0, head_ps = 0;
    long head2_off = 0, head2_bs = 0, head2_ps = 0;
    // derived at finalize
    float* packed = nullptr;
    float* wino = nullptr;          // Winograd F(2x2,3x3) weights (3x3 stride-1 convs), see ssd_wino.hip
    float* scale = nullptr;
    float* shift = nullptr;
    int cfg = -1;
    int split_k = 1;
    float* wh = nullptr;            // fp16 planes [2][Kpad / 32][Npad][32] of 2^wh_k w for the "dmah_*" tiles: conv layers of fp32 nets whose
    int wh_k = 0;                   // input is ReLU6-bounded and whose weights are finite (ssd_bf16x3.h); kept while the chosen tile reads them
    // fused inverted-residual block: LK_FUSED layer points at its three member layers;
    // members carry the index of their LK_FUSED layer in `fused_by`
    int f_expand = -1, f_dw = -1, f_project = -1;
    int f_type = 0;                 // 0: inverted-residual block, 1: stem (Conv1 -> dw -> project),
                                    // 2: depthwise + project (the expand conv stays a GEMM of its own)
    int fused_by = -1;
    int e_out = -1;                 // whole-block LK_FUSED layer that must ALSO materialise its expanded map: that tensor
                                    // (block 13, whose expanded map is SSD feature map #1)
    int img_choice = -1;            // whole-block LK_FUSED layers the image kernel can run: 1 / 2 = its fp32-MFMA / split-bf16 form (with option image_f16x2 and a statically bounded input: the two-plane fp16 form in its place, same table line) won the finalize-time race against the layer kernels, 0 = it lost, -1 = not timed
    int fused_by2 = -1;             // depthwise / project members: their type-2 LK_FUSED layer
    Route route = RT_OFF;           // what runs this layer under the current options and tuning choices (resolve_routes, ssd_net.hip)
    PlaneWriter w_out = PW_NONE, w_e_out = PW_NONE;     // who writes the planes of `out` / `e_out` (resolve_storage, ssd_storage.hip, alone)
    float* splitk_part = nullptr;   // this layer's own split-K slab (layers may run concurrently)
    // LK_FUSED: weight copies with the folded BatchNorm scale multiplied in (per output channel)
    float *fz_we = nullptr, *fz_wd = nullptr, *fz_wp = nullptr;
    float *fz_we3 = nullptr, *fz_wp3 = nullptr;      // bf16 planes of fz_we / fz_wp for the split-bf16 band kernel (ssd_band3.hip)
    // whole-block LK_FUSED layers the image kernel's second form takes, fp32 nets, option image_f16x2: the fp16 pairs
    // [2][Ce][kpad_e] of 2^f16_ke fz_we and [2][npad_p][kpad_p] of 2^f16_kp fz_wp, and the exponent f16_s of the input's
    // scale from its static bound; nullptr: the block has no bounded input (or non-finite weights) and keeps the bf16 split
    float *fz_weh = nullptr, *fz_wph = nullptr;
    int f16_ke = 0, f16_kp = 0, f16_s = 0;
    int side = 0;                   // 1, 2: runs on that side stream (SSD head convs)
    hipEvent_t ev_ready = nullptr;  // recorded on the main stream when this layer's OUTPUT is complete
};

// Output routing of the fused label + box head conv of one level: columns below Cout1 go into the concatenated [B,N,L]
// label tensor `probs`, the rest into the [B,N,4] box tensor `deltas` (inference and training forward alike)
inline void conv_route_head(ConvParams& p, const Layer& l, float* probs, float* deltas) {
    p.out = probs + l.head_off;
    p.out_pixel_stride = l.head_ps;
    p.out_batch_stride = l.head_bs;
    p.n_split = l.Cout1;
    p.out2 = deltas + l.head2_off;
    p.out2_pixel_stride = l.head2_ps;
    p.out2_batch_stride = l.head2_bs;
    p.vec_store2 = (p.out2_pixel_stride % 4 == 0) && (p.out2_batch_stride % 4 == 0);
}

// Scope guards: the early error returns of the tuning / profiling entry points must not leak
struct ScopedDev {
    float* p = nullptr;
    ~ScopedDev() { if (p) (void)hipFree(p); }
};
struct ScopedEvent {
    hipEvent_t e = nullptr;
    ~ScopedEvent() { if (e) (void)hipEventDestroy(e); }
};
// The one timing primitive of the on-device races and the layer profile: two events, created once, that time ONE window
// (record, `reps` calls of `launch()`, record, synchronise, elapsed ms).  How many windows, which one warms up, how two
// alternatives interleave and when a candidate is given up stay with the caller.  window() returns the first non-zero
// launch() result (no synchronise then) or SSD_E_HIP from the synchronise, with *ms 0, for a caller that goes on regardless.
struct EventPair {
    ScopedEvent e0, e1;
    int create() {
        SSD_HIP(hipEventCreate(&e0.e));
        SSD_HIP(hipEventCreate(&e1.e));
        return SSD_OK;
    }
    template <class Launch>
    int window(hipStream_t st, int reps, Launch launch, float* ms) {
        *ms = 0.f;
        int rc = SSD_OK;
        (void)hipEventRecord(e0.e, st);
        for (int r = 0; r < reps && !rc; ++r) rc = launch();
        (void)hipEventRecord(e1.e, st);
        if (rc) return rc;
        SSD_HIP(hipEventSynchronize(e1.e));
        (void)hipEventElapsedTime(ms, e0.e, e1.e);
        return SSD_OK;
    }
};

// One launch of the forward's plan (plan_steps, ssd_net.hip, the fields' one writer): order, stream and cross-stream
// waits -- nothing about storage.  A pure function of the graph, the options, the routes and `timing`, built at the
// first forward that needs it and kept until ssd_net::drop_graphs().
struct Step {
    int layer = -1;
    int sid = -1;                   // stream: -1 the caller's (main), 0 / 1 ssd_net::side[]
    int wait[2] = {-1, -1};         // layers on another stream that produce its input / residual: wait for their ev_ready
    bool after_main = false;        // first work of a side stream whose input no layer produces: ordered behind the main stream
    bool publishes = false;         // a consumer runs on another stream: record ev_ready behind it
    bool join_first = false;        // the softmax: the side streams join the main stream in front of it
};

}  // namespace ssd

struct ssd_net {
    int backbone = 0, img_size = 300, levels = 6, L = 21;
    std::vector<int> n_ars;
    std::vector<ssd::Param> params;
    std::map<std::string, int> param_index;
    std::vector<ssd::Tensor> tensors;
    std::map<std::string, int> tensor_index;
    std::vector<ssd::Layer> layers;
    std::vector<int> fmap;          // feature-map size per level
    std::vector<long> level_off;    // prior offset per level
    int num_priors = 0;
    bool finalized = false;
    bool fuse_blocks = true;        // run eligible inverted-residual blocks as one fused kernel
    bool fuse_softmax = true;       // ssd_net_predict: the softmax runs inside the decoder's compaction kernel (csrc/ssd_decode.hip) instead of as a pass of its own
    bool fuse_dwproj = true;        // ... and depthwise + project of the others as one kernel
    bool use_wino = true;           // offer the Winograd F(2x2,3x3) kernels to the autotune
    int precision = 0;              // 0: fp32 results everywhere (the reference's arithmetic); 1: "bf16" -- every matrix operand of the dense / 1x1 convs rounded once to bf16, one bf16 MFMA per product, fp32 accumulation and epilogues (BASELINE.json configs[3] / [4])
    int fuse_band = 2;              // blocks 1-6: 2 row-band kernel with the 1x1 convs on the bf16 matrix cores through an exact 3-way split (ssd_band3.hip), 1 row-band kernel on the fp32 MFMA (ssd_bandblock.hip), 0 the 8x8-tile kernel
    int fuse_image = 1;             // whole-image block kernel (ssd_imgblock.hip): 0 never, 1 where it won the finalize-time race, 2 wherever it applies
    int lanes_hint = 1;             // replicas of this net running concurrently (lanes): the whole-image kernel then splits an image's expanded channels over fewer workgroups (B x groups x lanes fills the CUs; fewer slab passes)
    bool tail_on_side = false;      // diagnostics: big heads on the main stream, extras tail + small heads on the side streams
    bool image_split = true;        // fp32 nets: the finalize-time race also times the image kernel's split-bf16 form (img_choice 2; option "image_split" 0: leave it out)
    bool image_v2 = true;           // whole-image kernel only (the row-band kernels of blocks 1-6 have one form): the second form (ssd_imgblock2.hip: compile-time geometry, adjacent pixels per lane) where it has a configuration; 0 = the first form (A/B; equal within tolerance, not bitwise: the k-slot order inside the project MFMAs differs)
    bool conv_dma = true;           // offer the LDS-DMA tiles over pre-split activation planes (ssd_convdma.hip) to the autotune / accept them from tables
    bool conv_f16x2 = true;         // accept the two-plane fp16 tiles ("dmah_*") from tables / offer them to the autotune; 0: a "dmah_*" line runs its "dma3_*" twin (the same tile and split-K)
    bool dma_ring = true;           // "dmah_*" tiles with one k-step per barrier run the three-stage LDS ring (ssd_convdma.hip); 0: the two-stage loop, the same bits
    bool image_f16x2 = true;        // whole-image blocks of fp32 nets on the split route (img_choice 2): the two-plane fp16 form (three fp16 MFMAs per product in both 1x1 GEMMs) where the block's input has a static bound (Tensor::bound); 0: the split-bf16 form everywhere
    bool plane_only = true;         // drop the fp32 copy of an activation whose readers all take its bf16 planes (Tensor::plane_only); 0: store both
    bool image_ticket = false;      // combine the channel-group slabs inside the launch (arrival ticket) instead of by a second launch
    float* img_slabs = nullptr;     // its partial-sum slabs and arrival tickets (sized for max_batch)
    unsigned* img_tickets = nullptr;
    int max_batch = 0;
    int last_batch = 0;
    std::vector<float*> owned;      // device allocations to free
    float* arena = nullptr;
    size_t arena_bytes = 0, plane_bytes = 0, slab_bytes = 0;    // ssd_net_memory_bytes
    size_t wplane_bytes = 0;        // the fp16 weight planes of the layers on "dmah_*" tiles (counted with the planes)
    size_t iplane_bytes = 0;        // the fp16 weight planes of the whole-image blocks (option image_f16x2; counted with the planes)
    float* splitk_ws = nullptr;
    size_t splitk_floats = 0;
    // predict() scratch
    float* deltas = nullptr;
    float* probs = nullptr;
    void* nms_ws = nullptr;
    size_t nms_ws_bytes = 0;
    int nms_ws_batch = 0;           // the batch the workspace was carved (and its candidate counters zeroed) for
    int nms_ws_total = 0;           // ... and the max_total it was carved for
    int scratch_batch = 0;          // batch capacity deltas/probs were allocated for
    std::map<std::string, std::pair<std::string, int>> preset;   // layer -> (config name, split_k)
    int n_preset = 0;               // conv layers the last finalize took from preset lines
    int n_autotuned = 0;            // choices the last finalize timed on the device (0 = fully reproducible table)
    bool launch_raced = false;      // the graph-replay / direct-launch choice was made by a race or a preset line
    // hipGraph replay of a whole forward/predict step, keyed by every pointer baked into it
    bool use_graph = true;
    bool graphs_unsafe = false;     // GPU_MAX_HW_QUEUES < 4 in the environment: never capture / replay
    bool use_graph_auto = true;     // finalize races graph replay against direct launches (until "use_graph" is set explicitly)
    struct GraphEntry {
        std::vector<const void*> key;
        hipGraphExec_t exec = nullptr;
        hipGraph_t graph = nullptr;
        const float* image = nullptr;   // restored on replay (fetch_activation / profile hooks read them)
        int batch = 0;
    };
    std::vector<GraphEntry> graphs;
    // graphs cannot be captured on the legacy NULL stream (PyTorch's default stream): such
    // calls are captured/replayed on this BLOCKING stream, which the NULL stream implicitly
    // orders with (legacy default-stream semantics), so callers see the same ordering.
    hipStream_t gstream = nullptr;
    // the head convs only depend on their feature map: they run on `side` concurrently with the
    // rest of the backbone / extras (fork after the producer, join before the softmax)
    bool overlap_heads = true;
    static constexpr int kSides = 2;
    hipStream_t side[kSides] = {nullptr, nullptr};
    hipEvent_t ev_side_done[kSides] = {nullptr, nullptr};
    std::vector<ssd::Step> steps;       // the forward's launch plan (empty: not built for the current state)
    float* splitk_layers = nullptr;     // per-layer split-K slabs (post-autotune)
    bool timing = false;                // optional per-layer hipEvent timing of forward()/predict() (bench.py roofline leg)
    ssd_train_state* train = nullptr;    // training step state (csrc/ssd_train.h), lazily created
    // fine-tuning: Keras layer names (a parameter name up to its last '/') whose `trainable` is False; trainable_rev counts
    // the changes (the training step re-plans its backward when it lags behind: ssd_net_set_trainable, csrc/ssd_train.hip)
    std::set<std::string> frozen;
    unsigned trainable_rev = 0;
    std::vector<std::vector<hipEvent_t>> timing_events;   // one vector of (layers + 2) events per forward

    ~ssd_net() {
        for (auto& p : params)
            if (p.dev && !p.in_flat) (void)hipFree(p.dev);
        if (train) ssd_train_state_free(train);
        for (float* p : owned)
            if (p) (void)hipFree(p);
        if (arena) (void)hipFree(arena);
        if (splitk_ws) (void)hipFree(splitk_ws);
        if (deltas) (void)hipFree(deltas);
        if (probs) (void)hipFree(probs);
        if (nms_ws) (void)hipFree(nms_ws);
        for (auto& v : timing_events)
            for (auto e : v) (void)hipEventDestroy(e);
        drop_graphs();
        if (gstream) (void)hipStreamDestroy(gstream);
        for (int k = 0; k < kSides; ++k) {
            if (side[k]) (void)hipStreamDestroy(side[k]);
            if (ev_side_done[k]) (void)hipEventDestroy(ev_side_done[k]);
        }
        for (auto& l : layers)
            if (l.ev_ready) (void)hipEventDestroy(l.ev_ready);
        if (splitk_layers) (void)hipFree(splitk_layers);
    }
    // whatever a captured graph bakes in has changed: drop the graphs, and the launch plan with them
    void drop_graphs() {
        steps.clear();
        for (auto& g : graphs) {
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
            if (g.graph) (void)hipGraphDestroy(g.graph);
        }
        graphs.clear();
    }
};

namespace ssd {

// ---- what the kernel-selection unit (ssd_tune.hip) needs of the graph runner (ssd_net.hip)
// (as_read_by: a CONV_READS_* family that is to read the input's planes whatever form they have now; -1: as they stand)
ConvParams layer_conv_params(const ssd_net& net, const Layer& l, int B, const float* in, float* out, const float* res,
                             float* deltas_out, float* probs_out, int as_read_by = -1);
int run_layer(ssd_net& net, const Layer& l, int B, float* deltas_out, float* probs_out, hipStream_t st, int cfg_override = -1);
void resolve_routes(ssd_net& net);
inline bool layer_runs(const Layer& l) { return l.route != RT_OFF; }
bool image_kernel_takes(const ssd_net& net, const Layer& f);
ImagePlan image_plan(const ssd_net& net, const Layer& f, int B, FusedBlockParams* shape = nullptr, bool probe_pairs = false);
int dev_alloc(ssd_net& net, size_t floats, float** out);
void dev_free(ssd_net& net, float* p);

// ---- ... and ssd_net_finalize of that unit: the four steps that choose, in the order finalize takes them
int finalize_apply_preset(ssd_net* net, int max_batch, bool* image_preset_ok);    // the table's lines, where they can run
int autotune(ssd_net& net, int B, hipStream_t st);                                // conv layers without one: raced
int tune_image_blocks(ssd_net& net, int B, hipStream_t st);                       // whole-image blocks without one: raced
int tune_launch_mode(ssd_net* net, int B);                                        // graph replay or direct launches: read or raced

// ---- the activation-storage unit (ssd_storage.hip): its rule, its pure resolver and the one writer of the resolved fields
struct StoragePlan {
    std::vector<char> live, only;               // per tensor: Tensor::planes_live, Tensor::plane_only
    std::vector<PlaneWriter> w_out, w_e_out;    // per layer: Layer::w_out, Layer::w_e_out
};
PlaneWriter plane_writer(const ssd_net& net, const Layer& l, int cfg, PlaneOutput which);
StoragePlan plan_storage(const ssd_net& net);
void resolve_storage(ssd_net& net);             // beside resolve_routes: ssd_net_create, ssd_net_set_option, the end of ssd_net_finalize
int planes_pass(ssd_net& net, int tensor, int B, hipStream_t st);
bool tensor_relu6_bounded(const ssd_net& net, int t);
int dmah_or_twin(const ssd_net& net, const Layer& l, int cfg, bool pair = true);
int finalize_planes(ssd_net* net, int max_batch, hipStream_t st);     // ... and its finalize steps, in the order finalize takes them
void finalize_resolve_f16x2(ssd_net* net);
int finalize_free_unread_planes(ssd_net* net, hipStream_t st);
long fetch_tensor(ssd_net* net, const char* who, const char* layer, float* host_out, size_t cap, bool want_planes, int* planes_out);

}  // namespace ssd
