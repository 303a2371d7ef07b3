// Kernel selection: everything that decides, at finalize, which kernel runs a layer.  The table's text (one parser, one
// writer), the three on-device races that fill in what a table lacks (conv tiles and split-K, whole-image blocks, graph
// replay against direct launches; their one timing primitive is EventPair, ssd_net.h) and the per-tensor rule that settles
// whether a tensor's readers take its fp32 copy, its bf16 planes or its fp16 pair.  ssd_net_finalize (ssd_net.hip) calls
// finalize_apply_preset, autotune, tune_image_blocks and tune_launch_mode, in this order.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ssd_net.h"

using namespace ssd;

extern "C" {

// The table's text: "layer config split_k" with split_k in 1..64, "block image 0|1|2", "__launch graph 0|1" (0..64 is
// read).  Comment and empty lines are skipped; any other line is dropped, and what it would have named is raced.
int ssd_net_set_tuning(ssd_net* net, const char* text) {
    SSD_CHECK_ARG(net && text, "ssd_net_set_tuning: NULL argument");
    net->preset.clear();
    for (const char* p = text; *p;) {
        const std::string line(p, strcspn(p, "\n"));         // (a copy: sscanf must not read on into the next line)
        p += line.size() + (p[line.size()] == '\n');
        char name[128], word[128];
        int n = 1;
        if (line.empty() || line[0] == '#' || sscanf(line.c_str(), "%127s %127s %d", name, word, &n) != 3) continue;
        const bool flag = !strcmp(word, "image") || !strcmp(word, "graph");
        if (n >= (flag ? 0 : 1) && n <= 64) net->preset[name] = {word, n};
    }
    net->finalized = false;
    return SSD_OK;
}

// ... and written: a line per conv layer with a configuration, per block the image kernel can run, the launch mode's.
long ssd_net_get_tuning(const ssd_net* net, char* buf, size_t cap) {
    if (!net) return SSD_E_INVALID;
    std::string out;
    for (const auto& l : net->layers)
        if (l.kind == LK_CONV && l.cfg >= 0)
            out += l.name + " " + conv_config_name(l.cfg) + " " + std::to_string(l.split_k) + "\n";
    for (const auto& l : net->layers)
        if (l.img_choice >= 0 && image_kernel_takes(*net, l)) out += l.name + " image " + std::to_string(l.img_choice) + "\n";
    if (net->finalized && net->use_graph_auto && net->launch_raced)
        out += std::string("__launch graph ") + (net->use_graph ? "1" : "0") + "\n";
    if (buf && cap > out.size()) memcpy(buf, out.c_str(), out.size() + 1);
    return (long)out.size();
}

int ssd_net_tuning_stats(const ssd_net* net, int* from_table, int* timed) {
    SSD_CHECK_ARG(net != nullptr, "ssd_net_tuning_stats: net is NULL");
    if (from_table) *from_table = net->n_preset;
    if (timed) *timed = net->n_autotuned;
    return SSD_OK;
}

}  // extern "C"

namespace ssd {

// The number behind `word` on the line of `name` ("block_7_fused image 2", "__launch graph 0"); -1: the table has no such line
static int preset_number(const ssd_net& net, const std::string& name, const char* word) {
    const auto it = net.preset.find(name);
    return it != net.preset.end() && it->second.first == word ? it->second.second : -1;
}

// The shared split-K workspace holds at least `floats`
static int ensure_splitk_ws(ssd_net& net, size_t floats) {
    if (floats <= net.splitk_floats) return SSD_OK;
    if (net.splitk_ws) (void)hipFree(net.splitk_ws);
    net.splitk_ws = nullptr;
    SSD_HIP(hipMalloc((void**)&net.splitk_ws, floats * sizeof(float)));
    net.splitk_floats = floats;
    return SSD_OK;
}

// Preset lines (ssd_net_set_tuning) replace the on-device autotune LAYER BY LAYER: a layer whose line
// is missing or names a configuration that cannot run it here is timed on the device, the others are
// not -- a complete table means no timing at all and therefore the same kernels (and the same bits)
// in every process that loads it.  *image_preset_ok: every block the image kernel can run has its line.
int finalize_apply_preset(ssd_net* net, int max_batch, bool* image_preset_ok) {
    for (auto& l : net->layers) { l.cfg = -1; l.split_k = 1; }
    size_t ws_need = 0;
    int n_tuned = 0, n_preset = 0;
    for (auto& l : net->layers) {
        if (l.kind != LK_CONV) continue;
        const auto it = net->preset.find(l.name);
        int cfg = it == net->preset.end() ? -1 : conv_config_by_name(it->second.first.c_str());
        SSD_UNSUPPORTED_IF(cfg >= 0 && conv_config_is_dmah(cfg) && net->precision != 0,
                           "finalize: the table puts layer %s on %s: the two-plane fp16 tiles are admitted in fp32 nets (precision 0) only",
                           l.name.c_str(), conv_config_name(cfg));
        cfg = dmah_or_twin(*net, l, cfg);       // a "dmah_*" line where the form may not run: its "dma3_*" twin
        if (cfg < 0 || !conv_config_allowed(cfg, net->precision)) { ++n_tuned; continue; }
        l.cfg = cfg;
        l.split_k = it->second.second;
        const ConvParams p = layer_conv_params(*net, l, max_batch, net->tensors[l.in].dev,
                                               l.out >= 0 ? net->tensors[l.out].dev : nullptr, nullptr,
                                               net->arena, net->arena, conv_config_reads(cfg));
        const bool split_ok = l.split_k == 1 || conv_k_tiles(cfg, p) >= l.split_k;
        if (l.split_k < 1 || !split_ok || !conv_config_valid(cfg, p)) { l.cfg = -1; l.split_k = 1; ++n_tuned; continue; }
        ++n_preset;
        if (l.split_k > 1) ws_need = std::max(ws_need, (size_t)l.split_k * p.M * p.Cout);
    }
    *image_preset_ok = true;
    for (auto& f : net->layers) {       // whole-block layers the image kernel can run: "name image 0|1|2"
        if (f.kind != LK_FUSED || f.f_type != 0) continue;
        f.img_choice = -1;
        if (!image_kernel_takes(*net, f)) continue;
        const int choice = preset_number(*net, f.name, "image");
        if (choice < 0) { *image_preset_ok = false; continue; }
        f.img_choice = std::min(choice, 2);
        if (f.img_choice == 2 && (net->precision != 0 || !net->image_split)) f.img_choice = 1;
    }
    if (const int rc = ensure_splitk_ws(*net, ws_need)) return rc;
    net->n_autotuned = n_tuned;
    net->n_preset = n_preset;
    return SSD_OK;
}

// The per-layer race keeps the best of EACH family -- fam 0: tiles that read the fp32 activation, fam 1: LDS-DMA tiles
// over its three bf16 planes ("dma3_*" / "dmab_*"), fam 2: LDS-DMA tiles over its fp16 pair ("dmah_*", layers with fp16
// weight planes only) -- because which of them a layer takes is decided per TENSOR (decide_tensor).  ms: per kReps launches.
constexpr int kReps = 4;
struct Best {
    float ms[3] = {1e30f, 1e30f, 1e30f}; int cfg[3] = {-1, -1, -1}; int split[3] = {1, 1, 1}; bool timed = false;
};
struct Timed { int cfg; float ms; };        // (SSD_HIP_DEBUG_TUNE: every candidate that was timed, for the report)
struct ConvRace {
    ssd_net& net;
    int B; hipStream_t st;
    EventPair ev;
    ScopedDev deltas, probs;               // scratch outputs for the head convs
    bool dbg_sync;                         // SSD_HIP_DEBUG_SYNC: name the launch a GPU fault belongs to
};

// Times each valid (tile configuration, split-K factor) of conv layer l and keeps the best per family.  Split-K is tried only
// where the plain grid cannot fill the 256 CUs.  One untimed launch, then the minimum over 3 windows of kReps back-to-back
// launches (robust against clock ramps / noise); a candidate clearly slower than its family's incumbent stops after the first.
static int race_conv_layer(ConvRace& r, Layer& l, Best* best, std::vector<Timed>* seen) {
    // dense around small factors: the best split is the one whose M-blocks x split just fills a
    // whole number of CU rounds (e.g. 100 M-blocks x 5 = 500 blocks on 512 slots for head 2)
    static const int kSplits[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 32};
    const ssd_net& net = r.net;
    Best& bb = *best;
    bb.timed = true;
    const float* in = net.tensors[l.in].dev;
    float* out = l.out >= 0 ? net.tensors[l.out].dev : nullptr;
    const float* res = l.res >= 0 ? net.tensors[l.res].dev : nullptr;
    for (int c = 0; c < conv_num_configs(); ++c) {
        const int fam = conv_config_reads(c);      // the best tile is kept per storage it reads: fp32, bf16 planes, fp16 pair
        if (fam == CONV_READS_F16X2 && (!net.conv_f16x2 || !l.wh)) continue;
        for (const int split : kSplits) {
            l.split_k = split;
            // (a pair tile is timed on whatever the planes hold: the matrix unit's time does not depend on the data)
            const ConvParams p = layer_conv_params(net, l, r.B, in, out, res, r.deltas.p, r.probs.p, fam);
            if (!conv_config_valid(c, p) || !conv_config_allowed(c, net.precision)) break;
            const bool direct = conv_config_family(c) == CF_DIRECT;
            if (direct && (bb.cfg[0] >= 0 || bb.cfg[1] >= 0 || split > 1)) break;     // direct only as a last resort
            if (split > 1) {
                if (conv_grid_blocks(c, p) > 384 || conv_k_tiles(c, p) < 4 * split) break;
                if ((size_t)split * p.M * p.Cout > net.splitk_floats) break;
            }
            if (r.dbg_sync) fprintf(stderr, "[ssd dbg] tune %s %s split %d\n", l.name.c_str(), conv_config_name(c), split);
            if (const int rc = conv_launch(p, c, r.st)) return rc;     // warm-up
            if (r.dbg_sync) SSD_HIP(hipStreamSynchronize(r.st));
            float ms = 1e30f;
            for (int trial = 0; trial < 3; ++trial) {
                float t = 0.f;
                if (const int rc = r.ev.window(r.st, kReps, [&] { return conv_launch(p, c, r.st); }, &t)) return rc;
                ms = t < ms ? t : ms;
                if (trial == 0 && ms > 1.5f * bb.ms[fam]) break;      // clearly slower than its family's incumbent
            }
            if (ms < bb.ms[fam]) { bb.ms[fam] = ms; bb.cfg[fam] = c; bb.split[fam] = split; }
            if (seen) seen->push_back({c, ms});
        }
    }
    return SSD_OK;
}

// SSD_HIP_DEBUG_TUNE: a raced layer's best per family, and the fp16 pair's best with one / two k-steps per barrier
static void report_conv_race(const Layer& l, const Best& bb, const std::vector<Timed>& seen) {
    fprintf(stderr, "[ssd] tune %s: %s/s%d %.4f ms | %s/s%d %.4f ms | %s/s%d %.4f ms\n", l.name.c_str(),
            bb.cfg[0] >= 0 ? conv_config_name(bb.cfg[0]) : "-", bb.split[0], bb.cfg[0] >= 0 ? bb.ms[0] / kReps : 0.f,
            bb.cfg[1] >= 0 ? conv_config_name(bb.cfg[1]) : "-", bb.split[1], bb.cfg[1] >= 0 ? bb.ms[1] / kReps : 0.f,
            bb.cfg[2] >= 0 ? conv_config_name(bb.cfg[2]) : "-", bb.split[2], bb.cfg[2] >= 0 ? bb.ms[2] / kReps : 0.f);
    if (bb.cfg[2] < 0) return;
    float ms_k64 = 1e30f, ms_k32 = 1e30f;
    for (const Timed& t : seen) {
        if (conv_config_reads(t.cfg) != CONV_READS_F16X2) continue;
        float& m = strstr(conv_config_name(t.cfg), "_ks2") ? ms_k64 : ms_k32;
        m = t.ms < m ? t.ms : m;
    }
    fprintf(stderr, "[ssd] tune %s: dmah best with one k-step per barrier %.4f ms, with two %.4f ms\n", l.name.c_str(),
            ms_k32 / kReps, ms_k64 < 1e29f ? ms_k64 / kReps : 0.f);
}

// What `bytes` more (less) per element in the store of tensor t's producer cost at batch B, at the 3 TB/s the epilogues'
// stores reach, in the race's unit (ms per kReps launches)
static double store_cost_ms(const Tensor& t, int B, double bytes) {
    return kReps * ((double)B * t.per_image * bytes / 3.0e12 * 1e3);
}
static void take_family(Layer& l, const Best& bb, int fam) { l.cfg = bb.cfg[fam]; l.split_k = bb.split[fam]; }

// The family is a property of the TENSOR: LDS-DMA readers make its producer store the bf16 planes (2 * planes_np bytes per
// element), and when every reader takes them the producer drops the fp32 store (4 bytes per element back: plane-only,
// Tensor::plane_only).  So per tensor: the sum of its timed readers' best fp32-reading tiles against the sum of their
// best LDS-DMA tiles plus what the producer's store changes by; all timed readers flip together.  Called under the routes
// decide_storage assumes.
static void decide_tensor(ssd_net& net, int t, int B, const std::vector<Best>& bests, bool dbg_tune) {
    const Tensor& tt = net.tensors[t];
    std::vector<size_t> flip;
    bool planes_anyway = false;
    // the fp16 pair (fam 2) is open to the tensor only when every reader of its planes can take it: all the timed ones
    // have a "dmah_*" best, and no other conv layer reads the planes through another family
    bool pair_ok = net.conv_f16x2;
    double sum0 = 0, sum1 = 0, sum2 = 0;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        Layer& l = net.layers[li];
        if (l.kind != LK_CONV || l.in != t) continue;
        const Best& bb = bests[li];
        if (!bb.timed) {
            if (layer_runs(l) && conv_config_is_dma(l.cfg)) planes_anyway = true;
            if (conv_config_is_dma(l.cfg) && !conv_config_is_dmah(l.cfg)) pair_ok = false;
            continue;
        }
        if (bb.cfg[1] < 0) continue;                 // no LDS-DMA tile takes it: stays where it is
        if (bb.cfg[0] < 0) { planes_anyway = true; pair_ok = false; continue; }      // ... only LDS-DMA tiles do: already there (three planes)
        if (!layer_runs(l)) {       // fused away under these routes: reads nothing; on its own, with the full plane store charged
            if (bb.ms[1] + store_cost_ms(tt, B, 2.0 * tt.planes_np) < bb.ms[0]) { take_family(l, bb, 1); pair_ok = false; }
            continue;
        }
        flip.push_back(li);
        sum0 += bb.ms[0]; sum1 += bb.ms[1]; sum2 += bb.ms[2];
        if (bb.cfg[2] < 0) pair_ok = false;
    }
    if (flip.empty()) return;
    for (size_t li : flip) take_family(net.layers[li], bests[li], 1);
    const bool only = plan_storage(net).only[t];          // ... under the readers' LDS-DMA tiles: would the fp32 copy go?
    // what the producer's store changes by, per element: np planes of 2 bytes more, 4 bytes less where the fp32 copy goes
    auto store_ms_of = [&](int np) { return store_cost_ms(tt, B, only ? 2.0 * np - 4.0 : planes_anyway ? 0.0 : 2.0 * np); };
    const double store_ms = store_ms_of(tt.planes_np), store2_ms = store_ms_of(2);
    int take = sum1 + store_ms < sum0 ? 1 : 0;
    if (pair_ok && sum2 + store2_ms < (take ? sum1 + store_ms : sum0)) take = 2;
    for (size_t li : flip) take_family(net.layers[li], bests[li], take);
    if (dbg_tune)
        fprintf(stderr, "[ssd] tune tensor %s: fp32 readers %.4f ms, plane readers %.4f + store %+.4f ms, fp16-pair readers %.4f + store %+.4f ms%s (%s) -> %s\n",
                tt.name.c_str(), sum0 / kReps, sum1 / kReps, store_ms / kReps, sum2 / kReps, store2_ms / kReps, pair_ok ? "" : " [not open]",
                only ? "plane-only" : "both copies", take == 2 ? "fp16 pair" : take ? "planes" : "fp32");
}

// ... for every tensor.  The whole-image kernel is taken to run wherever it can (its own race comes later; it wins in
// every shipped table): what it fuses away reads no tensor.  The assumption is undone afterwards.  (Routes only: the
// stored storage state stays empty until the end of finalize; decide_tensor asks the pure plan_storage.)
static void decide_storage(ssd_net& net, int B, const std::vector<Best>& bests, bool dbg_tune) {
    std::vector<int> img_saved;
    for (auto& f : net.layers) {
        img_saved.push_back(f.img_choice);
        if (f.img_choice < 0 && image_kernel_takes(net, f)) f.img_choice = 1;
    }
    resolve_routes(net);
    for (size_t t = 1; t < net.tensors.size(); ++t) decide_tensor(net, (int)t, B, bests, dbg_tune);
    for (size_t i = 0; i < net.layers.size(); ++i) net.layers[i].img_choice = img_saved[i];
    resolve_routes(net);
}

// Conv layers without a (valid) preset line: each raced on the device, then the storage decision over the results.
int autotune(ssd_net& net, int B, hipStream_t st) {
    ConvRace race{net, B, st};
    if (const int rc = race.ev.create()) return rc;
    SSD_HIP(hipMalloc((void**)&race.deltas.p, (size_t)B * net.num_priors * 4 * sizeof(float)));
    SSD_HIP(hipMalloc((void**)&race.probs.p, (size_t)B * net.num_priors * net.L * sizeof(float)));
    race.dbg_sync = getenv("SSD_HIP_DEBUG_SYNC") != nullptr;
    const bool dbg_tune = getenv("SSD_HIP_DEBUG_TUNE") != nullptr;
    // split-K workspace: the largest [split][M][Cout] slab any candidate may need
    size_t ws_floats = 0;
    for (auto& l : net.layers) {
        if (l.kind != LK_CONV) continue;
        const size_t mc = (size_t)B * l.Ho * l.Wo * l.Cout;
        if (mc <= (size_t)4 << 20) ws_floats = std::max(ws_floats, mc * 32);
    }
    if (const int rc = ensure_splitk_ws(net, ws_floats)) return rc;
    std::vector<Best> bests(net.layers.size());
    std::vector<Timed> seen;
    for (size_t li = 0; li < net.layers.size(); ++li) {
        Layer& l = net.layers[li];
        if (l.kind != LK_CONV || l.cfg >= 0) continue;           // (cfg >= 0: chosen by a valid preset line)
        const Best& bb = bests[li];
        seen.clear();
        if (const int rc = race_conv_layer(race, l, &bests[li], dbg_tune ? &seen : nullptr)) return rc;
        SSD_UNSUPPORTED_IF(bb.cfg[0] < 0 && bb.cfg[1] < 0, "finalize: no conv kernel can run layer %s", l.name.c_str());
        take_family(l, bb, bb.cfg[0] >= 0 ? 0 : 1);          // the fp32-reading family until the tensor decision
        if (dbg_tune) report_conv_race(l, bb, seen);
    }
    decide_storage(net, B, bests, dbg_tune);
    return SSD_OK;
}

// Whole-image block kernel vs the layer kernels (expand GEMM + depthwise/project kernel) of the
// same block, timed on the device at batch B: at B = 64 the 4-way channel-group reduction costs
// what the E round trip through HBM costs, at large batches (one group) the image kernel wins.
// The race moves the routes alone (resolve_routes): storage is not resolved before the end of finalize, so no planes are
// live here and both sides are timed without their plane stores or split passes -- as they always were.
int tune_image_blocks(ssd_net& net, int B, hipStream_t st) {
    EventPair ev;
    if (const int rc = ev.create()) return rc;
    struct ModeGuard {          // the race runs in "tuned choice" mode; early error returns restore the caller's mode too
        ssd_net& n;
        int mode;
        ~ModeGuard() { n.fuse_image = mode; }
    } guard{net, net.fuse_image};
    net.fuse_image = 1;
    for (size_t fi = 0; fi < net.layers.size(); ++fi) {
        Layer& f = net.layers[fi];
        if (f.kind != LK_FUSED || f.f_type != 0) continue;
        if (!image_kernel_takes(net, f)) { f.img_choice = 0; continue; }
        if (f.img_choice >= 0) continue;        // preset line
        float ms[3] = {1e30f, 1e30f, 1e30f};
        const int nchoice = net.precision == 0 && net.image_split ? 3 : 2;     // 2: the fp32 net's split-bf16 form
        auto block = [&] {                      // the block's running layers under the current routes, once
            int rc = SSD_OK;
            for (int j = (int)fi; j <= f.f_project && !rc; ++j)
                if (layer_runs(net.layers[j])) rc = run_layer(net, net.layers[j], B, nullptr, nullptr, st);
            return rc;
        };
        for (int choice = 0; choice < nchoice; ++choice) {
            f.img_choice = choice;
            resolve_routes(net);
            if (choice == 2 && image_plan(net, f, B).form < 2) continue;     // (not raced: the plan is not the split-bf16 form or the fp16 pair it asks for)
            for (int trial = 0; trial < 4; ++trial) {        // trial 0 warms up
                float t = 0.f;
                if (const int rc = ev.window(st, 4, block, &t)) return rc;
                if (trial && t < ms[choice]) ms[choice] = t;
            }
        }
        f.img_choice = ms[2] < ms[1] && ms[2] < ms[0] ? 2 : ms[1] < ms[0] ? 1 : 0;
    }
    return SSD_OK;
}

// hipGraph replay vs direct launches of the whole forward, raced on the device at max_batch on a zero
// image (measured at B=64: direct launches 1.950 ms, replay 1.972 ms per step on a non-default stream).
// Skipped once "use_graph" was set explicitly; "__launch graph 0|1" is the recorded outcome of this race.
int tune_launch_mode(ssd_net* net, int B) {
    if (!net->use_graph_auto || net->timing) return SSD_OK;
    const int preset = preset_number(*net, "__launch", "graph");
    if (preset >= 0) {
        net->use_graph = preset != 0;
        net->launch_raced = true;
        return SSD_OK;
    }
    ++net->n_autotuned;
    const size_t n_img = (size_t)B * net->img_size * net->img_size * 3;
    ScopedDev img, del, prb;
    SSD_HIP(hipMalloc((void**)&img.p, n_img * sizeof(float)));
    SSD_HIP(hipMalloc((void**)&del.p, (size_t)B * net->num_priors * 4 * sizeof(float)));
    SSD_HIP(hipMalloc((void**)&prb.p, (size_t)B * net->num_priors * net->L * sizeof(float)));
    SSD_HIP(hipMemset(img.p, 0, n_img * sizeof(float)));
    hipStream_t st = nullptr;
    SSD_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    EventPair ev;
    int rc = ev.create();
    float ms[2] = {1e30f, 1e30f};
    auto forward = [&] { return ssd_net_forward(net, img.p, B, del.p, prb.p, st); };
    for (int mode = 0; mode < 2 && !rc; ++mode) {        // warm both modes: eager run, capture, replay
        net->use_graph = mode != 0;
        for (int w = 0; w < 3 && !rc; ++w) rc = forward();
    }
    for (int trial = 0; trial < 4 && !rc; ++trial)       // interleaved trials (clock drift cancels), best of 4 each
        for (int mode = 0; mode < 2 && !rc; ++mode) {
            net->use_graph = mode != 0;
            float t = 0.f;
            rc = ev.window(st, 6, forward, &t);
            if (!rc && t < ms[mode]) ms[mode] = t;
        }
    (void)hipStreamSynchronize(st);
    net->drop_graphs();
    (void)hipStreamDestroy(st);
    net->tensors[0].dev = nullptr;
    // the two are within ~1 % at B=64 and direct launches measured faster on real batches (heads overlap the
    // backbone earlier): replay only where it is clearly ahead (small batches, launch-bound hosts)
    net->use_graph = rc ? true : ms[1] < ms[0] * 0.99f;
    net->launch_raced = !rc;
    if (getenv("SSD_HIP_DEBUG_TUNE"))
        fprintf(stderr, "[ssd] launch mode race at B=%d: direct %.4f ms, graph replay %.4f ms per forward -> %s\n", B, ms[0] / 6,
                ms[1] / 6, net->use_graph ? "replay" : "direct");
    return rc;
}

}  // namespace ssd
