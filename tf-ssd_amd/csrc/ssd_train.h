// Shared by the training step (ssd_train.hip) and the optimizer (ssd_optim.hip): the state behind ssd_net::train and the
// few functions one of the two units calls in the other.
#pragma once
#include <vector>

#include "ssd_net.h"

struct TrainLayer {
    float* pre = nullptr;        // BN layers: conv / depthwise output before BatchNorm [M][C]
    float* mean = nullptr;       // [C] batch statistics of the last forward
    float* var = nullptr;
    float* istd = nullptr;
    float *fscale = nullptr, *fshift = nullptr;   // BN layers: the BatchNorm folded on its moving statistics (used while it is frozen)
    float* wfwd = nullptr;       // packed forward weights (dense convs)
    float* wbwd = nullptr;       // packed backward-data weights (rotated + transposed), nullptr: no dgrad
    int cpad = 0;                // dY channel count the backward-data conv sees (heads: padded to 32)
    long g_kernel = -1, g_bias = -1, g_gamma = -1, g_beta = -1, g_kernel2 = -1, g_bias2 = -1;
    bool active = false;
};

struct ssd_train_state {
    int batch = 0;
    size_t P = 0;
    int precision = 0;                  // the net's precision the weight re-pack jobs were planned for
    double step_flops[3] = {0, 0, 0};   // matrix-core FLOPs of the last forward_backward: fp32-MFMA convs, split-bf16 convs, weight gradients
    float *flat = nullptr, *m = nullptr, *v = nullptr;
    std::vector<long> poff;             // parameter -> offset in the flat trainable vector (-1: not trainable)
    std::vector<float*> act;            // training activations per tensor (own arena: no finalize needed)
    std::vector<float*> gact;           // gradient w.r.t. each activation tensor
    std::vector<char> gwritten;
    std::vector<TrainLayer> tl;
    std::vector<float*> owned;
    float *scratch_dz = nullptr, *partial = nullptr;
    // weight gradients on a side stream beside the rest of the backward (dX chain, BatchNorm backward of the layers below):
    // dY alternates between two buffers (a buffer is rewritten only after the weight gradient that reads it is done), the
    // weight-gradient partial slab is its own
    float* dy_buf[2] = {nullptr, nullptr};
    float* partial_w = nullptr;
    size_t partial_w_floats = 0;
    hipStream_t wstream = nullptr;
    hipEvent_t ev_dy = nullptr, ev_wdone[2] = {nullptr, nullptr}, ev_wall = nullptr, ev_main_pos = nullptr;
    bool wpending[2] = {false, false};
    float* pack_jobs = nullptr;  // device array of PackJob (one launch re-packs every conv weight)
    int n_pack_jobs = 0;
    size_t partial_floats = 0;
    float *dgamma_tmp = nullptr, *dbeta_tmp = nullptr;
    float *deltas = nullptr, *probs = nullptr, *gdeltas = nullptr, *glogits = nullptr;
    void* loss_ws = nullptr;
    size_t loss_ws_bytes = 0;
    long step = 0;
    // gradient buckets for the data-parallel exchange (ssd_net_train_set_buckets): bucket k = flat offsets
    // [bucket_lo[k], bucket_lo[k + 1]) and is FINAL once the backward has passed every layer that owns a
    // parameter at or above bucket_lo[k]; bucket_ev[k] is recorded on the backward's stream right there
    std::vector<long> bucket_lo;
    std::vector<hipEvent_t> bucket_ev;
    std::vector<long> pending_hi;       // per layer i: end of the highest parameter of any ACTIVE layer j < i (0: none)
    // fine-tuning (ssd_net_set_trainable): the backward plan of the net's current flags, one SSD_PLAN_* word per layer, made
    // by refresh_plan when plan_rev lags behind ssd_net::trainable_rev
    unsigned plan_rev = ~0u;
    std::vector<int> plan;
    bool any_frozen = false;
    float* fold_jobs = nullptr;         // device array of FoldJob, room for every BatchNorm layer; the first n_fold_jobs are the frozen ones
    int n_fold_jobs = 0, fold_jobs_cap = 0, fold_maxC = 0;
    // the optimizer (ssd_optim.hip): the table of the trainable ranges, one run of segments per Keras variable (a frozen
    // variable has none), room for opt_segs_cap segments and n_opt_vars variables, and the norm pass's scratch: a sum of
    // squares per segment, a clip scale per variable
    float *opt_segs = nullptr, *opt_vars = nullptr, *opt_partial = nullptr, *opt_norm = nullptr;
    int n_opt_segs = 0, opt_segs_cap = 0, n_opt_vars = 0;
    int opt_kind = -1;                  // SSD_OPT_* of the steps that wrote m / v (-1: none since the last reset)
};

namespace ssd {

// ssd_train.hip
int talloc(ssd_train_state& s, size_t floats, float** out);      // a device buffer the state owns
bool param_frozen(const ssd_net* net, int p);
int refresh_plan(const ssd_net* net, ssd_train_state& s);
// ssd_optim.hip: the table's buffers (ssd_net_train_begin), and the table of the net's current trainable flags
// (refresh_plan, after it has waited for the device)
int opt_alloc_tables(const ssd_net* net, ssd_train_state& s);
int opt_refresh_tables(const ssd_net* net, ssd_train_state& s);

}  // namespace ssd
