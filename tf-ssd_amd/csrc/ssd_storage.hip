// Activation storage: for every activation, does it exist as planes, in which form (three bf16 planes, one, the fp16 pair), does
// the fp32 copy exist, and which launch writes the planes.  One rule (plane_writer), one pure resolver (plan_storage) and
// resolve_storage, the only writer of Tensor::planes_live, Tensor::plane_only and Layer::w_out / w_e_out; the graph runner
// (ssd_net.hip) and the kernel selection (ssd_tune.hip) read the decision.  Also the planes' allocation, form and release at
// finalize, and the fetches that join them back.  No kernel: the split and join launches are ssd_convdma.hip's.
#include "ssd_net.h"

using namespace ssd;

namespace ssd {

// Who writes the planes of an output (`out`; for LK_FUSED also `e_out`, by the same kernel) of running layer l, given that
// they are live, when l runs conv config `cfg` (Layer::cfg, or run_layer's override).  The only place that knows: a
// producer that learns to store planes from registers is one line here.
PlaneWriter plane_writer(const ssd_net& net, const Layer& l, int cfg, PlaneOutput) {
    switch (l.kind) {
        case LK_CONV: {
            // the shared epilogue stores 4 channels of a dense output at a time (a tensor with planes has C % 32 == 0)
            if (l.head_kind != 0 || (l.Cout & 3) != 0) return PW_PASS;
            // A family with the CONV_WRITES_PLANES trait does.  The direct family has no trait to go by: it is one config over
            // two kernels, the RGB stem form stores the planes in-kernel, the generic VALU form does not, and which one a
            // launch takes follows from its shape -- so ask with the layer's parameters (none of them storage state).
            const float* res = l.res >= 0 ? net.tensors[l.res].dev : nullptr;
            const ConvParams p = layer_conv_params(net, l, 1, net.tensors[l.in].dev, net.tensors[l.out].dev, res, nullptr, nullptr);
            return conv_config_writes_planes(cfg, p) ? PW_KERNEL : PW_PASS;
        }
        case LK_POOL:
        case LK_L2NORM: return PW_KERNEL;
        case LK_DW: return PW_PASS;
        // the whole-image kernel stores both outputs from registers unless it combines its slabs inside the launch (option
        // image_ticket); the stem, dwproj, tile and band kernels never do
        case LK_FUSED: return route_is_image(l.route) && !net.image_ticket ? PW_KERNEL : PW_PASS;
        case LK_SOFTMAX: break;
    }
    return PW_NONE;
}
// ... and may the output then live as planes ALONE?  Whatever a kernel stores from registers -- except the direct family:
// its stem form stores the planes beside an fp32 output it always writes, so it never makes a tensor plane-only.
static bool writer_needs_no_fp32(const Layer& l, int cfg, PlaneWriter w) {
    return w == PW_KERNEL && !(l.kind == LK_CONV && conv_config_family(cfg) == CF_DIRECT);
}

// live: the inputs of the running dense convs whose chosen configuration is an LDS-DMA tile.  plane-only: live, option
// "plane_only" 1 without "image_ticket", EVERY running layer that reads the tensor (input or residual; a fused kernel reads
// fp32) such a conv, and its running producer a kernel that stores the planes from registers -- not a split pass over the
// fp32 copy.  The image (tensor 0) and the head outputs are not tensors of the arena: no network output ever qualifies.
StoragePlan plan_storage(const ssd_net& net) {
    const int nt = (int)net.tensors.size(), nl = (int)net.layers.size();
    StoragePlan s{std::vector<char>(nt, 0), std::vector<char>(nt, 0), std::vector<PlaneWriter>(nl, PW_NONE), std::vector<PlaneWriter>(nl, PW_NONE)};
    auto reads_planes = [&](const Layer& l) {
        return l.kind == LK_CONV && l.in >= 0 && conv_config_is_dma(l.cfg) && net.tensors[l.in].planes && layer_runs(l);
    };
    for (const Layer& l : net.layers)
        if (reads_planes(l)) s.live[l.in] = 1;
    if (net.plane_only && !net.image_ticket) s.only.assign(s.live.begin(), s.live.end());
    auto bar = [&](int t) { if (t >= 0) s.only[t] = 0; };
    for (int i = 0; i < nl; ++i) {
        const Layer& l = net.layers[i];
        if (!layer_runs(l)) continue;
        if (!reads_planes(l)) bar(l.in);
        bar(l.res);
        if (l.kind == LK_FUSED && l.f_project >= 0) bar(net.layers[l.f_project].res);      // (the block's residual source)
        const int outs[2] = {l.out, l.kind == LK_FUSED ? l.e_out : -1};
        for (int k = 0; k < 2; ++k) {
            if (outs[k] < 0 || !s.live[outs[k]]) continue;
            const PlaneWriter w = (k ? s.w_e_out : s.w_out)[i] = plane_writer(net, l, l.cfg, k ? PO_E_OUT : PO_OUT);
            if (!writer_needs_no_fp32(l, l.cfg, w)) bar(outs[k]);
        }
    }
    return s;
}

void resolve_storage(ssd_net& net) {
    const StoragePlan s = plan_storage(net);
    for (size_t t = 0; t < net.tensors.size(); ++t) { net.tensors[t].planes_live = s.live[t]; net.tensors[t].plane_only = s.only[t]; }
    for (size_t i = 0; i < net.layers.size(); ++i) { net.layers[i].w_out = s.w_out[i]; net.layers[i].w_e_out = s.w_e_out[i]; }
}

// fp32 activation -> its planes (producers whose writer is PW_PASS)
int planes_pass(ssd_net& net, int tensor, int B, hipStream_t st) {
    Tensor& t = net.tensors[tensor];
    return launch_split_planes(t.dev, (long)B * (long)t.per_image, t.C, t.planes_np, t.planes, t.plane_stride, st);
}

// May tensor t live as the two-plane fp16 split (Tensor::planes_np 2, ssd_bf16x3.h)?  Its values must lie in [0, 6] by
// construction: an fp32 net, and EVERY layer that can write it -- whatever the routes -- ends with ReLU6 over the whole
// tensor: a conv with SSD_ACT_RELU6 and no residual, or a whole-block layer's expanded map (the expand conv's output).
// In MobileNetV2-SSD: block 13's expanded map and Conv_1's output; nothing in VGG16 (ReLU / linear tensors).
bool tensor_relu6_bounded(const ssd_net& net, int t) {
    if (net.precision != 0 || t < 1) return false;
    bool any = false;
    for (const Layer& l : net.layers) {
        if (l.kind == LK_FUSED && l.e_out == t) {
            const Layer& le = net.layers[l.f_expand];
            if (le.act != SSD_ACT_RELU6 || le.res >= 0) return false;
            any = true;
            continue;
        }
        if (l.out != t) continue;
        if (l.kind != LK_CONV || l.act != SSD_ACT_RELU6 || l.res >= 0 || l.head_kind != 0) return false;
        any = true;
    }
    return any;
}

// A "dmah_*" config where the fp16 pair may not run -- option conv_f16x2 0, a layer without fp16 weight planes (its input is
// not ReLU6-bounded, or a weight is not finite), or `pair` false: another reader of the same planes is not on the pair --
// runs its "dma3_*" twin: the same tile, the same split-K.  Any other config is itself.
int dmah_or_twin(const ssd_net& net, const Layer& l, int cfg, bool pair) {
    return conv_config_is_dmah(cfg) && (!net.conv_f16x2 || !l.wh || !pair) ? conv_dmah_twin(cfg) : cfg;
}

// ---- finalize steps, in the order ssd_net_finalize takes them
// bf16 planes of every activation a dense conv with Cin % 32 == 0 reads (the LDS-DMA tiles' operand, ssd_convdma.hip),
// allocated for the race.  Storage is resolved before any exists: nothing is live until the end of finalize.
int finalize_planes(ssd_net* net, int max_batch, hipStream_t st) {
    for (auto& t : net->tensors) { t.planes = nullptr; t.planes_np = t.planes_cap = 0; t.plane_stride = 0; }
    resolve_storage(*net);
    for (const auto& l : net->layers) {
        if (!net->conv_dma || l.kind != LK_CONV || l.in < 0 || l.Cin % 32 != 0) continue;
        Tensor& t = net->tensors[l.in];
        if (t.planes) continue;
        t.planes_np = t.planes_cap = net->precision ? 1 : 3;
        t.plane_stride = (long)align_up(t.per_image * max_batch, 64);
        float* pl = nullptr;
        const int rcp = dev_alloc(*net, (size_t)t.planes_np * t.plane_stride / 2 + 64, &pl);
        if (rcp) return rcp;
        t.planes = reinterpret_cast<short*>(pl);
        SSD_HIP(hipMemsetAsync(pl, 0, ((size_t)t.planes_np * t.plane_stride / 2 + 64) * sizeof(float), st));
    }
    return SSD_OK;
}

// The two-plane fp16 form is a property of the TENSOR too: its planes are written once, in one form.  A tensor takes
// planes_np 2 iff EVERY conv layer reading its planes (running or fused away: the routes may change without a finalize)
// chose a "dmah_*" tile it may run (dmah_or_twin).  Otherwise the tensor keeps the exact three-way split and its "dmah_*"
// readers run their twins.  fp16 weight planes no chosen tile reads are freed.
void finalize_resolve_f16x2(ssd_net* net) {
    const int nt = (int)net->tensors.size();
    std::vector<char> any(nt, 0), all(nt, 1);
    for (const auto& l : net->layers) {
        if (l.kind != LK_CONV || l.in < 0 || !conv_config_is_dma(l.cfg)) continue;
        any[l.in] = 1;
        if (!conv_config_is_dmah(dmah_or_twin(*net, l, l.cfg))) all[l.in] = 0;
    }
    net->wplane_bytes = 0;
    for (auto& l : net->layers) {
        if (l.kind != LK_CONV) continue;
        if (conv_config_is_dmah(l.cfg)) l.cfg = dmah_or_twin(*net, l, l.cfg, any[l.in] && all[l.in]);
        if (conv_config_is_dmah(l.cfg)) {
            net->tensors[l.in].planes_np = 2;
            net->wplane_bytes += (conv_f16x2_plane_shorts(l.kh * l.kw * l.Cin, l.Cout) + 1) / 2 * sizeof(float);
        } else if (l.wh) {
            dev_free(*net, l.wh);
            l.wh = nullptr;
        }
    }
}

// The planes were allocated for the race; keep them only where a CHOSEN tile reads them (6 bytes per element in fp32 nets,
// 2 in the bf16 mode: a table without LDS-DMA tiles leaves none).  A plane-only tensor keeps its fp32 arena slot too -- the
// layout of the arena does not depend on the routing state, and option "plane_only" 0 writes it again -- so the planes
// always come on top of the slot in ssd_net_memory_bytes.
int finalize_free_unread_planes(ssd_net* net, hipStream_t st) {
    std::vector<char> read(net->tensors.size(), 0);
    for (const auto& l : net->layers)
        if (l.kind == LK_CONV && l.in >= 0 && conv_config_is_dma(l.cfg)) read[l.in] = 1;
    SSD_HIP(hipStreamSynchronize(st));
    net->plane_bytes = net->wplane_bytes;
    for (size_t i = 0; i < net->tensors.size(); ++i) {
        Tensor& t = net->tensors[i];
        if (!t.planes) continue;
        const size_t bytes = ((size_t)t.planes_cap * t.plane_stride / 2 + 64) * sizeof(float);
        if (read[i]) { net->plane_bytes += bytes; continue; }
        dev_free(*net, reinterpret_cast<float*>(t.planes));
        t.planes = nullptr; t.planes_np = t.planes_cap = 0; t.plane_stride = 0;
    }
    return SSD_OK;
}

// The values of a named tensor in the last forward, copied to the host (host_out NULL: their count).  want_planes: its planes
// joined back to fp32, 0 when no running consumer asks for them in the net's current state; *planes_out = 3 (exact split:
// h + m + l is exact), 2 (the fp16 pair of a ReLU6-bounded tensor: the value the conv tiles read, within 2^-22 |x| + 2^-33
// of what an fp32 store would have held, ssd_bf16x3.h) or 1 (bf16 rounding).  Otherwise the activation: the fp32 slot --
// or, for a plane-only tensor, whose slot is not written, the joined planes again.
long fetch_tensor(ssd_net* net, const char* who, const char* layer, float* host_out, size_t cap, bool want_planes, int* planes_out) {
    if (!net || !layer) return SSD_E_INVALID;
    auto it = net->tensor_index.find(layer);
    if (it == net->tensor_index.end()) {
        set_error("%s: unknown tensor '%s'", who, layer);
        return SSD_E_INVALID;
    }
    const Tensor& t = net->tensors[it->second];
    if (planes_out) *planes_out = t.planes_np;
    if (want_planes && (!t.planes || !t.planes_live)) return 0;
    const size_t n = t.per_image * (size_t)net->last_batch;
    if (!host_out) return (long)n;
    if (cap < n) {
        set_error("%s: buffer holds %zu floats, need %zu", who, cap, n);
        return SSD_E_INVALID;
    }
    ScopedDev joined;
    const float* src = t.dev;
    if ((want_planes || t.plane_only) && n) {
        SSD_HIP(hipMalloc((void**)&joined.p, n * sizeof(float)));
        SSD_HIP(hipDeviceSynchronize());
        const int rc = launch_join_planes(t.planes, (long)n, t.C, t.planes_np, t.plane_stride, joined.p, nullptr);
        if (rc) return rc;
        src = joined.p;
    }
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_out, src, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("%s: copy failed", who);
        return SSD_E_HIP;
    }
    return (long)n;
}

}  // namespace ssd

extern "C" long ssd_net_fetch_planes(ssd_net* net, const char* layer, float* host_out, size_t cap, int* planes_out) {
    return fetch_tensor(net, "ssd_net_fetch_planes", layer, host_out, cap, true, planes_out);
}
