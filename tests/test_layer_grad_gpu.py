"""Every training backward kernel (csrc/ssd_train.hip) against the float64 LAYER oracle (oracle/layer_grad_oracle.py).

Part A, teacher forced over the real graphs: one device training step, then every layer's backward is recomputed in
float64 from the device's own tensors (the layer's input activation, ``pre`` / ``mean`` / ``var``, the device's gradient
of the layer's output, the weights) and compared element by element in E = |got - ref64| / (2^-24 A), A the
absolute-value sum of the element's terms; bar E <= 16 (derivation: the oracle's docstring; the CPU proof that the bar
separates right from subtly wrong: tests/test_layer_grad_cpu.py).  Compared per layer: the gradient of the input tensor
(summed over all consumers of that tensor), dW, dgamma / dbeta / dbias, the batch statistics and the new moving averages.
Max-pool: input cells that tie for a window's maximum (after ReLU: all-zero windows) are left out of the elementwise
comparison -- which of them receives the gradient is a convention -- and the gradient's mass per image and channel is
checked instead (pool4's input conv4_3 has a second consumer, the L2 normalisation: no mass check there).

Part B, the kernels outside a net (ssd_conv2d_wgrad_ex, ssd_dwconv3x3_backward): EVERY weight-gradient tile shape of the
table -- the training step times them on the device and keeps the fastest, so which one a whole-net test reaches is up
to timing noise -- and the depthwise backward, at edge shapes, against the same oracle and bar.

The bf16 mode's dense-conv data gradients: test_mobilenet_v2_dense_data_gradients_bf16 states the rounding rule and which
layers it can be held to bit for bit (the extras and the heads; not the BatchNorm convs).

Worst E measured on an MI355X (bar 16), MobileNetV2 B = 2 / VGG16 B = 1, with the layer it occurred at:
  gradient of a layer's input   1x1 conv + BN 5.1 (block_1_expand), + residual 2.0, bias + ReLU 6.9 (extra1_1) / 10.1 (conv9_1);
                                3x3 s1 bias + ReLU 10.8 (conv3_3), dilation 6 5.7 (conv6), 3x3 s2 6.0 (extra1_2) / 4.3 (conv8_2);
                                depthwise s1 3.7 (expanded_conv_depthwise), s2 7.1 (block_13_depthwise);
                                heads 14.7 (VGG16 level 1, K = 900); pool 2/2 4.2 (pool4 + L2 norm), pool 3/1 3.1
  dW                            1x1 2.9 / 7.8 (conv7), 3x3 s1 8.9 (conv4_1), dilation 6 8.6, 3x3 s2 5.7, im2col stem 0.15 (Conv1),
                                depthwise 0.9, head label 7.2 / box 5.2
  dgamma / dbeta / dbias        2.0 / 2.0 / 2.7; L2-norm scale 3.0
  batch mean / variance         3.3 / 13.2 (Conv_1; the kernel's one-pass shifted sums against the two-pass A: a small margin)
  bf16 data gradients           3.4 (extras and heads, 10 tensors)
Where the figures above ~4 come from (the step's tile log, SSD_HIP_TRAIN_AUTOTUNE=2): the largest two, heads 14.7 and
conv3_3 10.8, ran on split-bf16 "mfma3_*" tiles (K = 1152 / 2304); MobileNetV2, on fp32 "mfma_*" tiles but for one
conv, tops out at 7.1; the fp32-MFMA weight gradients reach 8.9; every VALU kernel (depthwise, reductions, pools, L2
norm) stays at the CPU floor of <= 4.  The excess belongs to matrix-core accumulation and grows with its length: an
error with a sign bias (the split's dropped cross terms and truncated low plane; the MFMA's own accumulate rounding was
not isolated), not a random walk.  The conv tile is chosen by timing, so the head figure's margin to the bar is real.
  max-pool mass                 0.25; cells left out as ties: 35.3 % (VGG16)
  ssd_conv2d_wgrad_ex           4.3 over 10 shapes x 13 configs;  ssd_dwconv3x3_backward  dx 3.8, dw 2.6"""
import ctypes

import numpy as np
import pytest
import torch

import helpers
from oracle import layer_grad_oracle as lg

pytestmark = pytest.mark.gpu


def _targets(hp, B, seed=3):
    from oracle import bbox_oracle as bo
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=hp["total_labels"], seed=seed)
    return bo.calculate_actual_outputs(priors, gt, gl, hp)


def _step_and_check(backbone, B, seed, precision="fp32", **check):
    """One device training step on synthetic weights, then the whole graph through the layer oracle."""
    from models._net import SSDModel
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = helpers.hyper_params(backbone)
    w = {k: v.copy() for k, v in helpers.synthetic_weights(backbone, hp).items()}
    x = helpers.images(B, 300, seed=seed)
    yd, yl = _targets(hp, B)
    m = SSDModel(backbone, hp, precision=precision)
    m.set_weights(w)
    m.compile()
    _, _, g = m.forward_backward(x, yd, yl)
    g = g.cpu().numpy().copy()
    assert np.isfinite(g).all()
    after = m.get_weights()
    grads = {name: g[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in m.trainable_offsets().items()}
    specs = lg.layers(backbone, hp)
    shapes = lg.tensor_shapes(specs, w)
    N, L = yl.shape[1], hp["total_labels"]
    cache = {}

    def fetch(name):
        if name not in cache:
            if name == "input":
                cache[name] = x
            elif name in ("grad_logits", "grad_deltas"):
                cache[name] = m.train_fetch(name, B).reshape(B, N, L if name == "grad_logits" else 4)
            elif name.startswith(("mean:", "var:")):
                cache[name] = m.train_fetch(name, B)
            else:
                key = name[5:] if name.startswith("grad:") else name
                cache[name] = m.train_fetch(name, B).reshape((B,) + shapes[key])
        return cache[name]
    report = lg.Report()
    info = lg.check_graph(specs, fetch, w, grads, hp, B, report, moving_after=after, moving_before=w, **check)
    for line in report.lines():
        print(line)
    print("%s: %d layers, %d tensors compared, max-pool cells left out as ties: %.2f %%" % (
        backbone, info["layers"], report.compared, 100.0 * info["pool_excluded"]))
    return report, info


def test_mobilenet_v2_every_layer_backward_fp32():
    """MobileNetV2-SSD300, B = 2 (the smallest batch with non-degenerate batch statistics): the maps 150 .. 1 cover odd
    and even widths of the four-column depthwise data gradient, the correct_pad stride-2 depthwise layers, the Cin = 3
    im2col stem, the 16- / 24-channel sides and the padded head dY."""
    report, info = _step_and_check("mobilenet_v2", 2, seed=41)
    # 66 layers; per BatchNorm layer (52): mean, var, dW, dgamma, dbeta; per bias layer (8): dW, dbias; per head (6): 2 dW +
    # 2 dbias; 60 activation gradients (every tensor but the image)
    assert info["layers"] == 66 and report.compared == 52 * 5 + 8 * 2 + 6 * 4 + 60
    assert not report.fails, "\n".join(report.fails[:20])


def test_vgg16_every_layer_backward_fp32():
    """VGG16-SSD300, B = 1 (no BatchNorm): dilation 6, VALID and stride-2 SAME convs, pool 2/2 and the overlapping 3/1
    pool, L2 normalisation with its scale gradient, the 1e-3 w regulariser term in dW."""
    report, info = _step_and_check("vgg16", 1, seed=43)
    # 35 layers: 23 convs (dW, dbias), 6 heads (2 dW + 2 dbias), the L2-norm scale, 4 max-pool mass checks, 29 activation
    # gradients (23 conv outputs, 5 pools, the normalised map)
    assert info["layers"] == 35 and report.compared == 23 * 2 + 6 * 4 + 1 + 4 + 29
    assert 0.0 < info["pool_excluded"] < 0.9
    assert not report.fails, "\n".join(report.fails[:20])


BF16_LAYERS = (["extra%d_%d" % (i, j) for i in range(1, 5) for j in (1, 2)] + ["%d_conv_heads" % i for i in range(1, 7)] +
               ["block_13_depthwise"])


def test_mobilenet_v2_dense_data_gradients_bf16():
    """precision="bf16", B = 2.  The rule, from the code (launch_conv in csrc/ssd_train.hip): the data gradient of a dense
    conv is a forward conv of dY (fp32 in memory) with the rotated weights.  In the bf16 mode it runs on a "bf16_*" tile --
    both operands rounded ONCE to bf16, nearest with ties to even (rne2, csrc/ssd_bf16x3.h: the weights when they are
    re-packed, dY when the tile stages it), products and sums fp32 -- unless an fp32 "mfma_*" tile timed faster for the
    shape on this device (the race admits them; measured: the 1x1 extras with K = 128), and then NO operand is rounded.
    Which of the two ran is not observable, so the oracle computes both (operands rounded as above, or not, products
    and sums in float64) and a tensor's gradient must meet E <= 16 for one combination of its consumers' forms; a wrong
    term in either tile family matches neither.  That needs dY bit for bit: for the 8 bias + ReLU extra convs it is
    grad:<out> times the ReLU mask, for the 6 head pairs the fetched loss gradients -- both exact in fp32.  For a
    BatchNorm conv dY is the fp32 result of bn_bwd_apply_kernel in a scratch buffer the fetch hook does not expose; one
    element rounded differently there moves a bf16 rounding by 2^-9 of a term = 2^15 u, so those layers cannot be held to
    this bar from outside and stay with the fp32 test.  Compared: the gradient of every tensor all of whose dense-conv
    consumers are extras or heads -- out_relu, extra1_1 .. extra4_2 and block_13_expand_relu (head 1 plus the fp32
    depthwise backward of block 13): 10 tensors, 15 layers."""
    report, info = _step_and_check("mobilenet_v2", 2, seed=41, precision="bf16", only=set(BF16_LAYERS), params=False,
                                   round_dx=lg.bf16_rne)
    assert info["layers"] == 15 and report.compared == 10
    assert not report.fails, "\n".join(report.fails[:20])


# ---------------------------------------------------------------------------------------------- Part B
def _dev(a):
    import ssd_hip as h
    return h.to_dev(np.ascontiguousarray(a, dtype=np.float32))


def _nan(n):
    import ssd_hip as h
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device=h.device())


#              Cin Cout k  s  dil  H   W  B  pads (pt, pb, pl, pr) or None = TF SAME     ldg  column offset
WGRAD_CASES = [(3, 32, 3, 2, 1, 31, 33, 2, (1, 1, 0, 1), None, 0),        # im2col path, pads (1,1) and (0,1)
               (16, 96, 1, 1, 1, 19, 19, 2, None, None, 0),               # small channel side
               (96, 24, 1, 1, 1, 10, 10, 2, None, None, 0),               # N below every tile
               (68, 20, 3, 1, 1, 5, 5, 1, None, None, 0),                 # Cin, N off every tile multiple; M = 25 < one slab
               (64, 84, 3, 1, 1, 3, 3, 2, None, None, 0),                 # N = 84
               (64, 84, 3, 1, 1, 3, 3, 2, None, 88, 84),                  # ... inside a padded buffer, 84 columns in
               (64, 24, 3, 1, 1, 3, 3, 2, None, 150, 126),                # a real head pair's box half: unaligned g, scalar staging
               (32, 64, 3, 1, 6, 19, 19, 1, None, None, 0),               # dilation 6, SAME
               (128, 256, 3, 2, 1, 10, 10, 2, None, None, 0),             # stride 2, SAME
               (256, 128, 1, 1, 1, 1, 1, 2, None, None, 0),               # M = 2
               (64, 64, 3, 1, 1, 38, 38, 3, None, None, 0)]               # more than one M chunk


@pytest.mark.parametrize("case", WGRAD_CASES, ids=["%dx%d_k%d_s%d_d%d_%dx%d_b%d%s" % (c[:8] + ("_ld%d" % c[9] if c[9] else "",))
                                                   for c in WGRAD_CASES])
def test_weight_gradient_every_tile_shape(case):
    import ssd_hip as h
    from oracle import net_oracle as no
    lib = h.lib()
    Cin, N, k, s, dil, H, W, B, pads, ldg, off = case
    if pads is None:
        (_, pt, pb), (_, pl, pr) = no.same_pads(H, k, s, dil), no.same_pads(W, k, s, dil)
    else:
        pt, pb, pl, pr = pads
    d = h.ConvDesc(B, H, W, Cin, N, k, k, s, dil, pt, pl, pb, pr, 0, 0)
    Ho, Wo = lib.ssd_conv_out_size(H, k, s, dil, pt, pb), lib.ssd_conv_out_size(W, k, s, dil, pl, pr)
    M = B * Ho * Wo
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    ldg = ldg or N
    buf = rng.standard_normal(off + M * ldg).astype(np.float32)          # the columns beside g hold data too, not zeros
    g = buf[off:].reshape(M, ldg)[:, :N].reshape(B, Ho, Wo, N)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    wz = torch.zeros((k, k, Cin, N), dtype=torch.float64)
    _, ref = lg.conv_backward(t64(x), wz, t64(g), s, dil, (pt, pb, pl, pr), need_dx=False)
    _, A = lg.conv_backward(t64(x).abs(), wz, t64(g).abs(), s, dil, (pt, pb, pl, pr), need_dx=False)
    xd, bd = _dev(x), _dev(buf)
    need = lib.ssd_conv_wgrad_workspace_floats(ctypes.byref(d), N)
    assert need >= k * k * Cin * N
    if (Cin, H, B) == (64, 38, 3):
        assert need > k * k * Cin * N, "this shape is here for its M chunks"
    n_cfg = lib.ssd_conv_wgrad_num_configs()
    assert n_cfg == 12
    worst, fails, ran = 0.0, [], 0
    for cfg in range(-1, n_cfg):
        dW, ws = _nan(k * k * Cin * N), _nan(need)          # fresh poison per config: stale partial sums would look plausible
        h.check(lib.ssd_conv2d_wgrad_ex(ctypes.byref(d), h.ptr(xd), h.vp(bd.data_ptr() + 4 * off), ldg, N, cfg, h.ptr(dW),
                                        h.ptr(ws), need, h.stream()), "ssd_conv2d_wgrad_ex")
        E, i = lg.e_metric(dW.cpu().numpy(), ref, A)
        ran += 1
        worst = max(worst, E)
        if not E <= lg.E_BAR:
            fails.append("config %d: E = %.3g at flat index %d" % (cfg, E, i))
    print("wgrad %s: worst E over %d configs %.2f" % (case, ran, worst))
    assert ran == 13 and not fails, "\n".join(fails)


#           C    H   W  stride pad_t pad_l B
DW_CASES = [(32, 7, 5, 1, 1, 1, 2),
            (96, 19, 19, 1, 1, 1, 2),
            (144, 10, 9, 1, 1, 1, 1),
            (192, 38, 38, 2, 0, 0, 1),          # correct_pad of an even map: (0, 1)
            (576, 19, 19, 2, 1, 1, 2),          # ... of an odd map: (1, 1)
            (68, 4, 3, 1, 1, 1, 1),
            (960, 1, 1, 1, 1, 1, 2)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", DW_CASES, ids=["c%d_%dx%d_s%d_p%d%d_b%d" % c for c in DW_CASES])
def test_depthwise_backward_edge_shapes(case, accumulate):
    import ssd_hip as h
    lib = h.lib()
    C, H, W, s, pt, pl, B = case
    Ho, Wo = (H + pt + 1 - 3) // s + 1, (W + pl + 1 - 3) // s + 1
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    g = rng.standard_normal((B, Ho, Wo, C)).astype(np.float32)
    w = rng.standard_normal((3, 3, C, 1)).astype(np.float32)
    dx0 = rng.standard_normal((B, H, W, C)).astype(np.float32)
    t64 = lambda a: torch.from_numpy(a).to(torch.float64)
    ref_dx, ref_dw = lg.depthwise_backward(t64(x), t64(w), t64(g), s, (pt, 1, pl, 1))
    A_dx, A_dw = lg.depthwise_backward(t64(x).abs(), t64(w).abs(), t64(g).abs(), s, (pt, 1, pl, 1))
    if accumulate:
        ref_dx, A_dx = ref_dx + t64(dx0), A_dx + t64(dx0).abs()
    dx = _dev(dx0) if accumulate else _nan(dx0.size)
    dw = _nan(9 * C)
    need = 9 * C * ((B * Ho * Wo + 63) // 64)
    ws = _nan(need)
    xd, gd, wd = _dev(x), _dev(g), _dev(w)
    h.check(lib.ssd_dwconv3x3_backward(h.ptr(xd), h.ptr(gd), h.ptr(wd), B, H, W, C, s, pt, pl, accumulate,
                                       h.ptr(dx), h.ptr(dw), h.ptr(ws), need, h.stream()), "ssd_dwconv3x3_backward")
    E_dx, i = lg.e_metric(dx.cpu().numpy(), ref_dx, A_dx)
    E_dw, j = lg.e_metric(dw.cpu().numpy(), ref_dw, A_dw)
    print("depthwise backward %s accumulate %d: E dx %.2f, dw %.2f" % (case, accumulate, E_dx, E_dw))
    assert E_dx <= lg.E_BAR, "dx: E = %.3g at flat index %d" % (E_dx, i)
    assert E_dw <= lg.E_BAR, "dw: E = %.3g at flat index %d" % (E_dw, j)
