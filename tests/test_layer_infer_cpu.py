"""The bars of tests/test_layer_infer_gpu.py (the INFERENCE layer path held to the float64 layer oracle) proven from
reference formulas alone, at the K and channel counts of the real layers: no GPU.

tests/test_layer_forward_cpu.py does the same for tiny layers (K <= 288); the inference graphs reach K = 9216 (VGG16 head 2),
where the max-norm statistic loses its margin: both operands rounded to 16 significand bits -- a three-way bf16 split that
lost its third plane -- score max E = 15.7 there on random data, under E_BAR = 16.  The RMS of E keeps the margin, so the
GPU test holds a dense conv to BOTH

    max E <= E_BAR = 16     and     rms E <= RMS_BAR x rms(r32),      RMS_BAR <= RMS_CAP = rms(r16) / (4 rms(r32)),

RMS_BAR per kernel family, measured on the device (tests/test_layer_infer_gpu.py: 2 ... 9), and RMS_CAP evaluated on every
layer's own reference there,

r32 the plain fp32 restatement and r16 the float64 forward with both operands rounded to nearest to 16 bits, each on the
layer's own input (oracle/layer_grad_oracle.py: forward_yardstick).  Here, on small maps (the cost goes with the map, the
error with K):

* the floor: the fp32 restatement's max E <= 4 on every shape;
* the cap: RMS_CAP >= 5 (the block oracle's FP32_BAR) on every shape and every output (out; deltas and probs of a head);
* eight kinds of subtly wrong inference forwards, built from the reference alone, each FAIL the combined bar with
  RMS_BAR = 9, the largest bar of the GPU file (and so with 5, what the cap is sized for): (a) both operands cut to 16 bits, truncated and rounded; (b) a ReLU6-bounded input replaced by the high fp16
  plane of 2^8 x alone; (c) the fp32 mode answered in the bf16 mode's rounded form; (d) the folded BatchNorm shift without
  its moving_mean x fscale term; (e) the bias added after the ReLU; (f) a tap skipped at the last output column of a stride-2
  layer; (g) the head's label / box halves swapped at the split column; (h) the bf16 mode with the weights rounded AFTER
  fscale was folded into them (the layer kernels keep scale and shift in the epilogue and round the plain weights --
  csrc/ssd_net.hip finalize_fold_bn -- so neither of the two admitted bf16 forms may accept it);
* the glue of the GPU test: check_forward_graph with ``frozen=`` every BatchNorm layer, fed from the float32 activations
  of oracle/net_oracle.py for one MobileNetV2 and one VGG16 image: every layer passes; with ONE element of one tensor
  moved by 2^-12 of its value exactly the layers that write or read that tensor fail.

Measured (torch-CPU, one thread for the floor; the fp32 figures follow the BLAS's summation order and move by a few tenths
from host to host).  Columns: K, r32 max / rms, r16 max / rms, RMS_CAP; the mutants' (max E, rms E / rms r32) follow per shape
in the test's output (``pytest -s``).

    shape                     K     r32 max  rms     r16 max  rms    RMS_CAP   mutant a, rounded: max E, rms E / rms r32
    c3x3_cin3                 27     2.34   0.331    307.3   45.49    34.4      308    138
    c3x3_cin64               576     1.06   0.153     63.9   11.21    18.3      63.8   73.2
    c3x3_cin512             4608     0.73   0.094     27.5    4.00    10.7      27.6   42.7
    c3x3_cin1024            9216     0.50   0.077     15.3    2.96     9.6      15.3   42.4     <- under E_BAR: the RMS catches it
    c1x1_cin256_bn6          256     2.79   0.330     79.6   16.30    12.3      79.7   49.4
    c1x1_cin1024            1024     1.44   0.196     37.1    7.42     9.5      37.2   43.7
    c1x1_cin1280            1280     1.22   0.167     33.4    6.14     9.2      33.5   38.0
    c1x1_cin320_bn6          320     2.92   0.340     70.2   15.20    11.2      70.1   44.7
    c3x3_s2_cin256          2304     0.85   0.142     30.6    6.05    10.6      30.0   42.5
    c3x3_d6_cin512          4608     0.87   0.105     31.7    4.56    10.8      31.8   43.3
    head_k5184  deltas      5184     0.46   0.142     17.2    5.24     9.2      17.2   37.0
                probs                0.34   0.084     13.3    3.21     9.5      13.5   38.2
    head_k9216  deltas      9216     0.45   0.115     15.6    4.41     9.6      15.6   44.4     <- under E_BAR
                probs                0.27   0.068     11.3    2.36     8.7      11.4   38.9     <- under E_BAR

The smallest cap on these random shapes is 8.7 (the probabilities of the K = 9216 head pair).  FINDING on the real graphs (the
glue test, one image): the caps of the 66 + 35 layers are >= 6.7 except for the 84 probabilities of MobileNetV2's head 6 on
its 1 x 1 map: 4.1 on one host, 3.5 on another (an RMS over 84 elements follows the BLAS's summation order; the NumPy
oracle's own ratio there is 1.2).  So no bar is sized on the random shapes alone: the GPU file asserts its bar against the cap
of every layer it compares, on that layer's own reference, and a family's bar never exceeds it; here every layer of the
NumPy oracle has to sit under its own cap, and every cap but that one has to reach 5.
The other mutants sit far above both bars: (b) max E 248 - 715, rms ratio 776 - 816; (c) max E >= 3.0e3; (d) 9e5; (e) >= 8.8e4;
(f) 1.8e6; (g) deltas >= 3.5e6, probs >= 8.6e12; (h) >= 1.6e4 against either admitted bf16 form.  The NumPy oracle's own
layers (another summation order than torch's) score an rms ratio of at most 2.07 (MobileNetV2) / 2.26 (VGG16) in the glue
test, max E 4.5."""
import numpy as np
import pytest
import torch

import helpers
from oracle import layer_grad_oracle as lg
from oracle import net_oracle as no

FLOOR_BAR = 4.0
CAP_BAR = 5.0            # tests/test_block_oracle_gpu.py: FP32_BAR
RMS_BAR_MAX = 9.0        # the largest RMS bar of tests/test_layer_infer_gpu.py (its unsplit dma3 family): every mutant has to fail at it,
RMS_BAR = RMS_BAR_MAX    # and so fails at 5, the bar the cap is sized for, all the more
RMS_KEYS = ("out", "deltas", "probs")


def _spec(k=3, stride=1, pad="same", dil=1, bn=None, bias=False, act=None):
    return dict(kind="conv", name="layer", tin="in", tout="out", k=k, stride=stride, pad=pad, dil=dil, bn=bn, bias=bias,
                act=act, res=None)


def _head(anchors):
    return dict(kind="head", name="layer", tin="in", tout=None, k=3, stride=1, pad="same", dil=1, level=0, anchors=anchors,
                labels=21)


BIAS = dict(bias=True, act="relu")
BN6 = dict(bn="bn", act="relu6")
#        id                  spec                               B  H   W   Cin  Cout  ReLU6-bounded input
CASES = [("c3x3_cin3", _spec(**BIAS), 2, 9, 9, 3, 64, False),                       # conv1_1
         ("c3x3_cin64", _spec(**BIAS), 2, 9, 8, 64, 64, False),                     # conv1_2, conv2_1
         ("c3x3_cin512", _spec(**BIAS), 2, 7, 6, 512, 100, False),                  # conv4_x, conv5_x; Cout % 16 != 0
         ("c3x3_cin1024", _spec(**BIAS), 2, 5, 5, 1024, 64, False),                 # K of VGG16 head 2 as a plain conv
         ("c1x1_cin256_bn6", _spec(k=1, **BN6), 2, 7, 7, 256, 128, False),
         ("c1x1_cin1024", _spec(k=1, **BIAS), 2, 7, 6, 1024, 128, False),           # conv7, conv8_1
         ("c1x1_cin1280", _spec(k=1, pad="valid", **BIAS), 2, 7, 7, 1280, 128, True),   # extra1_1 behind Conv_1's ReLU6
         ("c1x1_cin320_bn6", _spec(k=1, **BN6), 2, 7, 7, 320, 128, False),          # Conv_1
         ("c3x3_s2_cin256", _spec(stride=2, **BIAS), 2, 9, 9, 256, 128, False),     # extra1_2, conv8_2
         ("c3x3_d6_cin512", _spec(dil=6, **BIAS), 2, 19, 19, 512, 64, False),       # conv6: the pad-6 taps need the real map
         ("head_k5184", _head(4), 2, 5, 5, 576, None, True),                        # MobileNetV2 head 1 (ReLU6 input)
         ("head_k9216", _head(6), 2, 5, 5, 1024, None, False)]                      # VGG16 head 2
IDS = [c[0] for c in CASES]
_DATA = {}


@pytest.fixture
def one_thread():
    """The fp32 floor follows the BLAS's summation order: one thread, so that it does not move with the host's cores."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _make(case):
    """The layer's tensors as fp32 values (what a device holds), computed once per case and shared."""
    name, spec, B, H, W, Cin, Cout, relu6_in = case
    if name in _DATA:
        return _DATA[name]
    g = torch.Generator().manual_seed(1000 + IDS.index(name))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    f = lambda a: a.to(torch.float32)
    x = (3.0 * rn(B, H, W, Cin)).clamp(0.0, 6.0) if relu6_in else (2.0 * rn(B, H, W, Cin)).clamp(min=0.0)
    K = spec["k"] ** 2 * Cin
    sd = (2.0 / K) ** 0.5
    t = {"x": f(x)}
    if spec["kind"] == "head":
        a, L = spec["anchors"], spec["labels"]
        t.update(w_label=f(2.0 * sd * rn(3, 3, Cin, a * L)), b_label=f(0.5 * rn(a * L)), w_box=f(sd * rn(3, 3, Cin, a * 4)),
                 b_box=f(0.1 * rn(a * 4)))
    else:
        t["w"] = f(sd * rn(spec["k"], spec["k"], Cin, Cout))
        if spec["bias"]:
            t["bias"] = f(0.1 * rn(Cout))
        if spec["bn"]:
            t.update(gamma=f(1.0 + 0.1 * rn(Cout)), beta=f(1.5 + 0.5 * rn(Cout)), moving_mean=f(0.3 * rn(Cout)),
                     moving_var=f(0.5 + torch.rand(Cout, generator=g, dtype=torch.float64)))
    _DATA[name] = (spec, t, K)
    return _DATA[name]


def _judge(spec, t, bad, yard, round_ops=None):
    """(max E, rms E / rms r32) per output of a candidate forward against the float64 reference, and whether the combined
    bar of the GPU test would let it pass."""
    ref, A = lg.layer_forward(spec, t, round_ops=round_ops), lg.layer_forward(spec, t, absolute=True, round_ops=round_ops)
    out, ok = {}, True
    for k in ref:
        E, _, rms = lg.e_stats(bad[k].numpy(), ref[k], A[k])
        ratio = rms / yard[k]["r32"][1]
        out[k] = (E, ratio)
        ok = ok and E <= lg.E_BAR and (k not in RMS_KEYS or ratio <= RMS_BAR)
    return out, ok


def _show(tag, name, res):
    print("infer mutant %-28s %-16s %s" % (tag, name, "  ".join("%s max E %.3g rms ratio %.3g" % (k, v[0], v[1])
                                                                for k, v in sorted(res.items()))))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_floor_and_cap(case, one_thread):
    spec, t, K = _make(case)
    yard = lg.forward_yardstick(spec, t)
    assert set(yard) == ({"deltas", "probs"} if spec["kind"] == "head" else {"out"})
    for k, y in sorted(yard.items()):
        (m32, r32), (m16, r16) = y["r32"], y["r16"]
        cap = r16 / (4.0 * r32)
        print("infer yardstick %-16s %-6s K = %-5d r32 max %.2f rms %.3f   r16 max %.1f rms %.2f   RMS_CAP %.1f" % (
            case[0], k, K, m32, r32, m16, r16, cap))
        assert m32 <= FLOOR_BAR, (case[0], k, m32)
        if k in RMS_KEYS:
            assert cap >= CAP_BAR, (case[0], k, cap)
    # the correct fp32 restatement passes the combined bar, with room
    res, ok = _judge(spec, t, lg.layer_forward(spec, t, dtype=torch.float32), yard)
    assert ok and all(v[1] <= 1.0 + 1e-9 for v in res.values()), res


def _operand_keys(spec):
    return ("x", "w_label", "w_box") if spec["kind"] == "head" else ("x", "w")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mutant_a_operands_cut_to_16_bits(case):
    spec, t, _ = _make(case)
    yard = lg.forward_yardstick(spec, t)
    for rounded in (False, True):
        cut = dict(t, **{k: lg.cut16(t[k], rounded=rounded) for k in _operand_keys(spec)})
        res, ok = _judge(spec, t, lg.layer_forward(spec, cut, dtype=torch.float32), yard)
        _show("a: 16 bits, " + ("rounded" if rounded else "truncated"), case[0], res)
        assert not ok, (case[0], rounded, res)


@pytest.mark.parametrize("case", [c for c in CASES if c[7]], ids=[c[0] for c in CASES if c[7]])
def test_mutant_b_fp16_pair_without_its_low_plane(case):
    """x in [0, 6] as the two-plane tiles hold it: fp16(2^8 x) + fp16(rest); here the rest is dropped."""
    spec, t, _ = _make(case)
    assert float(t["x"].max()) == 6.0 and float(t["x"].min()) == 0.0
    hi = (t["x"] * 256.0).to(torch.float16).to(torch.float32) / 256.0
    res, ok = _judge(spec, t, lg.layer_forward(spec, dict(t, x=hi), dtype=torch.float32), lg.forward_yardstick(spec, t))
    _show("b: fp16 high plane alone", case[0], res)
    assert not ok, res


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mutant_c_fp32_mode_answered_in_the_bf16_form(case):
    spec, t, _ = _make(case)
    res, ok = _judge(spec, t, lg.layer_forward(spec, t, dtype=torch.float32, round_ops=lg.bf16_rne), lg.forward_yardstick(spec, t))
    _show("c: bf16 operands in fp32 mode", case[0], res)
    assert not ok, res


BN_CASES = [c for c in CASES if c[1].get("bn")]


@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_mutant_d_folded_shift_without_the_moving_mean(case):
    spec, t, _ = _make(case)
    f = torch.float32
    fscale = t["gamma"] * torch.rsqrt(t["moving_var"] + lg.BN_EPS)
    conv = lg.conv_forward(t["x"], t["w"], spec["stride"], spec["dil"], lg._pads(spec, t["x"].shape[1], t["x"].shape[2]))
    good = {"out": (fscale * conv + (t["beta"] - t["moving_mean"] * fscale)).clamp(0.0, 6.0)}
    bad = {"out": (fscale * conv + t["beta"]).clamp(0.0, 6.0)}
    assert good["out"].dtype == f
    yard = lg.forward_yardstick(spec, t)
    assert _judge(spec, t, good, yard)[1]
    res, ok = _judge(spec, t, bad, yard)
    _show("d: shift without mean x fscale", case[0], res)
    assert not ok, res


BIAS_CASES = [c for c in CASES if c[1].get("bias")]


@pytest.mark.parametrize("case", BIAS_CASES, ids=[c[0] for c in BIAS_CASES])
def test_mutant_e_bias_added_after_the_relu(case):
    spec, t, _ = _make(case)
    conv = lg.conv_forward(t["x"], t["w"], spec["stride"], spec["dil"], lg._pads(spec, t["x"].shape[1], t["x"].shape[2]))
    res, ok = _judge(spec, t, {"out": conv.clamp(min=0.0) + t["bias"]}, lg.forward_yardstick(spec, t))
    _show("e: bias after the ReLU", case[0], res)
    assert not ok, res


def test_mutant_f_tap_skipped_at_the_last_column_of_a_stride_2_layer():
    case = [c for c in CASES if c[0] == "c3x3_s2_cin256"][0]
    spec, t, _ = _make(case)
    good = lg.layer_forward(spec, t, dtype=torch.float32)
    w = t["w"].clone()
    w[1, 1] = 0                                            # tap (ky, kx) = (1, 1) (kx = 2 reads the SAME padding there) ...
    bad = good["out"].clone()
    bad[:, :, -1] = lg.layer_forward(spec, dict(t, w=w), dtype=torch.float32)["out"][:, :, -1]      # ... of the last output column
    assert not torch.equal(bad, good["out"])
    res, ok = _judge(spec, t, {"out": bad}, lg.forward_yardstick(spec, t))
    _show("f: tap skipped, last column", case[0], res)
    assert not ok, res


HEAD_CASES = [c for c in CASES if c[1]["kind"] == "head"]


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_mutant_g_head_halves_swapped_at_the_split_column(case):
    """The fused head conv writes a L label columns, then a 4 box columns; here the split falls after a 4."""
    spec, t, _ = _make(case)
    a, L = spec["anchors"], spec["labels"]
    pads = lg._pads(spec, t["x"].shape[1], t["x"].shape[2])
    full = lg.conv_forward(t["x"], torch.cat([t["w_label"], t["w_box"]], 3), 1, 1, pads) + torch.cat([t["b_label"], t["b_box"]])
    deltas, z = full[..., :a * 4], full[..., a * 4:]
    probs = torch.softmax(z.reshape(z.shape[:3] + (a, L)), -1).reshape(z.shape)
    res, ok = _judge(spec, t, {"deltas": deltas, "probs": probs}, lg.forward_yardstick(spec, t))
    _show("g: head split column", case[0], res)
    assert not ok and res["deltas"][0] > lg.E_BAR and res["probs"][0] > lg.E_BAR, res


@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_mutant_h_bf16_weights_rounded_after_the_fold(case):
    """bf16 mode: the admitted forms are conv(bf16 x, bf16 w) x fscale + fshift and the same unrounded; a kernel that folds
    fscale into the weights first and rounds the product matches neither."""
    spec, t, _ = _make(case)
    f = torch.float32
    fscale = t["gamma"] * torch.rsqrt(t["moving_var"] + lg.BN_EPS)
    fshift = t["beta"] - t["moving_mean"] * fscale
    pads = lg._pads(spec, t["x"].shape[1], t["x"].shape[2])
    xq = lg.bf16_rne(t["x"]).to(f)
    good = {"out": (fscale * lg.conv_forward(xq, lg.bf16_rne(t["w"]).to(f), spec["stride"], spec["dil"], pads) + fshift).clamp(0.0, 6.0)}
    bad = {"out": (lg.conv_forward(xq, lg.bf16_rne(t["w"] * fscale).to(f), spec["stride"], spec["dil"], pads) + fshift).clamp(0.0, 6.0)}
    yard = lg.forward_yardstick(spec, t, round_ops=lg.bf16_rne)
    assert _judge(spec, t, good, yard, round_ops=lg.bf16_rne)[1]
    for form, ops in (("rounded", lg.bf16_rne), ("plain", None)):
        res, ok = _judge(spec, t, bad, yard if ops else lg.forward_yardstick(spec, t), round_ops=ops)
        _show("h: bf16(w fscale), %s form" % form, case[0], res)
        assert not ok, (form, res)


# ------------------------------------------------------------------ the glue of the GPU test, on the NumPy oracle's activations
def _glue(backbone, perturb=None):
    """check_forward_graph as tests/test_layer_infer_gpu.py drives it -- frozen = every BatchNorm layer, B = 1, yardstick
    recorded -- with fetch() served from net_oracle's float32 activations of one image.  perturb: (tensor, flat index
    chooser): that element is moved by 2^-12 of its value."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = helpers.hyper_params(backbone)
    w = helpers.synthetic_weights(backbone, hp)
    x = helpers.block_test_images(1, 300, gain=8.0 if backbone == "mobilenet_v2" else 1.0)
    acts = {}
    deltas, probs = no.forward(backbone, hp, w, x, acts)
    acts = dict(acts, input=x, deltas=deltas, probs=probs)
    if perturb:
        name, choose = perturb
        a = acts[name].copy()
        i = choose(a.reshape(-1))
        a.reshape(-1)[i] *= np.float32(1.0 + 2.0 ** -12)
        assert a.reshape(-1)[i] != acts[name].reshape(-1)[i]
        acts[name] = a
    specs = lg.layers(backbone, hp)
    report, yard = lg.Report(), {}
    info = lg.check_forward_graph(specs, acts.__getitem__, w, hp, 1, report, frozen={s["name"] for s in specs if s.get("bn")},
                                  yardstick=yard)
    return specs, report, info, yard


GLUE = {}


@pytest.mark.parametrize("backbone,n_layers,n_tensors,n_yard", [("mobilenet_v2", 66, 72, 49), ("vgg16", 35, 41, 29)])
def test_glue_every_layer_of_the_numpy_oracle_passes(backbone, n_layers, n_tensors, n_yard):
    specs, report, info, yard = _glue(backbone)
    GLUE[backbone] = True
    for line in report.lines():
        print(line)
    assert info["layers"] == n_layers and report.compared == n_tensors and len(yard) == n_yard
    assert not report.fails, report.fails[:10]
    worst, caps = 0.0, {}
    for s in specs:
        for k, y in yard.get(s["name"], {}).items():
            if k in RMS_KEYS:
                ratio = report.stats[(s["name"], k + ":" + (s["tout"] or s["name"]))][1] / y["r32"][1]
                cap = y["r16"][1] / (4.0 * y["r32"][1])
                worst = max(worst, ratio)
                caps[(s["name"], k)] = cap
                assert ratio <= min(cap, RMS_BAR_MAX), (s["name"], k, ratio, cap)
    low = min(caps, key=caps.get)
    print("%s: largest rms ratio of the NumPy oracle's own layers %.2f; smallest cap %.1f (%s %s)" % ((backbone, worst, caps[low]) + low))
    assert sorted(caps.values())[1] >= CAP_BAR, sorted(caps.items(), key=lambda kv: kv[1])[:3]      # (the smallest: the docstring's finding)
    if backbone == "mobilenet_v2":          # the gain-8 image fires both clamps of every ReLU6 of the frozen graph
        c = info["clamps"]
        assert len(c) == 35 and min(v[0] for v in c.values()) >= 0.01 and min(v[1] for v in c.values()) >= 0.10, c


@pytest.mark.parametrize("backbone,tensor,expect", [
    # read by the depthwise conv alone (K = 9); an element strictly inside (0, 6)
    ("mobilenet_v2", "block_3_expand_relu", {"block_3_expand", "block_3_depthwise"}),
    # the largest element: the maximum of its pool window (bit for bit), one of 512 terms of its pixel's norm
    ("vgg16", "conv4_3", {"conv4_3", "pool4", "l2_normalization"})])
def test_glue_names_the_layers_around_a_perturbed_tensor(backbone, tensor, expect):
    choose = (lambda a: int(np.argmin(np.abs(a - 3.0)))) if backbone == "mobilenet_v2" else (lambda a: int(np.argmax(a)))
    _, report, _, _ = _glue(backbone, perturb=(tensor, choose))
    assert {f.split()[0] for f in report.fails} == expect, report.fails
