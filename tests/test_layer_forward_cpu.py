"""Self-tests of the FORWARD formulas of the float64 layer oracle (oracle/layer_grad_oracle.py: layer_forward) and of
their A in the metric E = |got - ref64| / (u A): no GPU.

* layer_forward in float64 equals the torch forward of every layer kind (tests/test_layer_grad_cpu.py: _forward), of a
  head pair and of a conv behind a frozen BatchNorm (written there in the subtract-first form, not the folded one);
* the plain fp32 restatement of the same formulas scores E <= 4 on every output (the floor; the figures are printed
  and recorded in the oracle's docstring);
* six subtly wrong forwards, each computed from the reference formulas alone, score E > 4 x E_BAR = 64 on the tensor
  they damage: the bar of 16 separates right from subtly wrong;
* the metric's edges: an all-zero pixel through the L2 norm (the 1e-12 floor; A == 0, exact match), a softmax row with
  one logit 80 above the rest (p = 1 exactly and p = e^-80 ~ 1.8e-35, a normal fp32 number, against A > 0);
* check_forward_graph itself on a tiny graph with every layer kind of MobileNetV2 and two head levels, against a plain
  fp32 implementation of it: tensor counts, the frozen form (pre / mean / var never asked for), the head slices, the
  bf16 mode's two-form rule, and planted defects reported at the layer and tensor they sit in."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_grad_oracle as lg
from test_layer_grad_cpu import CASES, _f32_inputs, _forward, _make, _nchw, _nhwc, _spec

FLOOR_BAR = 4.0
MUTANT_BAR = 4.0 * lg.E_BAR


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


HEAD = dict(kind="head", name="layer", tin="in", tout=None, k=3, stride=1, pad="same", dil=1, level=0, anchors=4, labels=21)


def _make_head(seed=0, B=2, H=5, W=4, Cin=32, spec=HEAD):
    """Random head pair; K = 9 Cin."""
    g = torch.Generator().manual_seed(100 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a, L = spec["anchors"], spec["labels"]
    sd = (2.0 / (9 * Cin)) ** 0.5
    return {"x": rn(B, H, W, Cin).clamp(min=0.0), "w_label": 2.0 * sd * rn(3, 3, Cin, a * L), "b_label": 0.5 * rn(a * L),
            "w_box": sd * rn(3, 3, Cin, a * 4), "b_box": 0.1 * rn(a * 4)}


def _head_torch(t, spec=HEAD):
    conv = lambda w, b: _nhwc(F.conv2d(_nchw(t["x"]), w.permute(3, 2, 0, 1), b, padding=1))
    z = conv(t["w_label"], t["b_label"])
    p = torch.softmax(z.reshape(z.shape[:3] + (-1, spec["labels"])), -1).reshape(z.shape)
    return {"deltas": conv(t["w_box"], t["b_box"]), "probs": p}


FROZEN = ("frozen_bn_relu6_res", _spec(bn="bn", act="relu6", res="skip"), 2, 7, 6, 8, 8)


def _make_frozen(seed=0):
    spec, t, _ = _make(FROZEN, seed)
    g = torch.Generator().manual_seed(200 + seed)
    t = {k: v for k, v in t.items() if k in ("x", "w", "gamma", "beta", "res")}
    t["moving_mean"] = 0.3 * torch.randn(8, generator=g, dtype=torch.float64)
    t["moving_var"] = 0.5 + torch.rand(8, generator=g, dtype=torch.float64)
    return spec, t


def _frozen_torch(spec, t):
    pre = _nhwc(F.conv2d(_nchw(t["x"]), t["w"].permute(3, 2, 0, 1), padding=1))
    z = (pre - t["moving_mean"]) / torch.sqrt(t["moving_var"] + lg.BN_EPS) * t["gamma"] + t["beta"]
    return z.clamp(0.0, 6.0) + t["res"]


def _close(got, want):
    return float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_forward_is_torch(case):
    spec, t, _ = _make(case)
    ref = lg.layer_forward(spec, t)
    assert set(ref) == ({"pre", "out"} if spec.get("bn") else {"out"})
    assert _close(ref["out"], t["out"])                 # _make's out: _forward of the same leaves
    if spec.get("bn"):
        assert _close(ref["pre"], t["pre"])
    if spec["kind"] == "pool":
        assert torch.equal(ref["out"], t["out"]) and not lg.layer_forward(spec, t, absolute=True)["out"].any()


def test_oracle_forward_is_torch_head_and_frozen():
    t = _make_head()
    ref, want = lg.layer_forward(HEAD, t), _head_torch(t)
    assert set(ref) == {"deltas", "probs"} and _close(ref["deltas"], want["deltas"]) and _close(ref["probs"], want["probs"])
    spec, t = _make_frozen()
    ref = lg.layer_forward(spec, t)
    assert set(ref) == {"out"} and _close(ref["out"], _frozen_torch(spec, t))
    o = ref["out"] - t["res"]
    assert (o == 6).any() and (o == 0).any()


def _floor(spec, t):
    t = _f32_inputs(t)
    ref, A = lg.layer_forward(spec, t), lg.layer_forward(spec, t, absolute=True)
    got = lg.layer_forward(spec, t, dtype=torch.float32)
    return {k: lg.e_metric(got[k].numpy(), ref[k], A[k]) for k in ref}


@pytest.mark.parametrize("case", CASES + [FROZEN, ("head",)], ids=[c[0] for c in CASES] + ["frozen", "head"])
def test_fp32_forward_restatement_scores_at_the_floor(case):
    worst = {}
    for seed in range(3):
        if case[0] == "head":
            spec, t = HEAD, _make_head(seed)
        elif case is FROZEN:
            spec, t = _make_frozen(seed)
        else:
            spec, t, _ = _make(case, seed)
        for k, (E, i) in _floor(spec, t).items():
            worst[k] = max(worst.get(k, 0.0), E)
            assert E <= FLOOR_BAR, "%s %s: E = %.3g at %d" % (case[0], k, E, i)
    print("fp32 forward floor %-20s worst E %s" % (case[0], "  ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


# ------------------------------------------------------------------ mutants
def _dense_bn_case():
    return ("dense_bn", _spec(bn="bn", act="relu6"), 2, 9, 8, 16, 24)          # K = 144


_cut16 = lg.cut16      # fp32 -> its leading 16 significand bits (truncated): the oracle's helper, shared with tests/test_layer_infer_cpu.py


def _e(got, ref, A):
    return lg.e_metric(got.numpy(), ref, A)[0]


def test_mutant_skipped_tap_at_last_column():
    spec, t, _ = _make(_dense_bn_case())
    t = _f32_inputs(t)
    ref, A = lg.layer_forward(spec, t), lg.layer_forward(spec, t, absolute=True)
    got = lg.layer_forward(spec, t, dtype=torch.float32)
    assert _e(got["pre"], ref["pre"], A["pre"]) <= FLOOR_BAR
    w = t["w"].clone()
    w[1, 0] = 0                                            # tap (ky, kx) = (1, 0) ...
    bad = got["pre"].clone()
    bad[:, :, -1] = lg.layer_forward(spec, dict(t, w=w), dtype=torch.float32)["pre"][:, :, -1]       # ... of the last output column
    E = _e(bad, ref["pre"], A["pre"])
    print("forward mutant, skipped tap: pre E = %.3g" % E)
    assert E > MUTANT_BAR


def test_mutant_operands_cut_to_16_bits():
    """The figure a raised bar of a layer class is capped by (a quarter of it): computed from the reference alone."""
    spec, t, _ = _make(_dense_bn_case())
    t = _f32_inputs(t)
    ref, A = lg.layer_forward(spec, t), lg.layer_forward(spec, t, absolute=True)
    bad = lg.layer_forward(spec, dict(t, x=_cut16(t["x"]), w=_cut16(t["w"])), dtype=torch.float32)
    E_pre = _e(bad["pre"], ref["pre"], A["pre"])
    th = _f32_inputs(_make_head())
    ref, A = lg.layer_forward(HEAD, th), lg.layer_forward(HEAD, th, absolute=True)
    cut = dict(th, x=_cut16(th["x"]), w_label=_cut16(th["w_label"]), w_box=_cut16(th["w_box"]))
    bad = lg.layer_forward(HEAD, cut, dtype=torch.float32)
    E_probs, E_deltas = _e(bad["probs"], ref["probs"], A["probs"]), _e(bad["deltas"], ref["deltas"], A["deltas"])
    print("forward mutant, 16-bit operands: pre E = %.3g (K = 144), probs E = %.3g, deltas E = %.3g (K = 288)" % (E_pre, E_probs, E_deltas))
    assert E_pre > MUTANT_BAR and E_probs > MUTANT_BAR and E_deltas > MUTANT_BAR


def _bn_case(res=False):
    case = ("bn", _spec(k=1, bn="bn", act="relu6", res="skip" if res else None), 2, 8, 9, 6, 16)
    spec, t, _ = _make(case)
    t = _f32_inputs(t)
    t["gamma"] = t["gamma"] * 3.0                            # both clamps fire
    return spec, t, lg.layer_forward(spec, t), lg.layer_forward(spec, t, absolute=True)


def test_mutant_istd_without_eps():
    spec, t, ref, A = _bn_case()
    assert _e(lg.layer_forward(spec, t, dtype=torch.float32)["out"], ref["out"], A["out"]) <= FLOOR_BAR
    z = t["gamma"] * (t["pre"] - t["mean"]) * torch.rsqrt(t["var"]) + t["beta"]
    E = _e(z.clamp(0.0, 6.0), ref["out"], A["out"])
    print("forward mutant, istd without eps: out E = %.3g" % E)
    assert E > MUTANT_BAR


def test_mutant_residual_added_before_the_activation():
    spec, t, ref, A = _bn_case(res=True)
    assert _e(lg.layer_forward(spec, t, dtype=torch.float32)["out"], ref["out"], A["out"]) <= FLOOR_BAR
    z = t["gamma"] * (t["pre"] - t["mean"]) * torch.rsqrt(t["var"] + lg.BN_EPS) + t["beta"]
    E = _e((z + t["res"]).clamp(0.0, 6.0), ref["out"], A["out"])
    print("forward mutant, residual before the activation: out E = %.3g" % E)
    assert E > MUTANT_BAR


def test_mutant_relu6_without_its_upper_clamp():
    spec, t, ref, A = _bn_case()
    assert float((ref["out"] == 6).double().mean()) >= 0.01 and float((ref["out"] == 0).double().mean()) >= 0.01
    z = t["gamma"] * (t["pre"] - t["mean"]) * torch.rsqrt(t["var"] + lg.BN_EPS) + t["beta"]
    E = _e(z.clamp(min=0.0), ref["out"], A["out"])
    print("forward mutant, ReLU instead of ReLU6: out E = %.3g" % E)
    assert E > MUTANT_BAR


def test_mutant_head_halves_swapped_at_the_split_column():
    """The fused head conv writes a*L label columns, then a*4 box columns; here the split falls after a*4."""
    t = _f32_inputs(_make_head())
    ref, A = lg.layer_forward(HEAD, t), lg.layer_forward(HEAD, t, absolute=True)
    a, L = HEAD["anchors"], HEAD["labels"]
    pads = lg._pads(HEAD, t["x"].shape[1], t["x"].shape[2])
    full = lg.conv_forward(t["x"], torch.cat([t["w_label"], t["w_box"]], 3), 1, 1, pads) + torch.cat([t["b_label"], t["b_box"]])
    deltas, z = full[..., :a * 4], full[..., a * 4:]
    probs = torch.softmax(z.reshape(z.shape[:3] + (a, L)), -1).reshape(z.shape)
    E_p, E_d = _e(probs, ref["probs"], A["probs"]), _e(deltas, ref["deltas"], A["deltas"])
    print("forward mutant, head split column: probs E = %.3g, deltas E = %.3g" % (E_p, E_d))
    assert E_p > MUTANT_BAR and E_d > MUTANT_BAR


# ------------------------------------------------------------------ the metric's edges
def test_l2norm_zero_pixel_hits_the_floor():
    spec, t, _ = _make([c for c in CASES if c[0] == "l2norm"][0])
    x = t["x"].clone()
    x[0, 0, 0] = 0.0                    # sum x^2 = 0 -> rsqrt(1e-12): out = 0 and A = 0, exact match asked
    x[0, 0, 1] *= 1e-8                  # below the floor too, but not zero: out = gamma x 1e6
    t = _f32_inputs(dict(t, x=x))
    ref, A = lg.layer_forward(spec, t), lg.layer_forward(spec, t, absolute=True)
    got = lg.layer_forward(spec, t, dtype=torch.float32)
    assert not ref["out"][0, 0, 0].any() and not A["out"][0, 0, 0].any() and not got["out"][0, 0, 0].any()
    assert torch.allclose(ref["out"][0, 0, 1], t["gamma"].double() * t["x"][0, 0, 1].double() * 1e6, rtol=1e-12, atol=0)
    assert _e(got["out"], ref["out"], A["out"]) <= FLOOR_BAR
    bad = got["out"].clone()
    bad[0, 0, 0, 3] = 1e-30
    assert _e(bad, ref["out"], A["out"]) == np.inf


def test_softmax_row_with_one_logit_80_above():
    z = torch.zeros(1, 1, 1, 2, 21, dtype=torch.float64)
    z[..., 0, :] = torch.linspace(-1, 1, 21, dtype=torch.float64)
    z[..., 0, 5] = 80.0
    z[..., 1, :] = torch.linspace(-2, 2, 21, dtype=torch.float64)
    a_z = z.abs() + 1.0
    p, A = lg.softmax_forward(z, a_z), lg.softmax_forward(z, a_z, absolute=True)
    assert float(p[..., 0, 5]) == 1.0 and 0.0 < float(p[..., 0, 0]) < 1e-34 and bool((A > 0).all())
    got = lg.softmax_forward(z.float(), a_z.float())
    assert float(got[..., 0, 5]) == 1.0
    assert _e(got, p, A) <= FLOOR_BAR
    flushed = got.clone()
    flushed[..., 0, :5] = 0.0            # exactly 0 where the reference holds e^-80: not an fp32 rounding of it
    assert _e(flushed, p, A) > MUTANT_BAR


# ------------------------------------------------------------------ check_forward_graph on a tiny graph
TINY_HP = {"feature_map_shapes": [5, 5], "aspect_ratios": [[1., 2., 0.5], [1., 2.]], "total_labels": 5}


def _tiny_graph():
    c = lg._conv
    specs = [c("c1", "input", "a1", 3, 2, "correct", bn="bn1", act="relu6"),
             c("d1", "a1", "a2", 3, 1, "same", bn="bn2", act="relu6", kind="dw"),
             c("p1", "a2", "a3", bn="bn3"),
             c("e1", "a3", "a4", bn="bn4", act="relu6"),
             c("p2", "a4", "a5", bn="bn5", res="a3"),
             c("x1", "a5", "a6", 1, 1, "valid", bias=True, act="relu")] + lg.head_specs(TINY_HP, ["a4", "a6"])
    g = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(torch.float32).numpy()
    w, cin = {}, {"c1": (3, 8), "p1": (8, 8), "e1": (8, 16), "p2": (16, 8), "x1": (8, 12)}
    for s in specs[:6]:
        if s["kind"] == "dw":
            w["d1/depthwise_kernel"] = 0.5 * rn(3, 3, 8, 1)
            co = 8
        else:
            ci, co = cin[s["name"]]
            w[s["name"] + "/kernel"] = rn(s["k"], s["k"], ci, co) * np.float32((2.0 / (s["k"] ** 2 * ci)) ** 0.5)
        if s["bn"]:
            w[s["bn"] + "/gamma"], w[s["bn"] + "/beta"] = 3.0 + 0.1 * rn(co), 1.5 + 0.1 * rn(co)
            w[s["bn"] + "/moving_mean"], w[s["bn"] + "/moving_variance"] = 0.1 * rn(co), 1.0 + 0.2 * np.abs(rn(co))
        else:
            w[s["name"] + "/bias"] = 0.1 * rn(co)
    for i, (ci, a) in enumerate(((16, 4), (12, 3)), start=1):
        w["%d_conv_label_output/kernel" % i], w["%d_conv_label_output/bias" % i] = 0.2 * rn(3, 3, ci, a * 5), 0.1 * rn(a * 5)
        w["%d_conv_boxes_output/kernel" % i], w["%d_conv_boxes_output/bias" % i] = 0.1 * rn(3, 3, ci, a * 4), 0.1 * rn(a * 4)
    return specs, w, np.abs(rn(2, 9, 9, 3))


def _tiny_device(specs, w, x, frozen=(), rounded=(), round_x_only=(), relu_for_relu6=(), swap_levels=False):
    """A plain fp32 implementation of the graph (layer_forward in float32, free running) with the tensors a device would
    serve by name; the keyword sets plant one defect each."""
    f32 = torch.float32
    T, probs, deltas, asked = {"input": x}, [], [], []
    for s in specs:
        rnd = lg.bf16_rne if s["name"] in rounded else None
        t = {"x": T[s["tin"]]}
        if s["name"] in round_x_only:
            t["x"] = lg.bf16_rne(t["x"]).to(f32).numpy()
        if s["kind"] == "head":
            i = s["level"] + 1
            t.update(w_label=w["%d_conv_label_output/kernel" % i], b_label=w["%d_conv_label_output/bias" % i],
                     w_box=w["%d_conv_boxes_output/kernel" % i], b_box=w["%d_conv_boxes_output/bias" % i])
            r = lg.layer_forward(s, t, dtype=f32, round_ops=rnd)
            probs.append(r["probs"].numpy().reshape(2, -1, 5))
            deltas.append(r["deltas"].numpy().reshape(2, -1, 4))
            continue
        t["w"] = w[s["name"] + ("/depthwise_kernel" if s["kind"] == "dw" else "/kernel")]
        if s["bias"]:
            t["bias"] = w[s["name"] + "/bias"]
        if s["res"]:
            t["res"] = T[s["res"]]
        if s["bn"]:
            t["gamma"], t["beta"] = w[s["bn"] + "/gamma"], w[s["bn"] + "/beta"]
            if s["name"] in frozen:
                t["moving_mean"], t["moving_var"] = w[s["bn"] + "/moving_mean"], w[s["bn"] + "/moving_variance"]
            else:
                pre = lg.layer_forward(dict(s, bn=None, act=None, res=None), t, dtype=f32, round_ops=rnd)["out"]      # the bare conv
                mean, var, _, _, _ = lg.batch_stats(pre, f32)
                t["pre"], t["mean"], t["var"] = pre.numpy(), mean.numpy(), var.numpy()
                for k in ("pre", "mean", "var"):
                    T[k + ":" + s["name"]] = t[k]
        spec = dict(s, act="relu") if s["name"] in relu_for_relu6 else s
        T[s["tout"]] = lg.layer_forward(spec, t, dtype=f32, round_ops=rnd)["out"].numpy()
    if swap_levels:
        probs, deltas = probs[::-1], deltas[::-1]
    T["probs"], T["deltas"] = np.concatenate(probs, 1), np.concatenate(deltas, 1)

    def fetch(name):
        asked.append(name)
        return T[name]
    return fetch, asked


def _run_tiny(frozen=(), round_ops=None, **defect):
    specs, w, x = _tiny_graph()
    fetch, asked = _tiny_device(specs, w, x, frozen=frozen, **defect)
    report = lg.Report()
    info = lg.check_forward_graph(specs, fetch, w, TINY_HP, 2, report, frozen=frozen, round_ops=round_ops)
    return report, info, asked


def test_check_forward_graph_on_a_tiny_graph():
    report, info, _ = _run_tiny()
    assert info["layers"] == 8 and report.compared == 5 * 2 + 1 + 2 * 2 and not report.fails, report.fails
    assert set(info["clamps"]) == {"c1", "d1", "e1"} and all(s6 > 0 and s0 > 0 for s6, s0 in info["clamps"].values())
    # frozen layers: the folded form, and their pre / mean / var are never asked for
    report, info, asked = _run_tiny(frozen={"c1", "d1", "p1"})
    assert report.compared == 3 + 2 * 2 + 1 + 2 * 2 and not report.fails, report.fails
    assert not [n for n in asked if n.split(":")[-1] in ("c1", "d1", "p1") and ":" in n]
    report, _, _ = _run_tiny(frozen={"e1"}, relu_for_relu6={"e1"})
    assert [f for f in report.fails if f.startswith("e1 out")]
    # planted defects are named
    report, _, _ = _run_tiny(relu_for_relu6={"e1"})
    assert len(report.fails) == 1 and report.fails[0].startswith("e1 out"), report.fails
    report, _, _ = _run_tiny(swap_levels=True)
    assert {f.split()[0] for f in report.fails} == {"1_conv_heads", "2_conv_heads"}


def test_check_forward_graph_two_form_rule():
    """bf16 mode: a dense conv passes with both operands rounded or with neither; one operand rounded matches neither
    form, and without round_ops a rounded conv fails."""
    report, _, _ = _run_tiny(round_ops=lg.bf16_rne, rounded={"e1", "x1", "2_conv_heads"})
    assert report.compared == 15 and not report.fails, report.fails
    report, _, _ = _run_tiny(round_ops=lg.bf16_rne)
    assert not report.fails, report.fails
    report, _, _ = _run_tiny(rounded={"e1"})
    assert [f.split(":")[0] for f in report.fails] == ["e1 pre"], report.fails
    report, _, _ = _run_tiny(round_ops=lg.bf16_rne, round_x_only={"p2"})
    assert [f.split(":")[0] for f in report.fails] == ["p2 pre"], report.fails
