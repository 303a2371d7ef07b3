"""Self-tests of the float64 layer oracle (oracle/layer_grad_oracle.py) and of its metric
E = |got - ref64| / (u A): no GPU.

* the oracle's hand-written backward of every layer kind equals torch autograd (float64) of the layer's
  forward (so the formulas the GPU tests hold the kernels to are the right ones);
* a plain fp32 restatement of the same local backward scores E <= 4 (the floor of the metric: its worst E
  per layer kind is printed and recorded in the oracle's docstring);
* three subtly wrong fp32 restatements -- one tap skipped at the last output column, one 32-row slab of M
  left out of a weight gradient, a residual gradient overwritten instead of accumulated -- each score
  E > 100 on at least one element: the bar of 16 separates right from subtly wrong."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_grad_oracle as lg

FLOOR_BAR = 4.0
MUTANT_BAR = 100.0


@pytest.fixture(autouse=True)
def _one_thread():
    """The fp32 floor depends on the summation order of the BLAS: one thread, so that it does not move with the host's
    core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _spec(kind="conv", k=3, stride=1, pad="same", dil=1, bn=None, bias=False, act=None, res=None, tin="in"):
    return dict(kind=kind, name="layer", tin=tin, tout="out", k=k, stride=stride, pad=pad, dil=dil, bn=bn, bias=bias,
                act=act, res=res)


#        id                    spec                                                    B  H  W  Cin Cout
CASES = [("dense3x3_s1", _spec(bias=True, act="relu"), 2, 7, 6, 5, 12),
         ("dense3x3_s2", _spec(stride=2, bias=True, act="relu"), 2, 9, 8, 6, 8),
         ("dense3x3_dil", _spec(dil=2, bias=True, act="relu"), 1, 9, 10, 4, 8),
         ("conv1x1", _spec(k=1, bn="bn"), 2, 6, 7, 12, 8),
         ("dw_s1", _spec(kind="dw", bn="bn", act="relu6"), 2, 7, 5, 8, 8),
         ("dw_s2_correct_pad", _spec(kind="dw", stride=2, pad="correct", bn="bn", act="relu6"), 2, 8, 7, 8, 8),
         ("bn_relu6", _spec(k=1, bn="bn", act="relu6"), 2, 8, 9, 6, 16),
         ("bn_residual", _spec(k=1, bn="bn", res="skip"), 2, 8, 9, 8, 8),
         ("bias_relu", _spec(k=1, pad="valid", bias=True, act="relu"), 2, 5, 5, 16, 8),
         ("maxpool2x2", dict(kind="pool", name="layer", tin="in", tout="out", k=2, stride=2, pad="same"), 2, 7, 6, 8, 8),
         ("maxpool3x3_s1", dict(kind="pool", name="layer", tin="in", tout="out", k=3, stride=1, pad="same"), 2, 6, 7, 8, 8),
         ("l2norm", dict(kind="l2norm", name="layer", tin="in", tout="out"), 2, 5, 6, 16, 16)]


def _nchw(a):
    return a.permute(0, 3, 1, 2)


def _nhwc(a):
    return a.permute(0, 2, 3, 1)


def _forward(spec, x, P, dtype=torch.float64):
    """torch forward of one layer on NHWC leaves; returns (out, intermediates)."""
    kind = spec["kind"]
    if kind == "pool":
        cells, _, _ = lg.pool_windows(x, spec)
        return cells.max(0).values, {}
    if kind == "l2norm":
        return x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-12)) * P["gamma"], {}
    pt, pb, pl, pr = lg._pads(spec, x.shape[1], x.shape[2])
    xp = F.pad(_nchw(x), (pl, pr, pt, pb))
    if kind == "dw":
        w = P["w"][..., 0].permute(2, 0, 1).unsqueeze(1)
        pre = _nhwc(F.conv2d(xp, w, stride=spec["stride"], groups=x.shape[3]))
    else:
        pre = _nhwc(F.conv2d(xp, P["w"].permute(3, 2, 0, 1), stride=spec["stride"], dilation=spec["dil"]))
    inter = {}
    if spec["bn"]:
        mean = pre.mean((0, 1, 2))
        var = ((pre - mean) ** 2).mean((0, 1, 2))
        inter = {"pre": pre, "mean": mean, "var": var}
        z = (pre - mean) * torch.rsqrt(var + lg.BN_EPS) * P["gamma"] + P["beta"]
    else:
        z = pre + P["bias"] if spec["bias"] else pre
    if spec["act"] == "relu6":
        z = z.clamp(0.0, 6.0)
    elif spec["act"] == "relu":
        z = z.clamp(min=0.0)
    if spec["res"]:
        z = z + P["skip"]
    return z, inter


def _make(case, seed=0):
    """Random layer: leaves (float64, requires_grad), the tensors the oracle is fed, autograd's gradients."""
    _, spec, B, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rn(B, H, W, Cin)
    P = {}
    if spec["kind"] == "conv":
        P["w"] = rn(spec["k"], spec["k"], Cin, Cout) * (2.0 / (spec["k"] ** 2 * Cin)) ** 0.5
    elif spec["kind"] == "dw":
        P["w"] = rn(3, 3, Cin, 1) * 0.5
    if spec["kind"] == "l2norm":
        P["gamma"] = 20.0 + rn(Cin)
    if spec.get("bn"):
        P["gamma"], P["beta"] = 1.0 + 0.1 * rn(Cout), 2.0 + rn(Cout)        # ReLU6: both clamps fire
    if spec.get("bias"):
        P["bias"] = 0.1 * rn(Cout)
    if spec.get("res"):
        P["skip"] = rn(B, *lg.out_hw(spec, H, W), Cout)
    leaves = dict(P, x=x)
    for v in leaves.values():
        v.requires_grad_(True)
    out, inter = _forward(spec, x, P)
    dout = rn(*out.shape)
    grads = dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), dout)))
    t = {"x": x.detach(), "dout": dout, "out": out.detach()}
    for k, key in (("w", "w"), ("gamma", "gamma"), ("beta", "beta"), ("bias", "bias"), ("skip", "res")):   # (the last three: the forward's)
        if k in P:
            t[key] = P[k].detach()
    for k, v in inter.items():
        t[k] = v.detach()
    return spec, t, grads


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_backward_is_autograd(case):
    spec, t, grads = _make(case)
    ref = lg.layer_backward(spec, t)
    pairs = {"dx": "x", "dw": "w", "dgamma": "gamma", "dbeta": "beta", "dbias": "bias", "dres": "skip"}
    seen = 0
    for key, leaf in pairs.items():
        if key in ref:
            seen += 1
            got, want = ref[key], grads[leaf]
            if key == "dx" and spec["kind"] == "pool":
                keep = ~ref["tied"]
                got, want = got[keep], want[keep]
            assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), key
    want = {"pool": {"dx"}, "l2norm": {"dx", "dgamma"}}.get(spec["kind"])
    if want is None:
        want = {"dx", "dw"} | ({"dgamma", "dbeta"} if spec["bn"] else set()) | ({"dbias"} if spec["bias"] else set()) | \
               ({"dres"} if spec["res"] else set())
    assert set(ref) - {"tied"} == want and seen == len(want)
    if spec.get("bn"):
        mean, var, _, _, _ = lg.batch_stats(t["pre"])
        assert torch.allclose(mean, t["mean"], rtol=0, atol=1e-13) and torch.allclose(var, t["var"], rtol=0, atol=1e-13)


def _f32_inputs(t):
    """The tensors as an fp32 implementation holds them (the oracle is then fed the SAME rounded values)."""
    return {k: v.to(torch.float32) for k, v in t.items()}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp32_restatement_scores_at_the_floor(case):
    worst = 0.0
    for seed in range(3):
        spec, t, _ = _make(case, seed)
        t = _f32_inputs(t)
        ref, A = lg.layer_backward(spec, t), lg.layer_backward(spec, t, absolute=True)
        got = lg.layer_backward(spec, t, dtype=torch.float32)
        for key in ref:
            if key == "tied":
                continue
            E, i = lg.e_metric(got[key].numpy(), ref[key], A[key], ref.get("tied") if key == "dx" else None)
            worst = max(worst, E)
            assert E <= FLOOR_BAR, "%s %s: E = %.3g at %d" % (case[0], key, E, i)
    print("fp32 floor %-20s worst E %.2f" % (case[0], worst))


def test_metric_exact_zero_and_nan():
    one = torch.ones(4, dtype=torch.float64)
    assert lg.e_metric(np.ones(4, np.float32), one, one)[0] == 0.0
    assert lg.e_metric(np.array([0, 0, 1e-30, 0], np.float32), 0 * one, 0 * one)[0] == np.inf      # A == 0: exact match only
    assert lg.e_metric(np.array([1, np.nan, 1, 1], np.float32), one, one) == (np.inf, 1)
    E, i = lg.e_metric(np.array([1, 1, 1 + 2.0 ** -20, 1], np.float32), one, one)
    assert i == 2 and abs(E - 16.0) < 1e-9


def _dense_case():
    return ("dense", _spec(bias=False, act=None), 2, 9, 8, 16, 24)


def test_mutant_skipped_tap_at_last_column():
    spec, t, _ = _make(_dense_case())
    t = _f32_inputs(t)
    ref, A = lg.layer_backward(spec, t), lg.layer_backward(spec, t, absolute=True)
    got = lg.layer_backward(spec, t, dtype=torch.float32)
    assert lg.e_metric(got["dx"].numpy(), ref["dx"], A["dx"])[0] <= FLOOR_BAR
    # tap (ky, kx) = (1, 0) of the last output column ox = Wo - 1 lands on input column Wo - 1 - pad_l + 0
    Wo = t["dout"].shape[2]
    ix = Wo - 1 - 1
    bad = got["dx"].clone()
    bad[:, :, ix] -= t["dout"][:, :, Wo - 1] @ t["w"][1, 0].t()
    E, _ = lg.e_metric(bad.numpy(), ref["dx"], A["dx"])
    print("skipped tap: E = %.3g" % E)
    assert E > MUTANT_BAR


def test_mutant_dropped_32_row_slab_in_weight_gradient():
    spec, t, _ = _make(_dense_case())
    t = _f32_inputs(t)
    ref, A = lg.layer_backward(spec, t), lg.layer_backward(spec, t, absolute=True)
    g = t["dout"].clone()
    assert g[..., 0].numel() >= 96
    g.view(-1, g.shape[-1])[32:64] = 0            # rows 32..63 of M never reach the accumulator
    bad = lg.layer_backward(spec, dict(t, dout=g), dtype=torch.float32)
    E, _ = lg.e_metric(bad["dw"].numpy(), ref["dw"], A["dw"])
    print("dropped slab: E = %.3g" % E)
    assert E > MUTANT_BAR


def test_mutant_residual_overwritten():
    case = [c for c in CASES if c[0] == "bn_residual"][0]
    spec, t, _ = _make(case)
    t = _f32_inputs(t)
    # the skip tensor has two consumers: the residual add (dres) and the layer's own conv input (dx);
    # Cin == Cout and k = 1 / stride 1 make the two contributions the same shape
    ref, A = lg.layer_backward(spec, t), lg.layer_backward(spec, t, absolute=True)
    got = lg.layer_backward(spec, t, dtype=torch.float32)
    total, total_A = ref["dx"] + ref["dres"], A["dx"] + A["dres"]
    assert lg.e_metric((got["dx"] + got["dres"]).numpy(), total, total_A)[0] <= FLOOR_BAR
    E, _ = lg.e_metric(got["dx"].numpy(), total, total_A)          # second write replaced the first
    print("overwritten residual: E = %.3g" % E)
    assert E > MUTANT_BAR


def test_graph_descriptions_cover_every_parameter():
    """Every trainable parameter of both graphs belongs to exactly one layer of the description, and (the forward side)
    every training activation the graph records -- what the step's fetch hook serves by name -- is the ``tout`` of exactly
    one layer, read only after it was written."""
    import helpers
    from oracle import net_oracle as no
    from oracle import torch_cpu_graph as tg
    torch.set_num_threads(min(8, os.cpu_count() or 1))       # one full-size forward per graph, on zeros (_one_thread restores it)
    for backbone, n_layers in (("mobilenet_v2", 66), ("vgg16", 35)):
        hp = helpers.hyper_params(backbone)
        specs = lg.layers(backbone, hp)
        assert len(specs) == n_layers
        names = set()
        for s in specs:
            if s["kind"] == "head":
                i = s["level"] + 1
                names |= {"%d_conv_%s_output/%s" % (i, a, b) for a in ("label", "boxes") for b in ("kernel", "bias")}
            elif s["kind"] == "l2norm":
                names.add("l2_normalization/scale")
            elif s["kind"] != "pool":
                names.add(s["name"] + ("/depthwise_kernel" if s["kind"] == "dw" else "/kernel"))
                if s["bias"]:
                    names.add(s["name"] + "/bias")
                if s["bn"]:
                    names |= {s["bn"] + "/gamma", s["bn"] + "/beta"}
        want = {n for n, _ in no.param_specs(backbone, hp) if not n.endswith(("moving_mean", "moving_variance"))}
        assert names == want
        zeros = {n: torch.zeros(shape) for n, shape in no.param_specs(backbone, hp)}
        acts = {}
        with torch.no_grad():
            no.forward(backbone, hp, zeros, np.zeros((1, 300, 300, 3), np.float32), acts, ops=tg.TorchOps)
        recorded = {n for n, v in acts.items() if getattr(v, "ndim", 0) == 4}
        touts = [s["tout"] for s in specs if s["tout"]]
        assert len(touts) == len(set(touts)) and set(touts) == recorded, set(touts) ^ recorded
        written = {"input"}
        for s in specs:
            assert s["tin"] in written and (not s.get("res") or s["res"] in written), s["name"]
            written.add(s["tout"])
        shapes = lg.tensor_shapes(specs, zeros)
        for n in recorded:
            v = acts[n]
            assert tuple(v.shape[1:]) in (shapes[n], (shapes[n][2],) + shapes[n][:2]), n      # NHWC, or the torch graph's NCHW
