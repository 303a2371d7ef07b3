"""Option ``image_f16x2``: blocks 7 - 16 of the fp32 MobileNetV2 on the whole-image kernel's two-plane fp16 form
(csrc/ssd_imgblock2.hip, NP = 2: three fp16 MFMAs per fp32 product in the expand AND the project GEMM), the block's input
scaled by 2^s from a bound of the tensor that finalize computes from the weights alone (``model.tensor_bound``).

* Oracle: every block, and block 13's expanded map, against oracle/block_oracle.py on its own input with the bar and
  norms of tests/test_block_oracle_gpu.py (5 x e32, max and RMS), table pinned to ``image 2``; the ratios of the
  split-bf16 form (``image_f16x2 0``) on the same images are printed beside them.  B = 1 (12 channel groups), 3, 24
  (uneven chunk-pair dealing) on every image; B = 232 (one group: direct epilogue with residual) on 24 images spread
  over the batch (first, last, evenly between: the one-group kernel treats every image alike, and the float64 oracle
  of 232 images is what takes the time); the gain-8 input at B = 3 (the upper clamp of every ReLU6 fires).
* Bound soundness: max |x| of blocks 6 - 15's outputs <= the static bound, at gain 1 and 8; the looseness bound / max |x|
  is printed and must stay below 2^13 (the range where the emulation of tests/test_tensor_bound_cpu.py shows no loss).
* Scale extremes: block 10's project weights x 64, x 1024 (s small / negative), x 1/8, x 1/64 (s large) and x 2^24 (the bound
  leaves the allowed range of s: blocks 11 and 12 must run the split-bf16 form, asserted through ``image_forms``).
* Option 0, determinism, neighbours: see the tests.

Measured on an MI355X (largest e_gpu / e32 over the blocks of a case; ``pytest -rA`` prints every line):

    case               fp16 pair: max  rms      split-bf16 (image_f16x2 0): max  rms
    B = 1                         0.84 0.87                                  0.86 0.90
    B = 3                         0.82 0.87                                  0.86 0.90
    B = 24                        0.94 0.86                                  1.05 0.90
    B = 232 (one group)           1.63 1.17                                  2.41 1.52
    B = 3, gain 8                 0.67 0.86                                  0.76 0.90

Static bound / max |x|: 2^2.5 .. 2^4.1 on the synthetic weights (profiles/HISTORY.md, "Whole-image blocks on the two-plane fp16 split").
"""
import numpy as np
import pytest

import helpers
from oracle import block_oracle as bo

pytestmark = pytest.mark.gpu

HIGH = list(range(7, 17))
FUSED = ["block_%d_fused" % k for k in HIGH]


def _model(B, w, f16, pin=True):
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    m.set_option("image_f16x2", f16)
    if pin:          # the image kernel's split route for every block, as test_block_oracle_gpu pins it
        m(helpers.block_test_images(1, 300))
        lines = m.get_tuning().splitlines()
        assert sorted(int(l.split("_")[1]) for l in lines if " image " in l) == HIGH
        m.set_tuning("\n".join((l.rsplit(" ", 1)[0] + " 2") if " image " in l else l for l in lines) + "\n")
    return m


def _weights():
    return helpers.synthetic_weights("mobilenet_v2", helpers.hyper_params("mobilenet_v2"))


def _records(m, x, w, blocks, images=None):
    """compare_forward on the last forward; ``images``: compare these images of the batch only."""
    import torch
    d, p = m(x)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(p).all())
    B = x.shape[0]
    fam = {l["name"]: l["config"] for l in m.layers(B) if l["flops"] > 0 and l["kind"] == "fused"}
    family = lambda k: fam.get("block_%d_fused" % k, "?")
    if images is None:
        return bo.compare_forward(m.fetch_activation, x, w, family, blocks=blocks)
    fetch = lambda name: np.ascontiguousarray(m.fetch_activation(name).reshape(B, -1)[images]).ravel()
    return bo.compare_forward(fetch, x[images], w, family, blocks=blocks)


def _within_bar(rec):
    """The bar of tests/test_block_oracle_gpu.py on one record: finite, e_gpu <= FP32_BAR x e32 in the max and RMS norm."""
    g, f32 = rec["gpu"], rec["f32"]
    if not (np.isfinite(g[0]) and np.isfinite(g[1])):
        return ["%s: non-finite" % rec["name"]]
    return ["%s: %s error %.3e > %d x e32 = %.3e" % (rec["name"], n, g[j], bo.FP32_BAR, bo.FP32_BAR * f32[j])
            for j, n in enumerate(("max", "rms")) if g[j] > bo.FP32_BAR * f32[j]]


@pytest.mark.parametrize("B,gain", [(1, 1.0), (3, 1.0), (24, 1.0), (232, 1.0), (3, 8.0)])
def test_fp16_form_vs_float64_block_oracle(B, gain):
    w = _weights()
    x = helpers.block_test_images(B, 300, gain=gain)
    images = None if B <= 24 else bo.spread(B, 24)
    cols = {}
    for f16 in (1, 0):
        m = _model(B, w, f16)
        recs = _records(m, x, w, HIGH, images)
        forms = m.image_forms(B)
        assert [forms.get(n) for n in FUSED] == [2 if f16 else 3] * len(FUSED), forms
        assert [r["family"] for r in recs] == ["image_split"] * len(recs)
        assert sorted({r["k"] for r in recs}) == HIGH and any(r["name"] == "block_13_expand_relu" for r in recs)
        cols[f16] = recs
        del m
    fails = []
    for r1, r0 in zip(cols[1], cols[0]):
        assert r1["name"] == r0["name"]
        line, f = bo.judge(r1)
        print("B=%-3d gain=%g  %s   | image_f16x2 0: e/e32 max %5.2f rms %5.2f" % (
            B, gain, line, r0["gpu"][0] / r0["f32"][0], r0["gpu"][1] / r0["f32"][1]))
        fails += f
        if gain != 1.0 and r1["is_output"] and (min(r1["sat6"]) < 0.01 or min(r1["sat0"]) < 0.10):
            fails.append("%s: the gain-%g input does not saturate its ReLU6 maps" % (r1["name"], gain))
    worst = [max(r["gpu"][j] / r["f32"][j] for r in cols[1]) for j in (0, 1)]
    worst0 = [max(r["gpu"][j] / r["f32"][j] for r in cols[0]) for j in (0, 1)]
    print("B=%-3d gain=%g  largest e/e32: fp16 pair max %.2f rms %.2f   split-bf16 max %.2f rms %.2f" % (B, gain, *worst, *worst0))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("gain", [1.0, 8.0])
def test_static_bound_holds_and_is_not_too_loose(gain):
    B = 3
    w = _weights()
    m = _model(B, w, 1, pin=False)
    m(helpers.block_test_images(B, 300, gain=gain))
    worst = 0.0
    for k in range(6, 16):
        name = bo.output_name(k)
        bound = m.tensor_bound(name)
        assert bound is not None and np.isfinite(bound) and bound > 0, name
        amax = float(np.abs(m.fetch_activation(name)).max())
        loose = bound / amax
        worst = max(worst, loose)
        print("gain=%g %-14s max|x| %9.4f  bound %10.4f  looseness 2^%.2f" % (gain, name, amax, bound, np.log2(loose)))
        assert amax <= bound, (name, amax, bound)
        assert loose < 2.0 ** 13, (name, loose)
    print("gain=%g largest looseness 2^%.2f" % (gain, np.log2(worst)))
    # tensors no project conv behind a ReLU6 depthwise writes have no bound
    assert m.tensor_bound("block_13_expand_relu") is None and m.tensor_bound("no_such_tensor") is None


@pytest.mark.parametrize("log2_scale,forms_want", [(6, [2, 2, 2]), (10, [2, 2, 2]), (-3, [2, 2, 2]), (-6, [2, 3, 2]), (24, [2, 3, 3])])
def test_scale_extremes_of_one_blocks_project_weights(log2_scale, forms_want):
    """Block 10's project weights times 2^log2_scale: its own kp follows max |w|, the bound of its output -- block 11's
    input, and through the residual block 12's -- scales with it and moves s.  x 2^24 pushes the bound past 2^27 (s < -12):
    blocks 11 and 12 keep the split-bf16 form.  x 1/64: block 11's input is bounded by 1.65 (the project shift and the
    shrunken sums), s would be 14 > 12, so block 11 keeps the split-bf16 form as well; block 12's input adds block 11's
    own interval and is back in range.  The bounds are facts of the seeded weights (He-normal, fan-in 384: 6 sum |w| / 2 ~ 100)."""
    B = 3
    w = dict(_weights())
    w["block_10_project/kernel"] = (w["block_10_project/kernel"] * np.float32(2.0 ** log2_scale)).astype(np.float32)
    x = helpers.block_test_images(B, 300)
    m = _model(B, w, 1)
    recs = _records(m, x, w, [10, 11, 12])
    forms = [m.image_forms(B).get("block_%d_fused" % k) for k in (10, 11, 12)]
    bounds = [m.tensor_bound(bo.output_name(k)) for k in (9, 10, 11)]
    print("x 2^%d: forms of blocks 10-12 %s, bounds of their inputs %s" % (log2_scale, forms, bounds))
    assert forms == forms_want, (forms, bounds)
    fails = []
    for r in recs:
        print("x 2^%-3d %s" % (log2_scale, bo.judge(r)[0]))
        fails += _within_bar(r)
    assert not fails, "\n".join(fails)


def test_option_off_runs_the_split_bf16_form_without_the_fp16_planes():
    B = 3
    w = _weights()
    x = helpers.block_test_images(B, 300)
    outs = []
    for _ in range(2):
        m = _model(B, w, 0)
        d, p = m(x)
        outs.append((d.cpu().numpy().view(np.uint32), p.cpu().numpy().view(np.uint32), m.fetch_activation("block_16_out").view(np.uint32)))
        assert m.memory_summary()["image_weight_planes"] == 0
        assert set(m.image_forms(B).get(n) for n in FUSED) == {3}
        d2, p2 = m(x)
        assert np.array_equal(d2.cpu().numpy().view(np.uint32), outs[-1][0]) and np.array_equal(p2.cpu().numpy().view(np.uint32), outs[-1][1])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_option_on_is_deterministic_and_leaves_the_neighbours_alone():
    B = 3
    w = _weights()
    x = helpers.block_test_images(B, 300)
    outs, mems = [], []
    for f16 in (1, 1, 0):
        m = _model(B, w, f16)
        d, p = m(x)
        outs.append((d.cpu().numpy().view(np.uint32), p.cpu().numpy().view(np.uint32), m.fetch_activation("block_16_out").view(np.uint32)))
        d2, p2 = m(x)
        assert np.array_equal(d2.cpu().numpy().view(np.uint32), outs[-1][0]) and np.array_equal(p2.cpu().numpy().view(np.uint32), outs[-1][1])
        cfg = {l["name"]: l["config"] for l in m.layers(B) if l["flops"] > 0}
        assert [cfg.get(n) for n in FUSED] == ["image_split"] * len(FUSED), cfg
        mems.append(m.memory_summary())
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert not np.array_equal(outs[0][2], outs[2][2])            # another rounding of the same sums: the option does switch kernels
    # the fp16 pairs of both 1x1 matrices of blocks 7 - 16: 2 planes x 2 bytes per padded weight, counted on their own
    want = 0
    for k in HIGH:
        cin, ce, cout, _, _ = bo.block_spec(k)
        want += 4 * (ce * cin + cout * ce)
    assert mems[0]["image_weight_planes"] == mems[1]["image_weight_planes"] == want, (mems[0], want)
    assert mems[2]["image_weight_planes"] == 0
    for key in ("arena", "planes", "image_slabs", "splitk_slabs"):
        assert mems[0][key] == mems[2][key], (key, mems[0], mems[2])
