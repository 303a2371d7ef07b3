"""Self-tests of the float64 conv oracle (oracle/conv_oracle.py) and of the geometry cases
(tests/conv_geometry_cases.py): no GPU.

* the oracle equals ``torch.nn.functional.conv2d`` in float64 (``F.pad`` for the four pads) within 1e-12 on every case
  (measured: 4e-15), equals the existing fp32 oracle ``net_oracle.conv2d`` within the rounding bound of an fp32 dot product,
  and gives a hand-worked answer;
* five wrong restatements -- the pads of the two axes swapped, the dilation dropped on x, the pixel decoded with ``Ho`` for
  ``Wo``, the tap decoded with ``kh`` for ``kw``, rows addressed with pitch ``H`` for ``W`` -- each differ from the right answer by
  more than 100 times the GPU bar ``1e-4 max(1, max |ref|)`` on at least one case, the pixel-decode and the row-pitch mutant on
  every case: the cases separate right from subtly wrong with two orders of magnitude to spare;
* the literal refusal table equals the one derived from the documented constraints, and every M is at most 168;
* the head helper equals ``net_oracle.heads_forward``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_geometry_cases as gc
from oracle import conv_oracle as cv
from oracle import net_oracle as no

MUTANT_FACTOR = 100.0
MUTANTS = ("swap_pads", "no_dil_x", "decode_Ho", "tap_kh", "pitch_H")
KILL_EVERY_CASE = ("decode_Ho", "pitch_H")


def gpu_bar(ref):
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def conv_flat(x, w, stride, dil, pads, mutant=None):
    """The convolution as a kernel walks it -- flat pixel index -> (oy, ox), flat tap index -> (ky, kx), flat input pixel
    iy * W + ix -- with one of the five mistakes planted.  ``mutant=None`` is a third restatement of the right answer."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    pt, pb, pl, pr = pads
    Ho = cv.out_size(H, kh, stride, dil, pt, pb)
    Wo = cv.out_size(W, kw, stride, dil, pl, pr)
    if mutant == "swap_pads":
        pt, pl = pl, pt
    dy, dx = dil, (1 if mutant == "no_dil_x" else dil)
    xf = x.reshape(B, H * W, Cin)
    out = np.zeros((B, Ho * Wo, Cout))
    for pix in range(Ho * Wo):
        oy = pix // (Ho if mutant == "decode_Ho" else Wo)
        ox = pix - oy * (Ho if mutant == "decode_Ho" else Wo)
        for t in range(kh * kw):
            ky = t // (kh if mutant == "tap_kh" else kw)
            kx = t - ky * (kh if mutant == "tap_kh" else kw)
            iy, ix = oy * stride - pt + ky * dy, ox * stride - pl + kx * dx
            if not (0 <= iy < H and 0 <= ix < W):
                continue
            lin = iy * (H if mutant == "pitch_H" else W) + ix
            if lin < H * W:         # (a wrong pitch may step past the image: a kernel would read the next image or poison)
                out[:, pix, :] += xf[:, lin, :] @ w[t // kw, t % kw]
    return out.reshape(B, Ho, Wo, Cout)


def torch_f64(x, w, stride, dil, pads):
    pt, pb, pl, pr = pads
    xt = F.pad(torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    wt = torch.from_numpy(np.asarray(w, np.float64)).permute(3, 2, 0, 1)
    return F.conv2d(xt, wt, stride=stride, dilation=dil).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_oracle_equals_torch_float64(c):
    d = gc.data(c)
    t = torch_f64(d["x"], d["w"], c.stride, c.dil, c.pads)
    assert t.shape == d["conv"].shape == (c.B,) + gc.out_hw(c) + (c.Cout,)
    err = float(np.abs(t - d["conv"]).max())
    print("%s: oracle vs torch float64 %.2e" % (c.name, err))
    assert err <= 1e-12
    np.testing.assert_allclose(conv_flat(d["x"], d["w"], c.stride, c.dil, c.pads), d["conv"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_oracle_equals_the_fp32_oracle_within_fp32_rounding(c):
    """An fp32 dot product of K terms, in any order, is within (K + 1) 2^-24 sum |x| |w| of the exact one (plus the
    rounding of the fp32 result); the bound is evaluated with the oracle itself on |x|, |w|."""
    d = gc.data(c)
    got = no.conv2d(d["x"], d["w"], None, c.stride, c.dil, c.pads).astype(np.float64)
    K = c.kh * c.kw * c.Cin
    bound = (K + 1) * 2.0 ** -24 * cv.conv2d_f64(np.abs(d["x"]), np.abs(d["w"]), c.stride, c.dil, c.pads) + 2.0 ** -24 * np.abs(d["conv"])
    assert (np.abs(got - d["conv"]) <= bound + 1e-30).all(), float(np.abs(got - d["conv"]).max())


def test_hand_worked_answer():
    """x = [[1, 2, 3], [4, 5, 6]] (one channel), a 1 x 2 kernel [10, 1], one column of padding on the LEFT only: the padded
    rows are [0, 1, 2, 3] and [0, 4, 5, 6], so the outputs are 10 a + b of neighbouring pairs.  Then the same with a 2 x 1
    kernel [[10], [1]], one row of padding at the BOTTOM, stride 2 along both axes: rows 0 and 2 of the padded map
    [[1, 2, 3], [4, 5, 6], [0, 0, 0]] start only one window (row 0), columns 0 and 2 are kept."""
    x = np.float32([[1, 2, 3], [4, 5, 6]]).reshape(1, 2, 3, 1)
    w = np.float32([10, 1]).reshape(1, 2, 1, 1)
    got = cv.conv2d_f64(x, w, 1, 1, (0, 0, 1, 0))
    np.testing.assert_array_equal(got[0, :, :, 0], [[1, 12, 23], [4, 45, 56]])
    got = cv.conv2d_f64(x, w.reshape(2, 1, 1, 1), 2, 1, (0, 1, 0, 0))
    np.testing.assert_array_equal(got[0, :, :, 0], [[14, 36]])
    # dilation 2 along x only shows with kw > 1: a 1 x 2 kernel at dilation 2 pairs columns 0 and 2
    got = cv.conv2d_f64(x, w, 1, 2, (0, 0, 0, 0))
    np.testing.assert_array_equal(got[0, :, :, 0], [[13], [46]])
    # the epilogue: * scale + shift, ReLU6, + residual
    y = cv.epilogue_f64(np.float64([[-1.0, 2.0, 5.0]]), [2.0, 2.0, 2.0], [0.5, 0.5, 0.5], cv.ACT_RELU6, [[1.0, 1.0, 1.0]])
    np.testing.assert_array_equal(y, [[1.0, 5.5, 7.0]])
    np.testing.assert_array_equal(cv.epilogue_f64(np.float64([-3.0, 7.0]), None, None, cv.ACT_RELU), [0.0, 7.0])


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_are_told_from_the_right_answer(mutant):
    killed, rows = [], []
    for c in gc.CASES:
        d = gc.data(c)
        # (against the same walk without the mistake, equal to the oracle within 1e-12 by the test above: an unchanged
        # case then differs by exactly 0, not by the summation order)
        right = conv_flat(d["x"], d["w"], c.stride, c.dil, c.pads)
        err = float(np.abs(conv_flat(d["x"], d["w"], c.stride, c.dil, c.pads, mutant) - right).max())
        bar = gpu_bar(d["conv"])
        rows.append("%s %.3g" % (c.name, err / bar))
        # a mutant either leaves a case exactly as it is or is far outside the bar: nothing in between, where a
        # verdict would hang on the seed
        assert err == 0.0 or err > MUTANT_FACTOR * bar, (mutant, c.name, err, bar)
        if err > MUTANT_FACTOR * bar:
            killed.append(c.name)
    print("%s: err / GPU bar per case: %s" % (mutant, ", ".join(rows)))
    assert killed, mutant
    if mutant in KILL_EVERY_CASE:
        assert len(killed) == len(gc.CASES), (mutant, sorted(set(c.name for c in gc.CASES) - set(killed)))


def test_refusal_table_follows_the_documented_constraints():
    assert sorted(gc.REFUSALS) == sorted(c.name for c in gc.CASES) and len(gc.CASES) == 16
    for c in gc.CASES:
        assert gc.REFUSALS[c.name] == gc.refusals_from_rules(c), c.name
        assert not gc.must_refuse(c, "auto")
        Ho, Wo = gc.out_hw(c)
        assert c.B * Ho * Wo <= 168 and Ho != Wo, c.name
    assert max(c.B * gc.out_hw(c)[0] * gc.out_hw(c)[1] for c in gc.CASES) == 168
    # the cases the families are there for: every tile family runs 13 of the 16
    for fam in gc.TILE_FAMILIES:
        assert sum(not gc.must_refuse(c, fam) for c in gc.CASES) >= 11, fam
    assert [c.name for c in gc.CASES if not gc.must_refuse(c, "wino")] == ["wide_same", "four_pads", "tiny_maps"]


def test_head_helper_equals_the_net_oracle():
    rng = np.random.default_rng(7)
    L, B = 5, 2
    hp = {"total_labels": L}
    feats, heads, P = [], [], {}
    for i, (H, W, C, A) in enumerate([(3, 4, 8, 4), (2, 2, 6, 6), (1, 1, 4, 4)], start=1):
        feats.append(rng.standard_normal((B, H, W, C)).astype(np.float32))
        wl = (rng.standard_normal((3, 3, C, A * L)) / np.sqrt(9 * C)).astype(np.float32)
        wb = (rng.standard_normal((3, 3, C, A * 4)) / np.sqrt(9 * C)).astype(np.float32)
        bl = rng.uniform(-0.5, 0.5, A * L).astype(np.float32)
        bb = rng.uniform(-0.5, 0.5, A * 4).astype(np.float32)
        heads.append((wl, bl, wb, bb))
        P["%d_conv_label_output/kernel" % i], P["%d_conv_label_output/bias" % i] = wl, bl
        P["%d_conv_boxes_output/kernel" % i], P["%d_conv_boxes_output/bias" % i] = wb, bb
    deltas, probs = cv.head_f64(feats, heads, L)
    rd, rp = no.heads_forward(hp, feats, P)
    assert deltas.shape == rd.shape == (B, 12 * 4 + 4 * 6 + 4, 4) and probs.shape == rp.shape == (B, 76, L)
    assert np.abs(deltas - rd).max() <= 1e-5 and np.abs(probs - rp).max() <= 1e-6
    np.testing.assert_allclose(probs.sum(-1), 1.0, rtol=0, atol=1e-14)
