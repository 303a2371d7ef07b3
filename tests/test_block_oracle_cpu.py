"""CPU self-tests of the block-local oracle (oracle/block_oracle.py) and of the comparison harness the GPU test
(tests/test_block_oracle_gpu.py) is built on: the oracle restates net_oracle block by block, the bar separates an fp32
evaluation from a two-plane split on the GPU test's inputs, the gain-8 inputs saturate every ReLU6, and the harness
flags a block whose matrix operands lost their third bf16 plane -- or whose upper clamp is wrong -- at that block only."""
import numpy as np
import pytest

import helpers
from oracle import block_oracle as bo
from oracle import net_oracle as no


def _setup(S, B, gain=1.0):
    hp = helpers.hyper_params("mobilenet_v2")
    if S == 512:
        hp["img_size"] = 512
        hp["feature_map_shapes"] = [32, 16, 8, 4, 2, 1]
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.block_test_images(B, S, gain=gain)
    acts = {}
    no.forward("mobilenet_v2", hp, w, x, acts)
    return w, x, acts


_CACHE = {}


def _records(S, B, gain=1.0):
    """The harness run on net_oracle's own activations (the fp32 NumPy forward stands in for the GPU)."""
    key = (S, B, gain)
    if key not in _CACHE:
        w, x, acts = _setup(S, B, gain)
        recs = bo.compare_forward(lambda n: acts[n].reshape(-1), x, w, lambda k: "numpy", inner_maps=range(0, 17), with_bf16=True)
        _CACHE[key] = (w, x, acts, recs)
    return _CACHE[key]


def test_round_bits():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -3.1415926535, 0.0, 1e-3, 255.5, 256.5])
    r8 = bo.round_bits(a, 8)
    # ties to even at 8 significand bits: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    np.testing.assert_array_equal(r8[:4], [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7])
    np.testing.assert_array_equal(r8[7:], [256.0, 256.0])
    import torch
    t = torch.from_numpy(a.astype(np.float32))
    np.testing.assert_array_equal(r8.astype(np.float32), t.to(torch.bfloat16).to(torch.float32).numpy())
    for bits in (8, 12, 16, 24):
        r = bo.round_bits(a, bits)
        nz = a != 0
        assert (np.abs(r[nz] / a[nz] - 1) <= 2.0 ** -bits).all()
        np.testing.assert_array_equal(bo.round_bits(r, bits), r)
    np.testing.assert_array_equal(bo.round_bits(a.astype(np.float32).astype(np.float64), 24), a.astype(np.float32))


@pytest.mark.parametrize("S,B", [(300, 2), (512, 1)])
def test_float32_blocks_restate_net_oracle(S, B):
    """block(k, ., float32) on net_oracle's block input IS net_oracle's block: every output and every ReLU6 map, stem
    included: the formulas and the per-image matrix products are the same, so the tensors are equal bit for bit."""
    w, x, acts, recs = _records(S, B)
    assert [r["name"] for r in recs if r["is_output"]] == [bo.output_name(k) for k in range(17)]
    assert sorted(r["name"] for r in recs if not r["is_output"]) == sorted(bo.RELU6_MAPS)
    for r in recs:
        # the stand-in differs from float64 exactly as the float32 evaluation does
        assert abs(r["gpu"][0] - r["f32"][0]) <= 1e-7 * r["f32"][0] + 1e-12, r
    y, c1, d = bo.stem(x, w, np.float32)
    for got, name in ((y, "expanded_conv_project_BN"), (c1, "Conv1_relu"), (d, "expanded_conv_depthwise_relu")):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, acts[name], err_msg=name)
    for k in range(1, 17):
        y, e, d = bo.block(k, acts[bo.input_name(k)], w, np.float32)
        assert y.dtype == e.dtype == d.dtype == np.float32
        for got, name in ((y, "block_%d_out" % k), (e, "block_%d_expand_relu" % k), (d, "block_%d_depthwise_relu" % k)):
            np.testing.assert_array_equal(got, acts[name], err_msg=name)


def test_the_gpu_cases_name_every_family():
    """Each case of tests/test_block_oracle_gpu.py asserts through ``m.layers(B)`` that its routing reached the families
    it names; together the cases name them all, the headline families at every batch size of the list, at both image
    sizes (no GPU needed: the case table is plain data; the GPU file also collects the config strings that really ran)."""
    import test_block_oracle_gpu as g
    named = {}
    for p in g.CASES:
        c = p.values[0]
        for fam, ks in c["reaches"].items():
            assert ks
            named.setdefault(fam, set()).add((c["S"], c["B"]))
    assert set(named) == g.FP32_FAMILIES | g.BF16_FAMILIES, sorted(named)
    for fam in ("stem_split", "band", "band3", "image", "image_split"):
        assert {B for S, B in named[fam] if S == 300} >= {1, 5, 24, 64, 232}, (fam, named[fam])
    assert {(p.values[0]["S"], p.values[0]["B"]) for p in g.CASES} >= {(300, 1), (300, 5), (300, 24), (300, 64), (300, 232), (512, 1), (512, 16)}
    assert len({p.id for p in g.CASES}) == len(g.CASES)


@pytest.mark.parametrize("S,B,gain", [(300, 2, 1.0), (300, 2, 8.0), (512, 1, 1.0)])
def test_the_bar_separates_fp32_from_a_two_plane_split(S, B, gain):
    """FP32_BAR x e32 <= e16 / SEPARATION at every block (max and RMS), on the GPU test's inputs; the bf16 yardstick sits
    two orders above."""
    recs = _records(S, B, gain)[3]
    for r in recs:
        if not r["is_output"]:
            continue
        line, fails = bo.judge(r)
        assert not fails, fails
        for j in (0, 1):
            assert 2e-8 <= r["f32"][j] <= 1e-6
            assert bo.FP32_BAR * r["f32"][j] <= r["b16"][j] / bo.SEPARATION, (r["name"], r["f32"], r["b16"])
            assert r["b8"][j] >= 100 * r["b16"][j]
        assert 1e-4 <= r["b8"][1] <= 2e-3 and 1e-3 <= r["b8"][0] <= 1e-2, r["b8"]


def test_gain_8_saturates_every_relu6():
    """At gain 8 every ReLU6 map of the stem and of blocks 1 - 16 holds >= 1 % sixes and >= 10 % zeros; at gain 1 the
    stem and blocks 1 - 2 hold (almost) no sixes -- which is why the gain-8 case exists."""
    recs = [r for r in _records(300, 2, 8.0)[3] if r["is_output"]]
    assert len(recs) == 17
    for r in recs:
        assert min(r["sat6"]) >= 0.01 and min(r["sat0"]) >= 0.10, (r["name"], r["sat6"], r["sat0"])
    plain = [r for r in _records(300, 2, 1.0)[3] if r["is_output"]]
    assert all(max(r["sat6"]) < 0.0005 for r in plain[:3])


def test_harness_flags_a_degraded_block_and_only_that_block():
    """A forward whose block 9 multiplies 16-bit operands (a split that lost its third plane), whose block 2 clamps at
    6.5 and whose stem drops a pad column is caught at blocks 9, 2 and 0 -- each downstream block is judged on the
    degraded forward's own activations and passes."""
    w, x, acts, _ = _records(300, 2, 8.0)
    bad = {}
    y = bo.stem(x, w, np.float32)[0]
    y[:, :, -1, :] = bo.stem(np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 0)), constant_values=0.5)[:, :, 1:, :], w, np.float32)[0][:, :, -1, :]
    bad[bo.output_name(0)] = y
    for k in range(1, 17):
        if k == 9:
            y = bo.block(k, y, w, np.float64, operand_bits=16)[0].astype(np.float32)
        elif k == 2:
            p = "block_2_"
            e = bo._conv1x1(y, w[p + "expand/kernel"], np.float32, None)
            e = np.minimum(np.maximum(bo._bn(w, p + "expand_BN", e, np.float32), 0), np.float32(6.5))
            d = bo._relu6(bo._bn(w, p + "depthwise_BN", bo._depthwise(e, w[p + "depthwise/depthwise_kernel"], 1, np.float32), np.float32), np.float32)
            y = y + bo._bn(w, p + "project_BN", bo._conv1x1(d, w[p + "project/kernel"], np.float32, None), np.float32)
        else:
            y = bo.block(k, y, w, np.float32)[0]
        bad[bo.output_name(k)] = y
    bad["block_13_expand_relu"] = bo.block(13, bad["block_12_out"], w, np.float32)[1]
    recs = bo.compare_forward(lambda n: bad[n].reshape(-1), x, w, lambda k: "numpy")
    failed = sorted({r["k"] for r in recs if bo.judge(r)[1]})
    assert failed == [0, 2, 9], failed
    # the two-plane block sits where the issue measured it: 1e-5 of max|y|, under the 2e-5 bar of the chained tests
    r9 = [r for r in recs if r["k"] == 9][0]
    assert 5e-6 <= r9["gpu"][0] <= 2.5e-5


def test_bf16_judgement_has_a_ceiling_and_a_floor():
    w, x, acts, _ = _records(300, 2, 1.0)
    k = 7
    xin = acts[bo.input_name(k)]
    for out, ok in ((bo.block(k, xin, w, np.float64, operand_bits=8)[0], True),
                    (bo.block(k, xin, w, np.float32)[0], False),                         # an fp32 kernel in a bf16 routing
                    (bo.block(k, xin, w, np.float64, operand_bits=6)[0], False)):        # a kernel that rounds twice over
        recs = bo.compare_forward(lambda n: (out if n == bo.output_name(k) else acts[n]).reshape(-1), x, w,
                                  lambda k: "image_bf16", with_bf16=True, blocks=[k])
        assert bool(bo.judge(recs[0])[1]) != ok, bo.judge(recs[0])
