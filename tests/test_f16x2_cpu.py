"""The two-plane fp16 split of the ``dmah_*`` conv tiles, restated in NumPy (tests/f16x2_cases.py): its representation
bound and the operand error of its three-product sum against the six-product bf16 form it replaces.  No GPU."""
import numpy as np

import f16x2_cases as fc


def test_representation_bound_of_the_activation_split():
    rng = np.random.default_rng(11)
    x = rng.uniform(0.0, 6.0, 4096).astype(np.float32)
    x[:8] = np.float32([0.0, -0.0, 6.0, 255.0, 1e-3, 1e-6, 2.0 ** -20, 2.0 ** -30])
    h, l = fc.split_act(x)
    back = fc.join_act(h, l).astype(np.float64)
    err = np.abs(back - x.astype(np.float64))
    bound = fc.REL * np.abs(x.astype(np.float64)) + fc.ABS
    assert (err <= bound).all(), (x[err > bound][:4], err[err > bound][:4])
    assert back[0] == 0.0 and back[1] == 0.0
    assert back[2] == 6.0 and back[3] == 255.0            # 1536 and 65280 are fp16 numbers
    # above fp16's range the split is non-finite: nothing is silently made finite
    big = fc.join_act(*fc.split_act(np.float32([256.0, 1e4, -300.0])))
    assert not np.isfinite(big).any()


def test_weight_scale_puts_the_maximum_in_range():
    for m in (1e-6, 0.02, 1.0, 300.0):
        w = np.float32([m, -m / 3, 0.0])
        k = fc.weight_exp(w)
        assert 2.0 ** 13 <= m * 2.0 ** k < 2.0 ** 14, (m, k)
        wh, wl, _ = fc.split_weights(w)
        back = (wh.astype(np.float64) + wl.astype(np.float64)) * 2.0 ** -k
        assert np.abs(back - w.astype(np.float64)).max() <= fc.REL * m
    assert fc.weight_exp(np.zeros(5, np.float32)) == 0


def test_three_product_operand_error_against_the_six_product_bf16_form():
    """K = 4608 N(0,1) data (the shape of test_split_bf16_tiles_are_as_accurate_as_the_fp32_mfma): the operand error
    (float64 accumulation) of the fp16 form is at most 1.5x that of the bf16 form."""
    rng = np.random.default_rng(31)
    B, H, Cin, Cout = 2, 19, 512, 128                  # that test's conv, as the [Cout, K] x [K, B H W] contraction it is
    xi = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32).reshape(9 * Cin, Cout).T.copy()
    xp = np.pad(xi, ((0, 0), (1, 1), (1, 1), (0, 0)))
    x = np.concatenate([xp[:, ky:ky + H, kx:kx + H, :].reshape(B * H * H, Cin) for ky in range(3) for kx in range(3)], 1).T.copy()
    ref = w.astype(np.float64) @ x.astype(np.float64)
    e_h = np.abs(fc.matmul_f16x2(w, x) - ref).max()
    e_b = np.abs(fc.matmul_bf16x3(w, x) - ref).max()
    print("operand error: f16x2 %.3g, bf16x3 %.3g" % (e_h, e_b))
    assert e_h <= 1.5 * e_b, (e_h, e_b)
