"""The static tensor bounds behind option ``image_f16x2`` (``ssd_block_output_interval``, ``ssd_f16x2_input_exp``: host
arithmetic of the library, no device) against brute force over the corners of the input box and against their NumPy
restatement (tests/tensor_bound_cases.py), and the operand error of the fp16 form of the expand GEMM under a loose
bound.  No GPU."""
import ctypes

import numpy as np
import pytest

import ssd_hip
import tensor_bound_cases as tb
import f16x2_cases as fc

_dp = ctypes.POINTER(ctypes.c_double)


def _lib_interval(w, scale=None, shift=None, res=None, ld=None):
    """``ssd_block_output_interval`` on a row-major [n, ld] copy of ``w`` (columns past k poisoned: they must not be read)."""
    w = np.asarray(w, np.float32)
    n, k = w.shape
    ld = ld or k + 3
    buf = np.full((n, ld), np.nan, np.float32)
    buf[:, :k] = w
    fp = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(ssd_hip.c_float_p)
    keep = [np.ascontiguousarray(a, np.float64) for a in (res or ())]
    lo, hi = np.empty(n), np.empty(n)
    rc = ssd_hip.lib().ssd_block_output_interval(buf.ctypes.data_as(ssd_hip.c_float_p), n, k, ld, fp(scale), fp(shift),
                                                 keep[0].ctypes.data_as(_dp) if keep else None,
                                                 keep[1].ctypes.data_as(_dp) if keep else None,
                                                 lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp))
    return rc, lo, hi


def _block(rng, n, k):
    w = (rng.standard_normal((n, k)) * np.sqrt(2.0 / k)).astype(np.float32)
    w[0] = np.abs(w[0])                      # an all-positive row, an all-negative row, a zero row
    w[1] = -np.abs(w[1])
    w[2] = 0.0
    return w, rng.uniform(0.5, 1.5, n).astype(np.float32), rng.uniform(-0.3, 0.3, n).astype(np.float32)


def test_interval_is_the_extreme_over_the_corners_of_the_input_box():
    rng = np.random.default_rng(5)
    w, scale, shift = _block(rng, 7, 10)
    rc, lo, hi = _lib_interval(w, scale, shift)
    assert rc == 1
    cmin, cmax, corners = tb.corner_extremes(w, scale, shift)
    # the interval is ATTAINED (it is the tightest box, not merely a bound), up to the order of the float64 sums
    tol = 1e-12 * (np.abs(w).sum(1) * 6 + 1)
    assert (np.abs(lo - cmin) <= tol).all() and (np.abs(hi - cmax) <= tol).all(), (lo - cmin, hi - cmax)
    # ... and holds for interior points of [0, 6]^k
    d = rng.uniform(0, 6, (4096, 10))
    y = d @ (w * scale[:, None]).astype(np.float32).astype(np.float64).T + shift.astype(np.float64)
    assert (y >= lo - tol).all() and (y <= hi + tol).all()
    nlo, nhi = tb.interval(w, scale, shift)
    assert np.allclose(lo, nlo, rtol=0, atol=tol) and np.allclose(hi, nhi, rtol=0, atol=tol)
    assert lo[2] == hi[2] == float(shift[2])           # the zero row: the shift alone


def test_residual_chains_add_their_intervals():
    """Four blocks, as the longest chain of the net (blocks 7 - 10 without the last: x7, x8 = x7 + f8, x9 = x8 + f9, ...):
    the bound of the last tensor against brute force over the corners of EVERY block's own depthwise box."""
    rng = np.random.default_rng(6)
    n, k = 5, 6
    blocks = [_block(rng, n, k) for _ in range(4)]
    res, brute_lo, brute_hi = None, np.zeros(n), np.zeros(n)
    for w, scale, shift in blocks:
        rc, lo, hi = _lib_interval(w, scale, shift, res=res)
        assert rc == 1
        res = (lo, hi)
        cmin, cmax, _ = tb.corner_extremes(w, scale, shift)       # the depthwise outputs of different blocks vary independently
        brute_lo, brute_hi = brute_lo + cmin, brute_hi + cmax
    assert np.allclose(res[0], brute_lo, rtol=0, atol=1e-10) and np.allclose(res[1], brute_hi, rtol=0, atol=1e-10)
    # the intervals ADD: no product of per-block bounds (a ReLU6 sits inside every block)
    widths = sum(6.0 * np.abs((w * s[:, None]).astype(np.float32).astype(np.float64)).sum(1) for w, s, _ in blocks)
    assert np.allclose(res[1] - res[0], widths, rtol=1e-12)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_inputs_leave_no_bound(bad):
    rng = np.random.default_rng(7)
    w, scale, shift = _block(rng, 4, 8)
    for where in ("w", "scale", "shift", "res"):
        a, s, h, res = w.copy(), scale.copy(), shift.copy(), (np.zeros(4), np.ones(4))
        if where == "w":
            a[3, 5] = bad
        elif where == "scale":
            s[1] = bad
        elif where == "shift":
            h[0] = bad
        else:
            res = (np.zeros(4), np.array([1.0, bad, 1.0, 1.0]))
        rc, _, _ = _lib_interval(a, s, h, res=res)
        assert rc == 0, where
    big = np.full((2, 8), 3e38, np.float32)                       # finite weights whose folded product overflows fp32
    assert _lib_interval(big, np.float32([2.0, 2.0]), None)[0] == 0


def test_input_exponent_keeps_the_scaled_bound_inside_fp16():
    lib = ssd_hip.lib()
    s = ctypes.c_int(99)
    for bound in [2.0 ** e for e in range(-2, 28)] + [3.0, 6.0, 65.9, 66.0, 1000.0, 32768.0, 32769.0, 1.5 * 2 ** 27, 7.99]:
        ok = lib.ssd_f16x2_input_exp(ctypes.c_float(bound), ctypes.byref(s))
        want = tb.input_exp(bound)
        assert (s.value if ok else None) == want, (bound, ok, s.value, want)
        exact = int(np.floor(np.log2(2.0 ** 15 / bound)))
        assert want == (exact if -12 <= exact <= 12 else None), (bound, want, exact)
        if ok:
            assert 2.0 ** 14 < bound * 2.0 ** s.value <= 2.0 ** 15 < 65504
    for bound in (-1.0, 0.0, np.inf, np.nan, 2.0 ** 28, 2.0 ** -3 * 0.99):
        assert lib.ssd_f16x2_input_exp(ctypes.c_float(bound), ctypes.byref(s)) == 0 and s.value == 0, bound


@pytest.mark.parametrize("K", [64, 96, 160])
@pytest.mark.parametrize("log2_loose", [0, 5, 13])
def test_operand_error_of_the_fp16_expand_under_a_loose_bound(K, log2_loose):
    """x is a linear bottleneck output (signed, no ReLU6 in front) whose static bound is 2^log2_loose times its real
    maximum.  Each operand of the pair is within 2^-22 relative (11 + 11 bits) plus half a step of fp16's subnormal grid
    (2^-25 in scaled units); the dropped low x low product is <= 2^-22 |w x|.  With 2^s bound in (2^14, 2^15] and
    2^k max|w| in [2^13, 2^14) that is, per output,

        |err| <= 3 x 2^-22 sum |w||x|  +  2^-39 bound sum |w|  +  2^-38 max|w| sum |x|."""
    rng = np.random.default_rng(100 + K + log2_loose)
    w = (rng.standard_normal((6 * K, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    x = (rng.standard_normal((K, 361)) * 3.0).astype(np.float32)
    bound = float(np.abs(x).max()) * 2.0 ** log2_loose
    s = tb.input_exp(bound)
    assert s is not None
    ref = w.astype(np.float64) @ x.astype(np.float64)
    err = np.abs(tb.matmul_f16x2_scaled(w, x, s) - ref)
    aw, ax = np.abs(w.astype(np.float64)), np.abs(x.astype(np.float64))
    lim = 3 * 2.0 ** -22 * (aw @ ax) + 2.0 ** -39 * bound * aw.sum(1)[:, None] + 2.0 ** -38 * aw.max() * ax.sum(0)[None, :]
    e6 = np.abs(fc.matmul_bf16x3(w, x) - ref)
    print("K=%d loose 2^%d s=%d: operand error / max|ref|  fp16 pair max %.3g rms %.3g   six bf16 max %.3g rms %.3g" % (
        K, log2_loose, s, err.max() / np.abs(ref).max(), np.sqrt((err ** 2).mean()) / np.abs(ref).max(),
        e6.max() / np.abs(ref).max(), np.sqrt((e6 ** 2).mean()) / np.abs(ref).max()))
    assert (err <= lim).all(), float((err / lim).max())
