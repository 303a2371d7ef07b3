"""NumPy restatements for the static tensor bounds and the two number formats of the whole-image block kernel's
two-plane fp16 form (option ``image_f16x2``): the interval of a project conv's output from its weights, the exponent of
the input scale, and the operand error of the three-product fp16 form beside the six-product bf16 form.  No GPU."""
import itertools

import numpy as np

import f16x2_cases as fc


def interval(w, scale=None, shift=None, res=None):
    """Rows of ``w`` [n, k] are output channels: (lo, hi) [n] of ``w' d + shift (+ r)`` over d in [0, 6]^k, r in ``res`` =
    (lo, hi); w' = fl32(w * scale[:, None]), sums in float64 -- what ``ssd_block_output_interval`` computes."""
    w = np.asarray(w, np.float32)
    if scale is not None:
        w = (w * np.asarray(scale, np.float32)[:, None]).astype(np.float32)
    w = w.astype(np.float64)
    h = np.zeros(w.shape[0]) if shift is None else np.asarray(shift, np.float32).astype(np.float64)
    lo = 6.0 * np.minimum(w, 0).sum(1) + h
    hi = 6.0 * np.maximum(w, 0).sum(1) + h
    if res is not None:
        lo, hi = lo + res[0], hi + res[1]
    return lo, hi


def corner_extremes(w, scale=None, shift=None):
    """The same by brute force: min and max of ``w' d + shift`` over the 2^k corners d in {0, 6}^k (a linear function on
    a box takes its extremes at corners), float64."""
    w = np.asarray(w, np.float32)
    if scale is not None:
        w = (w * np.asarray(scale, np.float32)[:, None]).astype(np.float32)
    w = w.astype(np.float64)
    h = np.zeros(w.shape[0]) if shift is None else np.asarray(shift, np.float32).astype(np.float64)
    corners = np.array(list(itertools.product((0.0, 6.0), repeat=w.shape[1])))          # [2^k, k]
    y = corners @ w.T + h
    return y.min(0), y.max(0), corners


def input_exp(bound):
    """s = floor(log2(2^15 / bound)) or None where the form is refused (unknown, zero or non-finite bound, |s| > 12)."""
    if bound is None or not np.isfinite(bound) or not bound > 0:
        return None
    f, e = np.frexp(np.float32(bound))
    s = int(16 - e if f == 0.5 else 15 - e)
    return s if -12 <= s <= 12 else None


def matmul_f16x2_scaled(w, x, s):
    """The expand GEMM of the fp16 form: w [n, k] as the pair of 2^ke w, x [k, m] as the pair of 2^s x, three products
    (lh, hl, hh) formed exactly, summed in float64, scaled back -- the OPERAND error of the form, no accumulation error."""
    wh, wl, k = fc.split_weights(w)
    xs = (np.asarray(x, np.float32) * np.float32(2.0 ** s)).astype(np.float32)
    xh = xs.astype(np.float16)
    xl = (xs - xh.astype(np.float32)).astype(np.float16)
    wh, wl, xh, xl = (a.astype(np.float64) for a in (wh, wl, xh, xl))
    return (wl @ xh + wh @ xl + wh @ xh) * 2.0 ** -(s + k)
