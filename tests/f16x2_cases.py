"""NumPy restatement of the two-plane fp16 split ("f16x2", tf-ssd_amd/csrc/ssd_bf16x3.h) and of the exact three-way bf16
split it stands beside: the oracle of tests/test_f16x2_cpu.py and tests/test_f16x2_gpu.py.

Activations: s = 256 x (exact), h = fp16(s), l = fp16(s - h), both to nearest even (NumPy's float32 -> float16 cast);
weights: the same pair of 2^k w with one k per layer, max |w| 2^k in [2^13, 2^14).  A product is wl xh + wh xl + wh xh
(wl xl dropped) times the exact 2^-(8 + k)."""
import numpy as np

ACT_SCALE = np.float32(256.0)
# |join(split(x)) - x| <= REL |x| + ABS for |x| <= 255: h carries 11 significand bits, l 11 more (2^-22 relative in all) or,
# where it is subnormal, fp16's grid of 2^-24 (half a step = 2^-25, over the scale 2^8: 2^-33)
REL, ABS = 2.0 ** -22, 2.0 ** -33


def split_h(s):
    """fp32 array (already scaled) -> the fp16 pair (h, l)."""
    s = np.asarray(s, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = s.astype(np.float16)
        l = (s - h.astype(np.float32)).astype(np.float16)
    return h, l


def split_act(x):
    return split_h(np.asarray(x, np.float32) * ACT_SCALE)


def join_act(h, l):
    with np.errstate(invalid="ignore"):
        return (h.astype(np.float32) + l.astype(np.float32)) * np.float32(1.0 / 256.0)


def weight_exp(w):
    """k with max |w| 2^k in [2^13, 2^14); 0 for all-zero weights."""
    m = float(np.abs(np.asarray(w, np.float32)).max()) if np.size(w) else 0.0
    if not m > 0.0:
        return 0
    return 14 - int(np.frexp(np.float32(m))[1])


def split_weights(w, k=None):
    k = weight_exp(w) if k is None else k
    h, l = split_h(np.ldexp(np.asarray(w, np.float32), k))
    return h, l, k


def split_bf16x3(x):
    """The exact three-way bf16 split x = h + m + l by truncation (split1), as float32 arrays."""
    x = np.asarray(x, np.float32)
    h = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r1 = x - h
    m = (r1.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r2 = r1 - m
    l = (r2.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    return h, m, l


def matmul_f16x2(w, x):
    """[N, K] x [K, M] through the three-product form with float64 accumulation: the OPERAND error of the form."""
    wh, wl, k = split_weights(w)
    xh, xl = split_act(x)
    f = lambda a: a.astype(np.float64)
    return (f(wl) @ f(xh) + f(wh) @ f(xl) + f(wh) @ f(xh)) * 2.0 ** -(8 + k)


def matmul_bf16x3(w, x):
    """The six-product form of the three-way bf16 split (mma6), float64 accumulation."""
    wh, wm, wl = [a.astype(np.float64) for a in split_bf16x3(w)]
    xh, xm, xl = [a.astype(np.float64) for a in split_bf16x3(x)]
    return wm @ xm + wh @ xl + wl @ xh + wh @ xm + wm @ xh + wh @ xh
