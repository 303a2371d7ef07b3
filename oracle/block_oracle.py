"""Block-local oracle (TEST INFRASTRUCTURE, not product code): ONE MobileNetV2 inverted-residual block, or the
stem, evaluated in any NumPy float dtype on a given input.

``net_oracle`` stays the fp32 restatement of the whole graph.  This module evaluates the same formulas (same pad rules,
same BatchNorm form, same ReLU6) for a single block so that a fused block kernel can be compared with a float64
evaluation of exactly the operation it implements, on the kernel's OWN input -- nothing upstream leaks into the
comparison -- and so that the size of an honest fp32 evaluation's error (``dtype=float32``) and of a degraded one
(``operand_bits``) can be computed from the reference alone:

* ``operand_bits=16``: both operands of every matrix product (the 1x1 convolutions, Conv1) rounded to 16 significand
  bits: what an exact three-way bf16 split computes once it has lost its third plane;
* ``operand_bits=8``: both operands rounded to bf16: the definition of ``precision="bf16"``, evaluated exactly.

Depthwise taps, BatchNorm, ReLU6 and the residual add are never rounded (the kernels keep them in fp32 in every mode).

Only tests/ may import this.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

try:
    from threadpoolctl import threadpool_limits
except ImportError:
    threadpool_limits = None

from oracle.net_oracle import _MBV2_BLOCKS, BN_EPS, correct_pad, same_pads

RELU6_MAPS = (["Conv1_relu", "expanded_conv_depthwise_relu"] +
              ["block_%d_%s_relu" % (k, s) for k in range(1, 17) for s in ("expand", "depthwise")])


def block_spec(k):
    """(Cin, Cexp, Cout, stride, residual) of block k = 1 .. 16."""
    cin = 16 if k == 1 else _MBV2_BLOCKS[k - 2][0]
    cout, s = _MBV2_BLOCKS[k - 1]
    return cin, 6 * cin, cout, s, (cin == cout and s == 1)


def round_bits(a, bits):
    """float64 array rounded (nearest, ties to even) to ``bits`` significand bits, the implicit one included: 8 is bf16,
    16 the sum of two bf16 planes.  Zeros, infinities and NaN pass through (subnormals do not occur here)."""
    a = np.ascontiguousarray(a, np.float64)
    drop = 53 - int(bits)
    if drop <= 0:
        return a
    u = a.view(np.uint64)
    u = (u + (np.uint64((1 << (drop - 1)) - 1) + ((u >> np.uint64(drop)) & np.uint64(1)))) & ~np.uint64((1 << drop) - 1)
    return u.view(np.float64)


def _bn(P, name, v, dt):
    g, b, m, var = (np.asarray(P[name + "/" + s], dt) for s in ("gamma", "beta", "moving_mean", "moving_variance"))
    inv = (g / np.sqrt(var + dt(BN_EPS))).astype(dt)
    return (v * inv + (b - m * inv)).astype(dt)


def _relu6(v, dt):
    return np.minimum(np.maximum(v, dt(0)), dt(6))


def _operand(a, dt, bits):
    a = np.asarray(a, dt)
    if bits is None:
        return a
    if dt != np.float64:
        raise ValueError("operand_bits needs dtype=float64")
    return round_bits(a, bits)


def _conv1x1(x, w, dt, bits):
    """x [B,H,W,Cin] x w [1,1,Cin,Cout]: one matrix product per image (the order net_oracle.conv2d uses)."""
    B, H, W, Cin = x.shape
    wm = _operand(w, dt, bits).reshape(Cin, -1)
    xo = _operand(x, dt, bits)
    out = np.empty((B, H, W, wm.shape[1]), dt)
    for b in range(B):
        out[b] = (xo[b].reshape(H * W, Cin) @ wm).reshape(H, W, -1)
    return out


def _pad_hw(x, pads):
    pt, pb, pl, pr = pads
    return np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))


def _depthwise(x, w, stride, dt):
    """3x3 depthwise, SAME at stride 1, keras-applications ``correct_pad`` + VALID at stride 2."""
    H, W = x.shape[1], x.shape[2]
    if stride == 2:
        pads = correct_pad(H) + correct_pad(W)
    else:
        pads = same_pads(H, 3, 1)[1:] + same_pads(W, 3, 1)[1:]
    xp = _pad_hw(x, pads)
    w = np.asarray(w, dt)[..., 0]
    Ho = (xp.shape[1] - 3) // stride + 1
    Wo = (xp.shape[2] - 3) // stride + 1
    out = np.zeros((x.shape[0], Ho, Wo, x.shape[3]), dt)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :] * w[ky, kx]
    return out


def block(k, x_in, weights, dtype=np.float64, operand_bits=None):
    """Block k (1 .. 16) on ``x_in`` [B,H,W,Cin]: expand 1x1 -> BN -> ReLU6 -> depthwise 3x3 -> BN -> ReLU6 -> project
    1x1 -> BN (+ x_in where the block is residual), every operation in ``dtype``.  Returns ``(block_k_out,
    block_k_expand_relu, block_k_depthwise_relu)``."""
    dt = np.dtype(dtype).type
    cin, cexp, cout, s, res = block_spec(k)
    x = np.asarray(x_in, dt)
    assert x.ndim == 4 and x.shape[3] == cin, (k, x.shape)
    p = "block_%d_" % k
    e = _relu6(_bn(weights, p + "expand_BN", _conv1x1(x, weights[p + "expand/kernel"], dt, operand_bits), dt), dt)
    d = _depthwise(e, weights[p + "depthwise/depthwise_kernel"], s, dt)
    d = _relu6(_bn(weights, p + "depthwise_BN", d, dt), dt)
    y = _bn(weights, p + "project_BN", _conv1x1(d, weights[p + "project/kernel"], dt, operand_bits), dt)
    if res:
        y = x + y
    return y, e, d


def stem(x, weights, dtype=np.float64, operand_bits=None):
    """Conv1 (3x3, stride 2, ``correct_pad``) -> BN -> ReLU6 -> depthwise 3x3 -> BN -> ReLU6 -> project 1x1 -> BN on
    images [B,S,S,3].  Returns ``(expanded_conv_project_BN, Conv1_relu, expanded_conv_depthwise_relu)``."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dt)
    B, H, W, _ = x.shape
    xp = _pad_hw(_operand(x, dt, operand_bits), correct_pad(H) + correct_pad(W))
    Ho, Wo = (xp.shape[1] - 3) // 2 + 1, (xp.shape[2] - 3) // 2 + 1
    wm = _operand(weights["Conv1/kernel"], dt, operand_bits).reshape(27, 32)
    c1 = np.empty((B, Ho, Wo, 32), dt)
    cols = np.empty((Ho, Wo, 3, 3, 3), dt)
    for b in range(B):
        for ky in range(3):
            for kx in range(3):
                cols[:, :, ky, kx, :] = xp[b, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2, :]
        c1[b] = (cols.reshape(Ho * Wo, 27) @ wm).reshape(Ho, Wo, 32)
    c1 = _relu6(_bn(weights, "bn_Conv1", c1, dt), dt)
    d = _depthwise(c1, weights["expanded_conv_depthwise/depthwise_kernel"], 1, dt)
    d = _relu6(_bn(weights, "expanded_conv_depthwise_BN", d, dt), dt)
    y = _bn(weights, "expanded_conv_project_BN", _conv1x1(d, weights["expanded_conv_project/kernel"], dt, operand_bits), dt)
    return y, c1, d


def input_name(k):
    """Activation name of block k's input (k = 0: the stem reads the image)."""
    return None if k == 0 else "expanded_conv_project_BN" if k == 1 else "block_%d_out" % (k - 1)


def output_name(k):
    return "expanded_conv_project_BN" if k == 0 else "block_%d_out" % k


# ------------------------------------------------------------------ the comparison harness
# The bar of the fp32 and split-bf16 kernel families: e_kernel <= FP32_BAR * e32 for the max and the RMS error, where e32
# is the error of THIS module's float32 evaluation of the same block on the same input.  A correct kernel differs from
# that evaluation only by more roundings of the same size (MFMA K-chunk and channel-group summation order, FMA
# contraction, the BatchNorm scale folded into the weight copies).  The condition fixed before measuring:
# FP32_BAR * e32 <= e16 / SEPARATION for every block, e16 being the error of a two-plane split (operand_bits=16) -- a
# kernel that lost its third plane misses the bar at least four times over.  Measured (table in the docstring of
# tests/test_block_oracle_gpu.py): the largest e_kernel / e32 is 2.90 (next 2.39), the smallest e16 / e32 is 23.2, so the
# condition admits 5 and no more -- 1.7 x headroom over the largest measured ratio rather than the 2 x aimed for.
# That headroom rests on the kernels being bitwise repeatable on these inputs.  A kernel change that trips the bar (say
# another summation order of the one-group form at B = 232) is a finding to look at -- where did the roundings go? --
# not a reason to move the bar: the separation condition leaves no room above 5.
FP32_BAR = 5
SEPARATION = 4
# bf16 families: e_kernel(RMS) <= BF16_BAR * e8(RMS) (the kernel rounds the BatchNorm-folded weights, the model rounds
# the plain ones) and e_kernel(RMS) >= e16(RMS) (otherwise no bf16 kernel ran).
BF16_BAR = 2


_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=8)
    return _POOL


class ErrorSum(object):
    """Max and RMS error against a float64 reference, accumulated over chunks of images."""

    def __init__(self):
        self.max_d = self.sum_sq = self.max_ref = 0.0
        self.n = 0

    def add(self, y, ref64):
        d = np.asarray(y, np.float64) - ref64
        self.max_d = max(self.max_d, float(np.abs(d).max()))
        self.sum_sq += float(np.sum(d * d))
        self.n += d.size
        self.max_ref = max(self.max_ref, float(np.abs(ref64).max()))

    @staticmethod
    def merged(parts):
        t = ErrorSum()
        t.max_d = max(p.max_d for p in parts)
        t.max_ref = max(p.max_ref for p in parts)
        t.sum_sq = sum(p.sum_sq for p in parts)
        t.n = sum(p.n for p in parts)
        return t

    def result(self):
        return self.max_d / self.max_ref, np.sqrt(self.sum_sq / self.n) / self.max_ref


def map_sizes(S):
    """Input height (= width) of the stem (index 0) and of blocks 1 .. 16 at image size S."""
    sizes = [S, -(-S // 2)]
    for k in range(1, 16):
        sizes.append(-(-sizes[-1] // _MBV2_BLOCKS[k - 1][1]))
    return sizes


def spread(B, n=8):
    """First image, last image and n - 2 spread between."""
    return sorted(set(int(round(v)) for v in np.linspace(0, B - 1, min(n, B))))


def compare_forward(fetch, x, weights, family, inner_maps=(), with_bf16=False, chunk=4, blocks=range(0, 17)):
    """One forward against the block oracle, block by block on the forward's OWN activations.

    ``fetch(name)`` returns the flat fp32 activation ``name`` of the forward of images ``x`` [B,S,S,3]; ``family(k)``
    names the kernel that produced block k's output (k = 0: the stem).  ``inner_maps``: block indices whose ReLU6 maps
    (``*_expand_relu``, ``*_depthwise_relu``; stem: ``Conv1_relu``, ``expanded_conv_depthwise_relu``) the forward also
    wrote and that are compared too; block 13's expanded map (SSD feature map 1) always is.  Blocks 7 - 16 are compared
    on every image, the stem and blocks 1 - 6 on ``spread(B)`` (all rows of each).

    "The kernel's own input" is the producer's fp32 tensor, as ``fetch`` returns it.  The split-bf16 and bf16 consumers
    of a tensor may read the bf16 planes its producer wrote beside it instead: a producer that writes a right fp32 tensor
    but wrong planes is caught all the same, but at the CONSUMING block, one block late.

    Returns one record per compared tensor: ``{"k", "name", "family", "is_output", "gpu", "f32", "b16", "b8" (with_bf16), "sat6",
    "sat0"}``: (max, rms) errors relative to max|ref64| of the forward's tensor and of the float32 / 16-bit-operand /
    bf16-operand evaluations of the oracle on the same input, and for the two ReLU6 maps of the block the share of
    reference values equal to 6 and to 0 (``sat6`` / ``sat0``: (expand, depthwise))."""
    B, S = x.shape[0], x.shape[1]
    sizes = map_sizes(S)
    out = []
    for k in blocks:
        cin = 3 if k == 0 else block_spec(k)[0]
        H = sizes[k]
        idx = list(range(B)) if k >= 7 else spread(B)
        xin_all = x if k == 0 else fetch(input_name(k)).reshape(B, H, H, cin)
        names = [output_name(k)]
        inner = ["Conv1_relu", "expanded_conv_depthwise_relu"] if k == 0 else ["block_%d_expand_relu" % k, "block_%d_depthwise_relu" % k]
        pos = {names[0]: 0}
        if k in inner_maps:
            names += inner
            pos.update({inner[0]: 1, inner[1]: 2})
        elif k == 13:
            names.append(inner[0])
            pos[inner[0]] = 1
        got = {n: fetch(n).reshape(B, -1) for n in names}
        evals = {"f32": (np.float32, None), "b16": (np.float64, 16)}
        if with_bf16:
            evals["b8"] = (np.float64, 8)
        fn = stem if k == 0 else (lambda *a, _k=k, **kw: block(_k, *a, **kw))

        def one_chunk(ii):
            acc = {n: {e: ErrorSum() for e in ["gpu"] + list(evals)} for n in names}
            xin = xin_all[ii]
            ref = fn(xin, weights, np.float64)
            sat = np.array([[(ref[1 + j] == 6).sum(), (ref[1 + j] == 0).sum(), ref[1 + j].size] for j in (0, 1)], np.float64)
            for n in names:
                acc[n]["gpu"].add(got[n][ii].reshape(ref[pos[n]].shape), ref[pos[n]])
            for e, (dt, bits) in evals.items():
                r = fn(xin, weights, dt, operand_bits=bits)
                for n in names:
                    acc[n][e].add(r[pos[n]], ref[pos[n]])
            return acc, sat

        # the elementwise NumPy passes (depthwise taps, BatchNorm, operand rounding) release the GIL: chunks in parallel
        # -- with the BLAS held to one thread per chunk; without threadpoolctl the chunks run one after the other
        chunks = [idx[c0:c0 + chunk] for c0 in range(0, len(idx), chunk)]
        if threadpool_limits is not None and len(chunks) > 1:
            with threadpool_limits(limits=1):
                parts = list(_pool().map(one_chunk, chunks))
        else:
            parts = [one_chunk(c) for c in chunks]
        acc = {n: {e: ErrorSum.merged([a[n][e] for a, _ in parts]) for e in ["gpu"] + list(evals)} for n in names}
        sat = sum(s_ for _, s_ in parts)
        cells = sat[:, 2]
        for n in names:
            rec = {"k": k, "name": n, "family": family(k), "is_output": pos[n] == 0}
            rec.update({e: a.result() for e, a in acc[n].items()})
            rec["sat6"] = tuple(sat[:, 0] / cells)
            rec["sat0"] = tuple(sat[:, 1] / cells)
            out.append(rec)
    return out


def judge(rec):
    """(line, failures) for one record of ``compare_forward``: the fp32 bar for the fp32 / split-bf16 families, the bf16
    bar for the ``*_bf16`` families."""
    g, f32, b16 = rec["gpu"], rec["f32"], rec["b16"]
    fails = []
    what = "%s [%s]" % (rec["name"], rec["family"])
    if not (np.isfinite(g[0]) and np.isfinite(g[1])):
        return what + " non-finite output", [what + ": non-finite output"]
    if rec["family"].endswith("_bf16"):
        b8 = rec["b8"]
        line = "%-30s %-12s bf16: e/e8 max %5.2f rms %5.2f   e/e16 rms %6.1f   e8 rms %.2e" % (
            rec["name"], rec["family"], g[0] / b8[0], g[1] / b8[1], g[1] / b16[1], b8[1])
        if g[1] > BF16_BAR * b8[1]:
            fails.append("%s: rms error %.3e > %d x e8 = %.3e" % (what, g[1], BF16_BAR, BF16_BAR * b8[1]))
        if g[1] < b16[1]:
            fails.append("%s: rms error %.3e is below the two-plane split's %.3e: no bf16 kernel ran" % (what, g[1], b16[1]))
        return line, fails
    line = "%-30s %-12s e/e32 max %5.2f rms %5.2f   e16/e32 max %6.1f rms %6.1f   e32 max %.2e" % (
        rec["name"], rec["family"], g[0] / f32[0], g[1] / f32[1], b16[0] / f32[0], b16[1] / f32[1], f32[0])
    for j, norm in enumerate(("max", "rms")):
        if rec["is_output"] and FP32_BAR * f32[j] > b16[j] / SEPARATION:
            fails.append("%s: the %s bar does not separate: %d x e32 = %.3e > e16 / %d = %.3e" % (
                what, norm, FP32_BAR, FP32_BAR * f32[j], SEPARATION, b16[j] / SEPARATION))
        if g[j] > FP32_BAR * f32[j]:
            fails.append("%s: %s error %.3e > %d x e32 = %.3e (e16 = %.3e)" % (
                what, norm, g[j], FP32_BAR, FP32_BAR * f32[j], b16[j]))
    return line, fails
