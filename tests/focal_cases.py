"""Cases and oracle for the focal confidence loss (csrc/ssd_focal.hip, ``ssd_loss.FocalLoss``); needs no GPU.

The formula is Keras' ``CategoricalFocalCrossentropy(alpha, gamma)`` on probabilities (include/ssd_hip.h states it):
``s = sum q``, ``r = clip(q / s, 1e-7, 1 - 1e-7)``, ``f = sum_c alpha (1 - r_c)^gamma (-y_c log r_c)``; per image the sum of
``f`` over ALL anchors divided by the positive count (1 when there is none).  The oracle is NumPy: ``r`` is formed in
float32 (sum in class order, one division, the clip), as Keras and the kernel form it, everything after it in float64.
The gradients come from a torch-CPU float64 autograd graph of the same formula, then through the softmax's Jacobian at
the given probabilities (``dz = p (dp - sum p dp)``): the gradient w.r.t. the LOGITS of a model whose softmax gave ``q``.
The clip passes the gradient exactly where the float32 ``q / s`` lies inside ``[1e-7, 1 - 1e-7]``, bounds included.
"""
import collections

import numpy as np

from oracle import loss_oracle as lo

F32 = np.float32
EPS = F32(1e-7)
ONE_M_EPS = F32(1) - EPS
TILE_L21 = 256          # ssd_focal_loss_tile(21): anchors per workgroup (tests/test_focal_cpu.py holds the library to it)
STAGED_MAX_L = 119      # rows up to this many floats go through LDS, longer ones are read directly


def softmax32(z):
    z = np.asarray(z, F32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=F32)).astype(F32)


def ratio32(q):
    """float32 ``q / s`` with ``s`` added in class order (what the kernel and oracle/loss_oracle.cross_entropy do)."""
    q = np.asarray(q, F32)
    s = q[..., 0].copy()
    for c in range(1, q.shape[-1]):
        s = s + q[..., c]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (q / s[..., None]).astype(F32)


def per_anchor(y, q, alpha, gamma):
    """[..., L] -> [...] float64 focal value."""
    r = np.clip(ratio32(q), EPS, ONE_M_EPS).astype(np.float64)
    y = np.asarray(y, np.float64)
    mod = np.ones_like(r) if gamma == 0 else (1.0 - r) ** float(gamma)
    return (float(alpha) * mod * (-(y * np.log(r)))).sum(-1)


def positives(y):
    return np.any(np.asarray(y)[..., 1:] != 0, axis=-1)


def conf_loss(y, q, alpha, gamma):
    """[B,N,L] -> [B] float64."""
    pos = positives(y).sum(-1).astype(np.float64)
    return per_anchor(y, q, alpha, gamma).sum(-1) / np.where(pos == 0, 1.0, pos)


def torch_loss_and_grads(yd, yl, pd, q, loc_loss_alpha, alpha, gamma, grad_scale=None, r_float32=True):
    """float64 autograd -> (loc [B], conf [B], d/d pred_deltas, d/d logits) of ``grad_scale * sum_b (loc_b + conf_b)``
    (``grad_scale`` None: 1 / B, the Keras batch mean).  ``r_float32=False``: the value of ``r`` is the float64 ratio too
    (for finite differences, which float32 steps would drown)."""
    import torch
    f64 = torch.float64
    yd_t, yl_t = torch.as_tensor(np.asarray(yd, np.float64)), torch.as_tensor(np.asarray(yl, np.float64))
    pd_t = torch.as_tensor(np.asarray(pd, np.float64)).requires_grad_(True)
    q_t = torch.as_tensor(np.asarray(q, np.float64)).requires_grad_(True)
    B = q_t.shape[0]
    gs = 1.0 / B if grad_scale is None else float(grad_scale)
    err = pd_t - yd_t
    a = err.abs()
    h = torch.minimum(a, torch.tensor(1.0, dtype=f64))
    hub = (0.5 * h * h + (a - h)).sum(-1)
    lpos = (yd_t != 0).any(-1).to(f64)
    ltp = lpos.sum(1)
    loc = (lpos * hub).sum(-1) / torch.where(ltp == 0, torch.ones_like(ltp), ltp) * float(loc_loss_alpha)
    r64 = q_t / q_t.sum(-1, keepdim=True)
    if r_float32:
        r32 = ratio32(q)
        inside = torch.as_tensor((r32 >= EPS) & (r32 <= ONE_M_EPS))
        value = torch.as_tensor(np.clip(r32, EPS, ONE_M_EPS).astype(np.float64))
        r = torch.where(inside, r64 + (value - r64).detach(), value)
    else:
        r = torch.clamp(r64, float(EPS), float(ONE_M_EPS))
    mod = torch.ones_like(r) if gamma == 0 else (1.0 - r) ** float(gamma)
    f = (float(alpha) * mod * (-(yl_t * torch.log(r)))).sum(-1)
    cpos = torch.as_tensor(positives(yl).sum(-1).astype(np.float64))
    conf = f.sum(-1) / torch.where(cpos == 0, torch.ones_like(cpos), cpos)
    (gs * (loc + conf).sum()).backward()
    gq = q_t.grad
    p = q_t.detach()
    gz = p * (gq - (p * gq).sum(-1, keepdim=True))
    return loc.detach().numpy(), conf.detach().numpy(), pd_t.grad.numpy(), gz.numpy()


def objective_from_logits(z, yl, alpha, gamma):
    """float64 all the way: mean_b conf_b of softmax(z) (the function the finite differences step)."""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    r = np.clip(p / p.sum(-1, keepdims=True), float(EPS), float(ONE_M_EPS))
    f = (float(alpha) * (1.0 - r) ** float(gamma) * (-(np.asarray(yl, np.float64) * np.log(r)))).sum(-1)
    pos = positives(yl).sum(-1).astype(np.float64)
    return float((f.sum(-1) / np.where(pos == 0, 1.0, pos)).mean())


Case = collections.namedtuple("Case", "name yd yl pd pp alpha gamma loc_alpha marks")


def _base(seed, B, N, L, pos_fraction):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((B, N, L)) * 2).astype(F32)
    pos = rng.random((B, N)) < pos_fraction
    cls = rng.integers(1, L, (B, N))
    yl = np.zeros((B, N, L), F32)
    yl[..., 0] = 1
    bi, ni = np.nonzero(pos)
    yl[bi, ni, 0] = 0
    yl[bi, ni, cls[bi, ni]] = 1
    yd = np.zeros((B, N, 4), F32)
    yd[bi, ni] = (rng.standard_normal((len(bi), 4)) * 2).astype(F32)
    pd = (rng.standard_normal((B, N, 4)) * 1.5).astype(F32)
    return rng, yd, yl, pd, softmax32(z)


def _tiny():
    """(1, 1, 2): one positive anchor; gamma 0, alpha 1 is the plain cross-entropy."""
    _, yd, yl, pd, pp = _base(11, 1, 1, 2, 2.0)
    return Case("tiny", yd, yl, pd, pp, 1.0, 0.0, 1.0, {})


def _small():
    """(2, 70, 3): image 0 has no positive (denominator 1), in image 1 every anchor is one; in image 1 the true-class
    probability of anchor 0 is exactly 0, of anchor 1 exactly 1 (both clip bounds: the gradient row is 0) and of anchor 2
    exactly 1e-7f (inside: the gradient passes)."""
    rng, yd, yl, pd, pp = _base(12, 2, 70, 3, 0.0)
    cls = rng.integers(1, 3, 70)
    yl[1] = 0
    yl[1, np.arange(70), cls] = 1
    yd[1] = (rng.standard_normal((70, 4)) * 2).astype(F32)
    yd[1, 5] = [0, 0, 1.5, 0]                                   # positive through one coordinate
    yl[1, :3] = [0, 1, 0]
    pp[1, 0] = [0.5, 0.0, 0.5]
    pp[1, 1] = [0.0, 1.0, 0.0]
    pp[1, 2] = [0.5, EPS, F32(0.5) - F32(2.0 ** -23)]           # 0.5 + 1e-7f rounds to 0.5 + 2^-23: the sum is exactly 1
    r = ratio32(pp[1, :3])[:, 1]
    assert r[0] == 0 and r[1] == 1 and r[2] == EPS and r[2].dtype == F32
    assert not positives(yl[0]).any() and positives(yl[1]).all()
    return Case("small", yd, yl, pd, pp, 1.0, 0.5, 1.0, {"below": (1, 0), "above": (1, 1), "at_bound": (1, 2)})


def _tile_plus_one():
    """(3, T + 1, 21): one anchor spills into a second tile; rows that do not sum to 1 (scaled by 0.5 .. 2) and smoothed,
    not one-hot, targets in image 2."""
    rng, yd, yl, pd, pp = _base(13, 3, TILE_L21 + 1, 21, 0.08)
    pp = (pp * (0.5 + 1.5 * rng.random(pp.shape[:2] + (1,))).astype(F32)).astype(F32)
    assert np.abs(pp.sum(-1) - 1).max() > 0.4
    yl[2] = (F32(0.9) * yl[2] + F32(0.1 / 21)).astype(F32)      # smoothed: every class counts, every anchor is "positive"
    return Case("tile_plus_one", yd, yl, pd, pp, 0.25, 2.0, 1.0, {"smoothed_image": 2})


def _two_tiles_plus_one():
    """(2, 2T + 1, 21): three tiles per image, B a power of two (the grad_scale property)."""
    _, yd, yl, pd, pp = _base(14, 2, 2 * TILE_L21 + 1, 21, 0.05)
    return Case("two_tiles_plus_one", yd, yl, pd, pp, 0.25, 5.0, 1.5, {})


def _long_rows():
    """L above the LDS-tile limit, N = 65: the direct-read path, two waves of which one holds a single anchor."""
    _, yd, yl, pd, pp = _base(15, 2, 65, STAGED_MAX_L + 11, 0.2)
    return Case("long_rows", yd, yl, pd, pp, 0.25, 2.0, 1.0, {})


_CASES = None


def cases():
    """name -> Case, built once, read-only."""
    global _CASES
    if _CASES is None:
        _CASES = collections.OrderedDict()
        for c in (_tiny(), _small(), _tile_plus_one(), _two_tiles_plus_one(), _long_rows()):
            for a in (c.yd, c.yl, c.pd, c.pp):
                a.setflags(write=False)
            _CASES[c.name] = c
    return _CASES


_ORACLE = {}


def oracle(name):
    """The case's oracle values, computed once: per-anchor f, conf [B] (float64), loc [B] (oracle/loss_oracle, float32),
    and the autograd gradients at grad_scale 1 / B."""
    if name not in _ORACLE:
        c = cases()[name]
        loc64, conf64, gd, gz = torch_loss_and_grads(c.yd, c.yl, c.pd, c.pp, c.loc_alpha, c.alpha, c.gamma)
        o = dict(f=per_anchor(c.yl, c.pp, c.alpha, c.gamma), conf=conf_loss(c.yl, c.pp, c.alpha, c.gamma),
                 loc=lo.loc_loss_fn(c.yd, c.pd, c.loc_alpha), loc64=loc64, conf64=conf64, gd=gd, gz=gz)
        for v in o.values():
            v.setflags(write=False)
        _ORACLE[name] = o
    return _ORACLE[name]


def float32_restatement(c):
    """The formula in plain float32 NumPy (values and analytic gradients at grad_scale 1 / B): its distance from the float64
    oracle is what float32 arithmetic costs on these cases, the yardstick for a bar wider than the mining kernel's."""
    y, q = c.yl, c.pp
    B = q.shape[0]
    rr = ratio32(q)
    s = q[..., 0].copy()
    for k in range(1, q.shape[-1]):
        s = s + q[..., k]
    s = s[..., None]
    r = np.clip(rr, EPS, ONE_M_EPS)
    g, a = F32(c.gamma), F32(c.alpha)
    mod = np.ones_like(r) if c.gamma == 0 else np.power(F32(1) - r, g).astype(F32)
    f = (a * mod * -(y * np.log(r))).sum(-1, dtype=F32)
    pos = positives(y).sum(-1).astype(F32)
    den = np.where(pos == 0, F32(1), pos)
    conf = f.sum(-1, dtype=F32) / den
    inside = (rr >= EPS) & (rr <= ONE_M_EPS) & (y != 0)
    rs = np.where(inside, rr, F32(0.5))
    om = F32(1) - rs
    m = np.ones_like(rs) if c.gamma == 0 else np.power(om, g).astype(F32)
    first = np.zeros_like(rs) if c.gamma == 0 else g * (m / om) * np.log(rs)
    gc = np.where(inside, (y * a) * (first - m / rs), F32(0)).astype(F32)
    gce = (F32(1.0 / B) / den)[:, None, None]
    ts = (gc * q).sum(-1, keepdims=True, dtype=F32) / (s * s)
    dp = gce * (gc / s - ts)
    dot = (q * dp).sum(-1, keepdims=True, dtype=F32)
    return f.astype(F32), conf.astype(F32), (q * (dp - dot)).astype(F32)
