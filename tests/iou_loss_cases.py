"""Cases and oracle for the IoU-family localisation losses (csrc/ssd_iouloss.hip, ``ssd_loss.IoULocLoss``); needs no GPU.

The formulas are the ones include/ssd_hip.h states (``ssd_iou_loc_loss``): the boxes ``t`` and ``b`` decoded from the actual
and the predicted deltas times the variances, then IoU / GIoU / DIoU / CIoU between them as ``torchvision.ops`` defines them,
per image ``loc_loss_alpha * sum_pos l / max(pos, 1)``.  The oracle is a torch-CPU float64 autograd graph of exactly that
(``a`` of CIoU detached).  Targets come from ``oracle/bbox_oracle.calculate_actual_outputs`` on the SSD300-MobileNetV2 priors,
of which every case keeps a subset of N anchors; predictions are the targets plus N(0,1) noise on the deltas, and among the
positives of every case but ``tiny`` the generator plants disjoint pairs (``dx + 25``), a prediction strictly inside its
target, a target strictly inside its prediction and up to three DESIGNATED anchors whose prediction equals the target
exactly (the loss has a kink there: only the value and finiteness are asserted at those; their target is a hand-made box).
Every other positive keeps all four coordinate pairs of ``b`` and ``t``, and both intersection extents, at least 1e-4 away
from a tie, so no comparison depends on the subgradient rule.

Bars (tests/test_iou_loss_gpu.py): the project's existing ones -- losses rtol 1e-5 / atol 1e-7, gradients 1e-6 absolute --
stand wherever four times the worst figure of ``float32_restatement`` stays inside them, which
tests/test_iou_loss_cpu.py::test_what_float32_costs_on_the_cases asserts; the gradients are also held, relative to the
case's largest oracle entry, to four times the restatement's worst relative figure (``restatement_figures()["grel"]``,
6.11e-7 with NumPy's float32 exp and arctan: a bar of 2.4e-6 of the largest entry)."""
import collections
import math

import numpy as np

import helpers
import ssd_hip
from oracle import bbox_oracle as bo

F32 = np.float32
EPS = float(F32(1e-7))
TILE = int(ssd_hip.lib().ssd_iou_loc_loss_tile())      # the kernel's anchors per workgroup (loading the library needs no GPU)
MODES = ("iou", "giou", "diou", "ciou")
K_V = 4.0 / math.pi ** 2
TIE_MARGIN = 1e-4
LOSS_RTOL, LOSS_ATOL, GRAD_ATOL = 1e-5, 1e-7, 1e-6
DESIGNATED_BOX = np.array([0.2, 0.25, 0.7, 0.8], F32)      # the target of every designated (prediction == target) anchor

Case = collections.namedtuple("Case", "name priors var yd pd loc_alpha marks")


# ---------------------------------------------------------------------------------------------- the formulas (torch)
def decode_t(priors, deltas, var):
    """utils/bbox_utils.py:61-85 on deltas * variances, torch, any dtype; priors [N,4], deltas [...,N,4]."""
    d = deltas * var
    pw = priors[..., 3] - priors[..., 1]
    ph = priors[..., 2] - priors[..., 0]
    pcx = priors[..., 1] + 0.5 * pw
    pcy = priors[..., 0] + 0.5 * ph
    w = d[..., 3].exp() * pw
    h = d[..., 2].exp() * ph
    cx = d[..., 1] * pw + pcx
    cy = d[..., 0] * ph + pcy
    y1 = cy - 0.5 * h
    x1 = cx - 0.5 * w
    import torch
    return torch.stack([y1, x1, h + y1, w + x1], -1)


def box_loss_t(b, t, mode, a_const=None):
    """[...,4] boxes (y1,x1,y2,x2) -> [...] loss; ``a_const``: CIoU's weight taken from outside (finite differences step the
    function whose ``a`` is a constant, which is what the stop-gradient differentiates)."""
    import torch
    y1, x1, y2, x2 = b.unbind(-1)
    ty1, tx1, ty2, tx2 = t.unbind(-1)
    ih = (torch.minimum(y2, ty2) - torch.maximum(y1, ty1)).clamp(min=0)
    iw = (torch.minimum(x2, tx2) - torch.maximum(x1, tx1)).clamp(min=0)
    inter = ih * iw
    union = (y2 - y1) * (x2 - x1) + (ty2 - ty1) * (tx2 - tx1) - inter
    iou = inter / (union + EPS)
    ch = torch.maximum(y2, ty2) - torch.minimum(y1, ty1)
    cw = torch.maximum(x2, tx2) - torch.minimum(x1, tx1)
    if mode == "iou":
        return 1 - iou
    if mode == "giou":
        ac = ch * cw
        return 1 - (iou - (ac - union) / (ac + EPS))
    rho2 = ((y1 + y2) / 2 - (ty1 + ty2) / 2) ** 2 + ((x1 + x2) / 2 - (tx1 + tx2) / 2) ** 2
    c2 = ch * ch + cw * cw + EPS
    l = 1 - iou + rho2 / c2
    if mode == "diou":
        return l
    assert mode == "ciou", mode
    v = K_V * (torch.atan((tx2 - tx1) / (ty2 - ty1)) - torch.atan((x2 - x1) / (y2 - y1))) ** 2
    a = (v / ((1 - iou) + v + EPS)).detach() if a_const is None else a_const
    return l + a * v


def positives(yd):
    return (np.asarray(yd) != 0).any(-1)


def torch_loss_and_grads(priors, var, yd, pd, mode, loc_alpha, grad_scale=None):
    """float64 autograd -> (per-anchor l [B,N], 0 where not positive; loc [B]; d/d pred_deltas of ``grad_scale * sum_b loc_b``).
    ``grad_scale`` None: 1 / B."""
    import torch
    dt = torch.float64
    p_t, v_t = torch.as_tensor(np.array(priors), dtype=dt), torch.as_tensor(np.array(var), dtype=dt)
    yd_t = torch.as_tensor(np.array(yd), dtype=dt)
    pd_t = torch.as_tensor(np.array(pd), dtype=dt).clone().requires_grad_(True)
    B = pd_t.shape[0]
    gs = 1.0 / B if grad_scale is None else float(grad_scale)
    pos = torch.as_tensor(positives(yd))
    l = box_loss_t(decode_t(p_t, pd_t, v_t), decode_t(p_t, yd_t, v_t), mode)
    l = torch.where(pos, l, torch.zeros_like(l))
    cnt = pos.sum(-1).to(dt)
    loc = l.sum(-1) / torch.where(cnt == 0, torch.ones_like(cnt), cnt) * float(loc_alpha)
    (gs * loc.sum()).backward()
    return l.detach().numpy(), loc.detach().numpy(), pd_t.grad.numpy()


def objective(priors, var, yd, pd, mode, loc_alpha, a_const=None):
    """float64: mean_b loc_b (the function the finite differences step)."""
    import torch
    with torch.no_grad():
        dt = torch.float64
        p_t, v_t = torch.as_tensor(np.array(priors), dtype=dt), torch.as_tensor(np.array(var), dtype=dt)
        yd_t, pd_t = torch.as_tensor(np.array(yd), dtype=dt), torch.as_tensor(np.array(pd), dtype=dt)
        pos = torch.as_tensor(positives(yd))
        l = box_loss_t(decode_t(p_t, pd_t, v_t), decode_t(p_t, yd_t, v_t), mode, a_const=a_const)
        l = torch.where(pos, l, torch.zeros_like(l))
        cnt = pos.sum(-1).to(dt)
        return float((l.sum(-1) / torch.where(cnt == 0, torch.ones_like(cnt), cnt) * float(loc_alpha)).mean())


def ciou_weight(priors, var, yd, pd):
    """float64 [B,N]: CIoU's a = v / ((1 - iou) + v + eps) at ``pd`` (held fixed by ``objective(..., a_const=)``)."""
    import torch
    with torch.no_grad():
        dt = torch.float64
        p_t, v_t = torch.as_tensor(np.array(priors), dtype=dt), torch.as_tensor(np.array(var), dtype=dt)
        b = decode_t(p_t, torch.as_tensor(np.array(pd), dtype=dt), v_t)
        t = decode_t(p_t, torch.as_tensor(np.array(yd), dtype=dt), v_t)
        one_minus_iou = box_loss_t(b, t, "iou")
        v = box_loss_t(b, t, "ciou", a_const=torch.ones((), dtype=dt)) - box_loss_t(b, t, "diou")
        return v / (one_minus_iou + v + EPS)


# ---------------------------------------------------------------------------------------------- the cases
_POOL = None


def pool():
    """The SSD300-MobileNetV2 priors [2268,4] and the targets of three seeded images on them."""
    global _POOL
    if _POOL is None:
        hp = helpers.hyper_params("mobilenet_v2")
        priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
        gt, gl = helpers.gt_inputs(3, G=8, L=hp["total_labels"], seed=3)
        yd, _ = bo.calculate_actual_outputs(priors, gt, gl, hp)
        _POOL = (priors, yd, np.asarray(hp["variances"], F32))
    return _POOL


def _decode64(priors, deltas, var):
    import torch
    return decode_t(torch.as_tensor(np.asarray(priors, np.float64)), torch.as_tensor(np.asarray(deltas, np.float64)),
                    torch.as_tensor(np.asarray(var, np.float64))).numpy()


def tie_distance(priors, var, yd, pd):
    """[B,N]: the smallest distance from a tie -- of the four coordinate pairs of b and t and of the two intersection extents
    from 0 (float64 decode)."""
    b, t = _decode64(priors, pd, var), _decode64(priors, yd, var)
    d = np.abs(b - t).min(-1)
    ihr = np.minimum(b[..., 2], t[..., 2]) - np.maximum(b[..., 0], t[..., 0])
    iwr = np.minimum(b[..., 3], t[..., 3]) - np.maximum(b[..., 1], t[..., 1])
    return np.minimum(d, np.minimum(np.abs(ihr), np.abs(iwr)))


def _make(name, seed, B, N, loc_alpha, n_equal, empty_image=None):
    priors_all, yd_all, var = pool()
    rng = np.random.default_rng(seed)
    pos_any = np.nonzero(positives(yd_all[:B]).any(0))[0]
    if N == 1:
        idx = np.nonzero(positives(yd_all[0]))[0][:1]
    else:
        k = min(len(pos_any), max(1, int(N * 0.45)))
        chosen = rng.choice(pos_any, k, replace=False)
        rest = np.setdiff1d(np.arange(priors_all.shape[0]), chosen)
        idx = np.sort(np.concatenate([chosen, rng.choice(rest, N - k, replace=False)]))
    priors = np.ascontiguousarray(priors_all[idx])
    yd = np.ascontiguousarray(yd_all[:B, idx])
    if empty_image is not None:
        yd[empty_image] = 0
    pd = (yd + rng.standard_normal(yd.shape)).astype(F32)
    marks = {"equal": [], "disjoint": [], "pred_inside": None, "target_inside": None}
    bi, ni = np.nonzero(positives(yd))
    order = rng.permutation(len(bi))
    where = [(int(bi[i]), int(ni[i])) for i in order]
    if N > 1:
        n_dis = -(-len(where) // 10) + 1                       # at least 10 % of the positives, rounded up, and one more
        assert len(where) >= n_dis + 2 + n_equal + 4, "%s: only %d positives" % (name, len(where))
        for at in where[:n_dis]:
            pd[at][1] += F32(25)
            marks["disjoint"].append(at)
        at = where[n_dis]
        pd[at] = yd[at] + np.array([0, 0, -3, -3], F32)        # same centre, 0.55 of the size
        marks["pred_inside"] = at
        at = where[n_dis + 1]
        pd[at] = yd[at] + np.array([0, 0, 3, 3], F32)
        marks["target_inside"] = at
        for at in where[n_dis + 2:n_dis + 2 + n_equal]:
            # a hand-made target of area 0.275: at b == t the formula gives l = eps / (area + eps) = 3.6e-7 (plus one float32
            # rounding of iou, 6e-8), so that |l| <= 1e-6 follows from the contract and not from the anchor drawn
            yd[at] = (bo.get_deltas_from_bboxes(priors[at[1]], DESIGNATED_BOX) / var).astype(F32)
            pd[at] = yd[at]
            marks["equal"].append(at)
        free = where[n_dis + 2 + n_equal:]
    else:
        free = where
    # no other positive within TIE_MARGIN of a tie: draw its noise again until that holds
    for _ in range(200):
        dist = tie_distance(priors, var, yd, pd)
        bad = [at for at in free if dist[at] < TIE_MARGIN]
        if not bad:
            break
        for at in bad:
            pd[at] = (yd[at] + rng.standard_normal(4)).astype(F32)
    dist = tie_distance(priors, var, yd, pd)
    for at in where:
        assert at in marks["equal"] or dist[at] >= TIE_MARGIN, (name, at, dist[at])
    return Case(name, priors, var, yd, pd, loc_alpha, marks)


_CASES = None


def cases():
    """name -> Case, built once, read-only.  tiny 1 x 1; small 2 x 70 (image 0 without a positive); tile_plus_one
    3 x (T + 1); two_tiles_plus_one 2 x (2T + 1)."""
    global _CASES
    if _CASES is None:
        _CASES = collections.OrderedDict()
        for c in (_make("tiny", 21, 1, 1, 1.0, 0), _make("small", 22, 2, 70, 1.0, 2, empty_image=0),
                  _make("tile_plus_one", 23, 3, TILE + 1, 1.5, 3), _make("two_tiles_plus_one", 24, 2, 2 * TILE + 1, 1.0, 1)):
            for a in (c.priors, c.var, c.yd, c.pd):
                a.setflags(write=False)
            _CASES[c.name] = c
    return _CASES


def compared(c):
    """[B,N] bool: the anchors whose gradient is compared with the oracle's -- all but the designated ones."""
    m = np.ones(c.yd.shape[:2], bool)
    for at in c.marks["equal"]:
        m[at] = False
    return m


_ORACLE = {}


def oracle(name, mode):
    """float64: per-anchor l [B,N], loc [B], gradient [B,N,4] at grad_scale 1 / B; computed once, read-only."""
    if (name, mode) not in _ORACLE:
        c = cases()[name]
        l, loc, gd = torch_loss_and_grads(c.priors, c.var, c.yd, c.pd, mode, c.loc_alpha)
        o = dict(l=l, loc=loc, gd=gd)
        for v in o.values():
            v.setflags(write=False)
        _ORACLE[(name, mode)] = o
    return _ORACLE[(name, mode)]


# ---------------------------------------------------------------------------------------------- float32 restatement
def _decode32(p, d, var):
    half = F32(0.5)
    dy, dx, dh, dw = (d[..., k] * var[k] for k in range(4))
    pw = p[..., 3] - p[..., 1]
    ph = p[..., 2] - p[..., 0]
    pcx = p[..., 1] + half * pw
    pcy = p[..., 0] + half * ph
    w = np.exp(dw) * pw
    h = np.exp(dh) * ph
    cx = dx * pw + pcx
    cy = dy * ph + pcy
    y1 = cy - half * h
    x1 = cx - half * w
    return y1, x1, h + y1, w + x1, h, w, ph, pw


def float32_restatement(c, mode, grad_scale=None):
    """The kernel's arithmetic in plain float32 NumPy, analytic gradient included (values, per-image losses, gradients at
    grad_scale 1 / B): its distance from the float64 oracle is what float32 arithmetic costs on these cases."""
    one, two, half, eps, kv = F32(1), F32(2), F32(0.5), F32(1e-7), F32(K_V)
    var = np.asarray(c.var, F32)
    yd, pd, p = np.asarray(c.yd, F32), np.asarray(c.pd, F32), np.asarray(c.priors, F32)
    B = pd.shape[0]
    with np.errstate(all="ignore"):
        ty1, tx1, ty2, tx2, _, _, _, _ = _decode32(p, yd, var)
        y1, x1, y2, x2, h, w, ph, pw = _decode32(p, pd, var)
        ihr = np.minimum(y2, ty2) - np.maximum(y1, ty1)
        iwr = np.minimum(x2, tx2) - np.maximum(x1, tx1)
        ih, iw = np.maximum(ihr, F32(0)), np.maximum(iwr, F32(0))
        inter = ih * iw
        hb, wb, ht, wt = y2 - y1, x2 - x1, ty2 - ty1, tx2 - tx1
        uni = (hb * wb + ht * wt) - inter
        U = uni + eps
        iou = inter / U
        ch = np.maximum(y2, ty2) - np.minimum(y1, ty1)
        cw = np.maximum(x2, tx2) - np.minimum(x1, tx1)
        l = one - iou
        g_inter = -((one + iou) / U)
        g_area = iou / U
        zero = np.zeros_like(l)
        g_ch, g_cw, g_cy, g_cx, g_hb, g_wb = zero, zero, zero, zero, zero, zero
        if mode == "giou":
            ac = ch * cw
            A = ac + eps
            l = one - (iou - (ac - uni) / A)
            rA = one / A
            g_inter = g_inter + rA
            g_area = g_area - rA
            g_ac = U / (A * A)
            g_ch, g_cw = g_ac * cw, g_ac * ch
        elif mode in ("diou", "ciou"):
            dyc = (y1 + y2) * half - (ty1 + ty2) * half
            dxc = (x1 + x2) * half - (tx1 + tx2) * half
            rho2 = dyc * dyc + dxc * dxc
            c2 = (ch * ch + cw * cw) + eps
            pen = rho2 / c2
            l = l + pen
            g_c2 = -(pen / c2)
            g_ch, g_cw = g_c2 * (two * ch), g_c2 * (two * cw)
            g_cy, g_cx = (two * dyc) / c2, (two * dxc) / c2
            if mode == "ciou":
                d = np.arctan(wt / ht) - np.arctan(wb / hb)
                v = kv * (d * d)
                a = v / (((one - iou) + v) + eps)
                l = l + a * v
                g_ap = a * (-(two * kv) * d)
                den = hb * hb + wb * wb
                g_wb = g_ap * (hb / den)
                g_hb = g_ap * (-(wb / den))
        gy1 = np.where((ihr > 0) & (y1 >= ty1), -(g_inter * iw), zero)
        gy2 = np.where((ihr > 0) & (y2 <= ty2), g_inter * iw, zero)
        gx1 = np.where((iwr > 0) & (x1 >= tx1), -(g_inter * ih), zero)
        gx2 = np.where((iwr > 0) & (x2 <= tx2), g_inter * ih, zero)
        g_hb = g_hb + g_area * wb
        g_wb = g_wb + g_area * hb
        gy2, gy1 = gy2 + g_hb, gy1 - g_hb
        gx2, gx1 = gx2 + g_wb, gx1 - g_wb
        gy2 = gy2 + np.where(y2 >= ty2, g_ch, zero)
        gy1 = gy1 - np.where(y1 <= ty1, g_ch, zero)
        gx2 = gx2 + np.where(x2 >= tx2, g_cw, zero)
        gx1 = gx1 - np.where(x1 <= tx1, g_cw, zero)
        gy1, gy2 = gy1 + half * g_cy, gy2 + half * g_cy
        gx1, gx2 = gx1 + half * g_cx, gx2 + half * g_cx
        raw = np.stack([(gy1 + gy2) * (var[0] * ph), (gx1 + gx2) * (var[1] * pw),
                        (half * (gy2 - gy1)) * (h * var[2]), (half * (gx2 - gx1)) * (w * var[3])], -1).astype(F32)
    pos = positives(yd)
    l = np.where(pos, l, F32(0)).astype(F32)
    cnt = pos.sum(-1).astype(F32)
    den = np.where(cnt == 0, F32(1), cnt)
    loc = (l.sum(-1, dtype=F32) / den * F32(c.loc_alpha)).astype(F32)
    gs = F32(1.0 / B if grad_scale is None else grad_scale)
    g = (gs * F32(c.loc_alpha) / den)[:, None, None]
    gd = np.where(pos[..., None], g * raw, F32(0)).astype(F32)
    return l, loc, gd


_FIGURES = None


def restatement_figures():
    """Worst distance of ``float32_restatement`` from the oracle over every case and mode (the designated anchors left out):
    ``l`` per-anchor relative, ``loc`` per-image relative, ``g`` gradient absolute, ``grel`` gradient over the case's largest
    oracle entry; ``rows`` one tuple per case and mode.  Computed once."""
    global _FIGURES
    if _FIGURES is None:
        w = dict(l=0.0, loc=0.0, g=0.0, grel=0.0, rows=[])
        for name, c in cases().items():
            keep = positives(c.yd) & compared(c)
            for mode in MODES:
                o = oracle(name, mode)
                l, loc, gd = float32_restatement(c, mode)
                dl = float(np.abs(l[keep] / o["l"][keep] - 1).max()) if keep.any() else 0.0
                nz = o["loc"] != 0
                dloc = float(np.abs(loc[nz] / o["loc"][nz] - 1).max())
                dg = float(np.abs(gd - o["gd"])[compared(c)].max())
                big = float(np.abs(o["gd"]).max())
                w["rows"].append((name, mode, dl, dloc, dg, dg / big, big))
                w.update(l=max(w["l"], dl), loc=max(w["loc"], dloc), g=max(w["g"], dg), grel=max(w["grel"], dg / big))
        _FIGURES = w
    return _FIGURES
