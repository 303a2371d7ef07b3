"""Target assignment behind a strategy (``ssd_match_encode_cfg``): the specification of include/ssd_hip.h as a NumPy oracle,
deliberately naive, and the cases the CPU and GPU tests share.

The oracle rescans every free (prior, box) pair in every round of the bipartite stage (the kernel caches a best prior per
box and rescans only the boxes that lost theirs) and sorts ``(d2, i)`` tuples for ATSS (the kernel runs arg-min rounds).
IoU bits are ``oracle.bbox_oracle.generate_iou_map``'s; ATSS's distances are fp32 NumPy, one operation per line; its
statistics are float64, summed by a loop in list order (``np.sum`` adds pairwise and rounds otherwise).

Every case is a ``Case`` with its seed recorded; ``oracle(case)`` is computed once per case and cached (read-only)."""
import collections
import os

import numpy as np

import helpers
from oracle import bbox_oracle as bo

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L = 21

Case = collections.namedtuple("Case", "name seed strategy priors gt gl iou_threshold topk level_start")
Result = collections.namedtuple("Result", "deltas onehot label_idx match_idx forced positives")


def priors_of(backbone):
    return np.load(os.path.join(GOLD, "priors.npz"))[backbone]


def level_starts(backbone):
    starts = [0]
    for fm, ratios in zip(helpers.FMAPS[backbone], helpers.ASPECT_RATIOS):
        starts.append(starts[-1] + fm * fm * (len(ratios) + 1))
    return starts


# --------------------------------------------------------------------------- the oracle
def max_iou_image(iou, thr):
    """The reference's rule on one image's [N, G] IoU map: (arg-max, positive) -- first maximum, a NaN never wins."""
    N, G = iou.shape
    if G == 0:
        return np.zeros(N, np.int32), np.zeros(N, bool)
    safe = np.where(np.isnan(iou), F32(-np.inf), iou)
    am = np.argmax(safe, axis=1).astype(np.int32)
    return am, safe.max(axis=1) > F32(thr)


def bipartite_image(iou, labels):
    """forced: {prior: box}.  Every round looks at ALL pairs (i, g), g unassigned and valid, i free, IoU > 0."""
    N, G = iou.shape
    open_boxes = [g for g in range(G) if labels[g] > 0]
    free = np.ones(N, bool)
    forced = {}
    while open_boxes and free.any():
        cols = np.array(open_boxes)
        m = iou[:, cols].T.astype(F32).copy()            # [boxes, priors]: a flat arg-max breaks ties by smaller g, then smaller i
        ok = (m > 0) & free[None, :]                     # NaN > 0 is False
        if not ok.any():
            break
        m[~ok] = -np.inf
        flat = int(np.argmax(m))
        g, i = int(cols[flat // N]), flat % N
        forced[i] = g
        open_boxes.remove(g)
        free[i] = False
    return forced


def centres(boxes):
    b = np.asarray(boxes, F32)
    sy = b[..., 0] + b[..., 2]
    sx = b[..., 1] + b[..., 3]
    cy = sy * F32(0.5)
    cx = sx * F32(0.5)
    return cy, cx


def atss_image(priors, boxes, labels, iou, topk, level_start):
    """positives: {prior: box} and, per valid box, its candidate list (level ascending, rank ascending)."""
    pcy, pcx = centres(priors)
    gcy, gcx = centres(boxes)
    owner, cands = {}, {}
    for g in range(len(labels)):
        if labels[g] <= 0:
            continue
        dy = pcy - gcy[g]
        dx = pcx - gcx[g]
        dy2 = dy * dy
        dx2 = dx * dx
        d2 = dy2 + dx2
        assert d2.dtype == F32
        cand = []
        for s, e in zip(level_start[:-1], level_start[1:]):
            order = sorted(range(s, e), key=lambda i: (bool(np.isnan(d2[i])), float(d2[i]), i))
            cand.extend(order[:min(topk, e - s)])
        cands[g] = cand
        n = len(cand)
        v = [np.float64(iou[i, g]) for i in cand]
        total = np.float64(0)
        for x in v:
            total = total + x
        mean = total / np.float64(n)
        sq = np.float64(0)
        for x in v:
            d = x - mean
            dd = d * d
            sq = sq + dd
        var = sq / np.float64(n - 1) if n > 1 else np.float64(0)
        with np.errstate(invalid="ignore"):
            thr = mean + np.sqrt(var)
        y1, x1, y2, x2 = boxes[g]
        for i, x in zip(cand, v):
            if not x >= thr:
                continue
            if not (y1 < pcy[i] < y2 and x1 < pcx[i] < x2):
                continue
            if i not in owner or iou[i, g] > iou[i, owner[i]]:      # boxes in ascending g: a tie keeps the smaller g
                owner[i] = g
    return owner, cands


_CACHE = {}


def oracle(case):
    """The four outputs of ``ssd_match_encode_cfg`` for ``case`` (and ``forced`` / ``positives``: per image the dict
    prior -> box of the bipartite stage / of ATSS).  Cached: one computation per case, shared by the tests."""
    if case.name in _CACHE:
        return _CACHE[case.name]
    priors, gt, gl = case.priors, case.gt, case.gl
    B, G = gl.shape
    N = priors.shape[0]
    label_idx = np.zeros((B, N), np.int32)
    match_idx = np.zeros((B, N), np.int32)
    chosen = np.zeros((B, N, 4), F32)
    forced_all, pos_all = [], []
    for b in range(B):
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = bo.generate_iou_map(priors, gt[b:b + 1])[0] if G else np.zeros((N, 0), F32)
        forced, owner = {}, {}
        if case.strategy == "atss":
            owner, _ = atss_image(priors, gt[b], gl[b], iou, case.topk, case.level_start)
            am = np.full(N, -1, np.int32)
            pos = np.zeros(N, bool)
            for i, g in owner.items():
                am[i], pos[i] = g, True
        else:
            am, pos = max_iou_image(iou, case.iou_threshold)
            if case.strategy == "bipartite":
                forced = bipartite_image(iou, gl[b])
                for i, g in forced.items():
                    am[i], pos[i] = g, True
        match_idx[b] = am
        for i in np.nonzero(pos)[0]:
            label_idx[b, i] = gl[b, am[i]]
            chosen[b, i] = gt[b, am[i]]
        forced_all.append(forced)
        pos_all.append(owner)
    deltas = (bo.get_deltas_from_bboxes(priors, chosen) / np.asarray(helpers.VARIANCES, F32)).astype(F32)
    onehot = (label_idx[..., None] == np.arange(L, dtype=np.int32)).astype(F32)
    for a in (deltas, onehot, label_idx, match_idx):
        a.setflags(write=False)
    _CACHE[case.name] = Result(deltas, onehot, label_idx, match_idx, forced_all, pos_all)
    return _CACHE[case.name]


# --------------------------------------------------------------------------- the cases
def _pad(rows, G):
    """rows: list of (box or None, label): None is a padding row (box 0, label -1)."""
    gt = np.zeros((1, G, 4), F32)
    gl = -np.ones((1, G), np.int32)
    for r, (box, lab) in enumerate(rows):
        if box is not None:
            gt[0, r] = np.asarray(box, F32)
            gl[0, r] = lab
    return gt, gl


def _shrunk(p, f):
    cy, cx, h, w = (p[0] + p[2]) / 2, (p[1] + p[3]) / 2, (p[2] - p[0]) * f, (p[3] - p[1]) * f
    return np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], F32)


def voc_like(rng, B, G, small_frac=0.4):
    """Random boxes, a share of them small (sides 0.02 .. 0.08: below what any prior overlaps by half), padded with
    box 0 / label -1 rows at random positions -- not only at the tail."""
    gt = np.zeros((B, G, 4), F32)
    gl = -np.ones((B, G), np.int32)
    for b in range(B):
        n = int(rng.integers(max(1, G // 2), G + 1))
        rows = np.sort(rng.choice(G, n, replace=False))
        c = rng.uniform(0.1, 0.9, (n, 2))
        s = np.where(rng.random((n, 1)) < small_frac, rng.uniform(0.02, 0.08, (n, 2)), rng.uniform(0.1, 0.6, (n, 2)))
        gt[b, rows] = np.clip(np.concatenate([c - s / 2, c + s / 2], -1), 0, 1).astype(F32)
        gl[b, rows] = rng.integers(1, L, n)
    return gt, gl


def _bipartite(name, seed, priors, gt, gl, thr=0.5):
    return Case(name, seed, "bipartite", np.ascontiguousarray(priors, F32), gt, gl, thr, 0, None)


def _atss(name, seed, priors, gt, gl, topk, level_start):
    return Case(name, seed, "atss", np.ascontiguousarray(priors, F32), gt, gl, 0.5, topk, list(level_start))


def _build():
    mb, vgg = priors_of("mobilenet_v2"), priors_of("vgg16")
    p300 = mb[:300]                                      # N = 300: two blocks of 256, the second partly filled
    cases = []
    # three boxes whose best prior is the same prior (shrunk copies of it), two padding rows BETWEEN the valid ones
    base = p300[4 * 24]
    gt, gl = _pad([(_shrunk(base, 0.97), 3), (None, 0), (_shrunk(base, 0.94), 5), (None, 0), (_shrunk(base, 0.91), 7)], 5)
    cases.append(_bipartite("shared_best_n300", None, p300, gt, gl))
    # eight nested boxes around one cell: a conflict chain, the rescan runs again and again
    gt, gl = _pad([(_shrunk(base, 1.0 - 0.04 * k), 1 + k) for k in range(8)], 8)
    cases.append(_bipartite("nested_chain", None, p300, gt, gl))
    # two identical boxes: the tie goes to the smaller g, the other takes the runner-up
    gt, gl = _pad([(_shrunk(base, 0.9), 2), (_shrunk(base, 0.9), 9)], 2)
    cases.append(_bipartite("identical_boxes", None, p300, gt, gl))
    # a valid label on a zero-area box: IoU 0 everywhere, never forced
    gt, gl = _pad([([0.3, 0.3, 0.3, 0.5], 4), ([0.31, 0.12, 0.36, 0.2], 6)], 2)
    cases.append(_bipartite("zero_area_box", None, p300, gt, gl))
    # more valid boxes than priors: the loop ends when the priors run out
    p3 = mb[[1444 + 6 * 44, 1444 + 6 * 45, 1444 + 6 * 55]]
    gt, gl = _pad([(_shrunk(p3[k % 3], 1.0 - 0.05 * k), 1 + k) for k in range(5)], 5)
    cases.append(_bipartite("three_priors_five_boxes", None, p3, gt, gl))
    cases.append(_bipartite("no_rows", None, p300, np.zeros((2, 0, 4), F32), np.zeros((2, 0), np.int32)))
    cases.append(_bipartite("no_images", None, p300, np.zeros((0, 5, 4), F32), np.zeros((0, 5), np.int32)))
    for name, pri, B, G, seed in (("real_mobilenet_v2", mb, 4, 12, 20261), ("real_vgg16", vgg, 2, 40, 20262)):
        gt, gl = voc_like(np.random.default_rng(seed), B, G)
        cases.append(_bipartite(name, seed, pri, gt, gl))
    # ---- ATSS
    ls = level_starts("mobilenet_v2")
    gt, gl = voc_like(np.random.default_rng(20263), 4, 12)
    for k in (1, 9, 64):                                 # the 2x2 and 1x1 levels (24 and 4 priors) are smaller than 9 / 64
        cases.append(_atss("atss_real_top%d" % k, 20263, mb, gt, gl, k, ls))
    # centred exactly on the centre of cell (9, 9) of the 19x19 map: ties inside the cell and between mirror cells
    cy, cx = centres(mb[4 * (9 * 19 + 9)])
    gt, gl = _pad([([cy - F32(0.125), cx - F32(0.25), cy + F32(0.125), cx + F32(0.25)], 8)], 1)
    cases.append(_atss("atss_cell_centre", None, mb, gt, gl, 9, ls))
    # one level of four equal priors: one IoU, deviation 0, all pass >=
    same = np.repeat(np.array([[0.25, 0.25, 0.5, 0.5]], F32), 4, 0)
    gt, gl = _pad([([0.2, 0.2, 0.6, 0.6], 11)], 1)
    cases.append(_atss("atss_one_iou", None, same, gt, gl, 4, [0, 4]))
    # n == 1
    gt, gl = _pad([([0.1, 0.1, 0.3, 0.3], 2)], 1)
    cases.append(_atss("atss_single_candidate", None, p300, gt, gl, 1, [0, 300]))
    # priors positive for two boxes: an identical pair (the tie goes to the smaller g) and a slightly larger third box
    box = np.array([0.3, 0.3, 0.6, 0.62], F32)
    gt, gl = _pad([(box, 3), (box, 4), (box + np.array([-0.01, -0.01, 0.01, 0.01], F32), 5)], 3)
    cases.append(_atss("atss_shared_prior", None, mb, gt, gl, 9, ls))
    # padding rows between the valid ones
    gt, gl = _pad([(None, 0), ([0.1, 0.1, 0.5, 0.4], 1), (None, 0), (None, 0), ([0.4, 0.5, 0.9, 0.95], 12), (None, 0),
                   ([0.45, 0.45, 0.55, 0.56], 20)], 7)
    cases.append(_atss("atss_padding_between", None, mb, gt, gl, 9, ls))
    cases.append(_atss("atss_no_rows", None, mb, np.zeros((2, 0, 4), F32), np.zeros((2, 0), np.int32), 9, ls))
    for c in cases:
        for a in (c.priors, c.gt, c.gl):
            a.setflags(write=False)
    return collections.OrderedDict((c.name, c) for c in cases)


_CASES = _build()


def names(strategy=None):
    return [n for n, c in _CASES.items() if strategy is None or c.strategy == strategy]


def by_name(name):
    return _CASES[name]


def rescued_boxes(case):
    """(image, box) pairs that ``max_iou`` leaves without a positive prior and ``bipartite`` gives one."""
    plain = oracle(case._replace(name=case.name + "/max_iou", strategy="max_iou"))
    forced = oracle(case)
    out = []
    for b in range(case.gl.shape[0]):
        for g in np.nonzero(case.gl[b] > 0)[0]:
            had = ((plain.match_idx[b] == g) & (plain.label_idx[b] > 0)).any()
            has = ((forced.match_idx[b] == g) & (forced.label_idx[b] > 0)).any()
            if has and not had:
                out.append((b, int(g)))
    return out


for _name in ("real_mobilenet_v2", "real_vgg16"):
    # a case in which the bipartite stage rescues no box would show nothing
    assert rescued_boxes(_CASES[_name]), "%s: no box is left without a positive by max_iou and given one by bipartite" % _name
