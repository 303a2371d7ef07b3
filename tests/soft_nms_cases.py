"""Cases and oracle for Soft-NMS and class-agnostic suppression (csrc/ssd_decode.hip ``soft_nms_kernel``, ``ssd_decode_nms_cfg`` /
``ssd_combined_nms_cfg`` / ``ssd_net_predict_cfg``); needs no GPU.

include/ssd_hip.h states the arithmetic (``ssd_nms_config``): the candidates of the hard NMS, then per list "take the largest
current score (ties: lower anchor, then lower class), decay or remove the others by their IoU with it" -- Gaussian with TF's
``soft_nms_sigma`` convention (weight ``exp(-0.5 / sigma * iou^2)``), linear, or hard -- and the per-image merge of
``ssd_decode_nms``.  TensorFlow is not installed where this runs: ``oracle`` below is that text in float64 and THE reference
here; no TF-executed data stands behind it.  ``float32_restatement`` is the same steps in NumPy float32, one rounding per
operation: what it loses against the oracle is what the number format costs, and sets the bars.

Bars (tests/test_soft_nms_gpu.py): selected anchors, classes, ``valid`` and the padding compare exactly; scores against the
float64 oracle, relative to the case's largest emitted score, within ``score_bar(case)`` = four times the restatement's worst
(relative, per score) deviation on that case with a floor of 2 ulp of fp32 (the factor covers ``expf`` against NumPy's ``exp``; it is the factor
tests/iou_loss_cases.py uses); boxes exactly in raw form, within ``test_bbox_gpu.TOL`` in decoder form (the oracle decodes in
float64).

Exact comparison of the ORDER needs the cases to stay away from near-ties: every case with a soft method satisfies
``tie_gap(case) >= 16 * deviation`` -- the relative gap between the winner and the runner-up of every selection step
against the worst relative deviation of an emitted score; two scores each off by the bar are 8 x the deviation apart, the 16
leaves a factor of two.  The IoUs
themselves need no margin in raw form: they are sums, products and one correctly rounded division of the same fp32 inputs,
the kernel's bits are the restatement's, whose order is asserted to be the oracle's.  Exactly
equal scores (planted duplicates) are exempt: equal bits stay equal and are resolved by index.  The generators draw seeds
from the recorded one upwards until that holds; ``case.seed`` is the seed used."""
import collections
import functools
import heapq
import os

import numpy as np

import helpers
import ssd_hip

F32 = np.float32
ULP = float(np.finfo(np.float32).eps)
LDS_CANDIDATES = int(ssd_hip.lib().ssd_nms_lds_candidates())       # loading the library needs no GPU
METHODS = ("hard", "gaussian", "linear")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Case = collections.namedtuple("Case", "name form boxes scores deltas priors var method agnostic max_per_class max_total "
                                      "iou_threshold score_threshold sigma clip seed")


def make_case(name, form, method, agnostic=False, max_per_class=200, max_total=200, iou_threshold=0.5, score_threshold=0.5,
              sigma=0.5, clip=True, boxes=None, scores=None, deltas=None, priors=None, var=None, seed=None):
    return Case(name, form, boxes, scores, deltas, priors, var, method, bool(agnostic), int(max_per_class), int(max_total),
                float(iou_threshold), float(score_threshold), float(sigma), bool(clip), seed)


# ---------------------------------------------------------------------------------------------- the specification
def _iou_many(a, w):
    """The TF IOU helper (csrc nms_iou): a [M,4] against one box w [4], in the dtype of ``a``; boxes unclipped."""
    zero = a.dtype.type(0)
    ymin_i, ymax_i = np.minimum(a[:, 0], a[:, 2]), np.maximum(a[:, 0], a[:, 2])
    xmin_i, xmax_i = np.minimum(a[:, 1], a[:, 3]), np.maximum(a[:, 1], a[:, 3])
    ymin_j, ymax_j = min(w[0], w[2]), max(w[0], w[2])
    xmin_j, xmax_j = min(w[1], w[3]), max(w[1], w[3])
    area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i)
    area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j)
    iy = np.maximum(np.minimum(ymax_i, ymax_j) - np.maximum(ymin_i, ymin_j), zero)
    ix = np.maximum(np.minimum(xmax_i, xmax_j) - np.maximum(xmin_i, xmin_j), zero)
    inter = iy * ix
    with np.errstate(divide="ignore", invalid="ignore"):
        o = inter / (area_i + area_j - inter)
    return np.where((area_i <= zero) | (area_j <= zero), zero, o)


def _first(anchor, cls, members):
    """Of the candidates ``members`` (equal scores): lower anchor index, then lower class index."""
    return members[np.lexsort((cls[members], anchor[members]))[0]]


def select_list(boxes, anchor, cls, scores, method, iou_thr, score_thr, scale, limit, stats=None):
    """The selection loop on one candidate list, in the dtype of ``boxes`` ([N,4], indexed by ``anchor``); ``scores`` the
    candidates' initial scores.  Returns [(anchor, class, emitted score)]; ``stats`` (a dict) receives the smallest winner /
    runner-up gap relative to the winner ("gap") and the smallest distance of a decayed score from the score threshold
    relative to the threshold ("margin")."""
    dt = boxes.dtype.type
    s = scores.astype(boxes.dtype).copy()
    bx = boxes[anchor]
    iou_thr, score_thr, scale = dt(iou_thr), dt(score_thr), dt(scale)
    alive = np.ones(s.shape[0], bool)
    out = []
    while len(out) < limit and alive.any():
        idx = np.nonzero(alive)[0]
        top = s[idx].max()
        w = _first(anchor, cls, idx[s[idx] == top])
        if stats is not None and idx.size > 1:
            rest = s[idx[idx != w]]
            rest = rest[rest != top]                    # equal bits: resolved by index, exempt
            if rest.size:
                stats["gap"] = min(stats.get("gap", np.inf), float(top - rest.max()) / (abs(float(top)) or 1.0))
        out.append((int(anchor[w]), int(cls[w]), s[w]))
        alive[w] = False
        idx = idx[idx != w]
        if idx.size == 0:
            break
        o = _iou_many(bx[idx], bx[w])
        if method == "hard":
            alive[idx[o > iou_thr]] = False
            continue
        if method == "linear":
            new = np.where(o > iou_thr, s[idx] * (dt(1) - o), s[idx])
        else:
            new = s[idx] * np.exp((scale * o) * o)
        if stats is not None:
            moved = new != s[idx]
            if moved.any():
                stats["margin"] = min(stats.get("margin", np.inf),
                                      float(np.abs(new[moved] - score_thr).min()) / (abs(float(score_thr)) or 1.0))
        s[idx] = new
        alive[idx[~(new > score_thr)]] = False
    return out


def lazy_gaussian_list(boxes, anchor, cls, scores, iou_thr, score_thr, scale, limit):
    """TF's structure (non_max_suppression_with_scores, V5 kernel) for the Gaussian method, float64: a priority queue of
    candidates; pop the maximum, apply the decays of the selections made since it was last examined (oldest first), select
    it if its score did not change, push it back otherwise.  Same ties as ``select_list``."""
    bx = boxes[anchor].astype(np.float64)
    heap = [(-float(s), int(a), int(c), k, 0) for k, (a, c, s) in enumerate(zip(anchor, cls, scores))]
    heapq.heapify(heap)
    selected, out = [], []
    while len(out) < limit and heap:
        neg, a, c, k, begin = heapq.heappop(heap)
        score = original = -neg
        alive = True
        for w in selected[begin:]:
            o = float(_iou_many(bx[k:k + 1], bx[w])[0])
            score = score * np.exp((scale * o) * o)
            if not score > score_thr:
                alive = False
                break
        if not alive:
            continue
        if score == original:
            out.append((a, c, score))
            selected.append(k)
        else:
            heapq.heappush(heap, (-score, a, c, k, len(selected)))
    return out


def scale_of(sigma):
    """``-0.5f / sigma``: ONE float division on the host -- the oracle takes the rounded value, as the kernel does."""
    return float(F32(-0.5) / F32(sigma))


def candidate_inputs(case, dtype):
    """(boxes [B,N,4] in ``dtype``, scores [B,N,C] float32 after the decoder's class mask)."""
    if case.form == "raw":
        return np.asarray(case.boxes, F32).astype(dtype), np.asarray(case.scores, F32)
    # models/decoder.py:41-45 -- utils/bbox_utils.py:61-85 on deltas * variances
    dt = np.dtype(dtype).type
    p = np.asarray(case.priors, F32).astype(dtype)
    d = np.asarray(case.deltas, F32).astype(dtype) * np.asarray(case.var, F32).astype(dtype)
    pw, ph = p[:, 3] - p[:, 1], p[:, 2] - p[:, 0]
    pcx, pcy = p[:, 1] + dt(0.5) * pw, p[:, 0] + dt(0.5) * ph
    w, h = np.exp(d[..., 3]) * pw, np.exp(d[..., 2]) * ph
    cx, cy = d[..., 1] * pw + pcx, d[..., 0] * ph + pcy
    y1, x1 = cy - dt(0.5) * h, cx - dt(0.5) * w
    boxes = np.stack([y1, x1, h + y1, w + x1], -1)
    probs = np.asarray(case.scores, F32)
    masked = np.where(np.argmax(probs, -1)[..., None] != 0, probs, F32(0))
    return boxes, masked


Result = collections.namedtuple("Result", "boxes scores classes idx valid stats")


def run(case, dtype=np.float64):
    """The whole post-processor on a case in ``dtype``: (boxes [B,T,4], scores [B,T], classes [B,T], idx [B,T] (-1 on padding),
    valid [B], stats)."""
    boxes, scores = candidate_inputs(case, dtype)
    B, N, C = scores.shape
    T = case.max_total
    thr32 = F32(case.score_threshold)
    iou_thr, score_thr = float(F32(case.iou_threshold)), float(thr32)
    scale = scale_of(case.sigma) if case.method == "gaussian" else 0.0
    ob = np.zeros((B, T, 4), boxes.dtype)
    osc = np.zeros((B, T), boxes.dtype)
    oc = np.zeros((B, T), np.int64)
    oi = np.full((B, T), -1, np.int64)
    valid = np.zeros((B,), np.int64)
    stats = {}
    for b in range(B):
        emitted = []
        if case.agnostic:
            a, c = np.nonzero(scores[b] > thr32)
            limit = min(case.max_per_class, T, a.size)
            emitted = select_list(boxes[b], a, c, scores[b][a, c], case.method, iou_thr, score_thr, scale, limit, stats)
        else:
            for c in range(C):
                a = np.nonzero(scores[b, :, c] > thr32)[0]
                if a.size:
                    emitted += select_list(boxes[b], a, np.full(a.shape, c), scores[b, a, c], case.method, iou_thr, score_thr,
                                           scale, min(case.max_per_class, N), stats)
        emitted.sort(key=lambda t: (-t[2], t[0], t[1]))
        emitted = emitted[:T]
        valid[b] = len(emitted)
        for r, (a, c, s) in enumerate(emitted):
            bx = boxes[b, a]
            ob[b, r] = np.clip(bx, 0, 1) if (case.clip or case.form == "decoder") else bx
            osc[b, r], oc[b, r], oi[b, r] = s, c, a
    return Result(ob, osc, oc, oi, valid, stats)


@functools.lru_cache(maxsize=None)
def _both(name):
    case = by_name(name)
    return run(case, np.float64), run(case, np.float32)


def oracle(case):
    """The float64 oracle's ``Result`` on a case of ``cases()`` (computed once, shared; treat as read-only)."""
    return _both(case.name)[0]


def float32_restatement(case):
    return _both(case.name)[1]


def _figures(o, r):
    top = float(np.abs(o.scores).max()) if o.valid.sum() else 1.0
    same = np.array_equal(o.idx, r.idx) and np.array_equal(o.classes, r.classes) and np.array_equal(o.valid, r.valid)
    dev = float("inf")
    if same:
        den = np.where(o.scores != 0, np.abs(o.scores), 1.0)
        dev = float((np.abs(r.scores.astype(np.float64) - o.scores) / den).max()) if o.scores.size else 0.0
    return {"deviation": dev, "order_agrees": same, "tie_gap": float(o.stats.get("gap", np.inf)),
            "threshold_margin": float(o.stats.get("margin", np.inf)), "top": top}


def restatement_figures(case):
    """{"deviation": worst relative deviation |restatement - oracle| / |oracle| of an emitted score, "order_agrees": the
    restatement selected the same (anchor, class) rows in the same order, "tie_gap", "threshold_margin", "top": the largest
    emitted score}."""
    return _figures(*_both(case.name))


def tie_gap(case):
    """The smallest gap between the winner and the runner-up over all selection steps of all lists in the float64 oracle
    (exactly equal scores exempt), relative to the winner's score."""
    return restatement_figures(case)["tie_gap"]


def score_bar(case):
    return max(4.0 * restatement_figures(case)["deviation"], 2.0 * ULP)


def holds_condition(fig, method):
    """What every case satisfies.  (``threshold_margin`` -- how close a decayed score comes to the score threshold, where a
    candidate stays in one arithmetic and leaves in the other -- is reported, not required: with ~10^5..10^7 decays a case
    some score always lands within 1e-7 of it, and such a candidate only matters when it is emitted afterwards, which
    the restatement's agreement with the oracle covers.)"""
    return fig["order_agrees"] and (method == "hard" or fig["tie_gap"] >= 16.0 * fig["deviation"])


# ---------------------------------------------------------------------------------------------- the cases
def clustered(rng, B, N, C, clusters=12, degenerate=True):
    """Boxes around a few centres (heavy overlap: many decays per candidate), some inverted, some of zero area."""
    ctr = rng.uniform(0.15, 0.85, (B, clusters, 2))
    which = rng.integers(0, clusters, (B, N))
    c = np.take_along_axis(ctr, which[..., None].repeat(2, -1), 1) + rng.normal(0, 0.04, (B, N, 2))
    sz = rng.uniform(0.08, 0.4, (B, N, 2))
    if degenerate:
        sz[:, ::13] *= -1                                                       # inverted
    boxes = np.concatenate([c - sz / 2, c + sz / 2], -1).astype(F32)
    if degenerate:
        boxes[:, ::17, 2:] = boxes[:, ::17, :2]                                  # zero area
    scores = rng.uniform(0.0, 1.0, (B, N, C)).astype(F32)
    return boxes, scores


def _raw(name, B, N, C, **kw):
    def build(seed):
        boxes, scores = clustered(np.random.default_rng(seed), B, N, C)
        return make_case(name, "raw", boxes=boxes, scores=scores, seed=seed, **kw)
    return build


def _one_class_full(name, N, **kw):
    """C = 2: every score of class 0 above the threshold (one long list), class 1 sparse."""
    def build(seed):
        rng = np.random.default_rng(seed)
        boxes, scores = clustered(rng, 1, N, 2, clusters=40, degenerate=False)
        scores[0, :, 0] = rng.uniform(0.35, 1.0, N).astype(F32)
        scores[0, :, 1] = np.where(rng.random(N) < 0.02, scores[0, :, 1], F32(0))
        return make_case(name, "raw", boxes=boxes, scores=scores, seed=seed, score_threshold=0.3, **kw)
    return build


def _agnostic(name, **kw):
    """B = 2, N = 300, C = 4: anchors with two classes above the threshold, identical boxes under different classes."""
    def build(seed):
        rng = np.random.default_rng(seed)
        boxes, scores = clustered(rng, 2, 300, 4, clusters=8, degenerate=False)
        scores *= (rng.random(scores.shape) < 0.35)                              # sparse: most anchors carry 0-2 classes
        scores[:, 5:40:5, 1] = rng.uniform(0.5, 0.9, (2, 7)).astype(F32)         # two classes above the threshold on one anchor
        scores[:, 5:40:5, 2] = rng.uniform(0.5, 0.9, (2, 7)).astype(F32)
        boxes[:, 100:110] = boxes[:, 200:210]                                    # identical boxes ...
        scores[:, 100:110] = 0
        scores[:, 200:210] = 0
        scores[:, 100:110, 0] = rng.uniform(0.5, 0.9, (2, 10)).astype(F32)       # ... on different classes
        scores[:, 200:210, 3] = rng.uniform(0.5, 0.9, (2, 10)).astype(F32)
        return make_case(name, "raw", boxes=boxes, scores=scores, seed=seed, agnostic=True, score_threshold=0.3, **kw)
    return build


def mobilenet_priors():
    return np.load(os.path.join(GOLD, "priors.npz"))["mobilenet_v2"].astype(F32)


def _decoder(name, **kw):
    def build(seed):
        deltas, probs = helpers.decoder_inputs(2, 2268, 21, seed=seed)
        return make_case(name, "decoder", deltas=deltas, scores=probs, priors=mobilenet_priors(), var=helpers.VARIANCES,
                         seed=seed, **kw)
    return build


def _fixed(case):
    def build(seed):
        return case._replace(seed=seed)
    build.fixed = True              # hand-made: no seed to draw
    return build


def _planted():
    """Duplicates (identical box AND score: the copy decays to 0 under "linear", to s * exp(-0.5 / sigma) under "gaussian")
    and equal scores on disjoint boxes (lower index first)."""
    boxes = np.array([[[0.1, 0.1, 0.3, 0.3], [0.1, 0.1, 0.3, 0.3], [0.5, 0.5, 0.7, 0.7], [0.75, 0.1, 0.9, 0.3],
                       [0.75, 0.5, 0.9, 0.7], [0.1, 0.1, 0.3, 0.3]]], F32)
    scores = np.array([[[0.9], [0.9], [0.6], [0.6], [0.6], [0.5]]], F32)
    return boxes, scores


def _edge(name, tag, **kw):
    """N = 1; C = 1; a class with no candidate -- max_per_class > N in all three."""
    def build(seed):
        rng = np.random.default_rng(seed)
        N, C, mpc = {"n1": (1, 3, 5), "c1": (40, 1, 50), "hole": (60, 3, 100)}[tag]
        boxes, scores = clustered(rng, 2, N, C, clusters=3, degenerate=False)
        if tag == "hole":
            scores[:, :, 1] = 0
        return make_case(name, "raw", boxes=boxes, scores=scores, seed=seed, score_threshold=0.2, max_per_class=mpc,
                         max_total=50, **kw)
    return build


# name -> (builder, first seed to try); the seeds are the ones the search settled on (a case states its own in ``.seed``)
def _table():
    t = collections.OrderedDict()
    for m in ("gaussian", "linear"):
        for k, (thr, mpc, mt) in enumerate(((0.3, 200, 200), (-3.0e38, 30, 40), (0.9, 5, 200))):
            t["raw_%s_%d" % (m, k)] = (_raw("raw_%s_%d" % (m, k), 3, 500, 5, method=m, score_threshold=thr, max_per_class=mpc,
                                            max_total=mt), 100 + k)
        t["wide_%s" % m] = (_one_class_full("wide_%s" % m, 700, method=m, max_per_class=200, max_total=200), 200)
        t["hbm_%s" % m] = (_one_class_full("hbm_%s" % m, LDS_CANDIDATES + 37, method=m, max_per_class=24, max_total=48), 300)
        pb, ps = _planted()
        t["planted_%s" % m] = (_fixed(make_case("planted_%s" % m, "raw", m, boxes=pb, scores=ps, score_threshold=-1.0,
                                                max_per_class=6, max_total=6, sigma=0.5)), 0)
        for tag in ("n1", "c1", "hole"):
            t["edge_%s_%s" % (tag, m)] = (_edge("edge_%s_%s" % (tag, m), tag, method=m), 500)
    for m in METHODS:
        t["agnostic_%s" % m] = (_agnostic("agnostic_%s" % m, method=m, max_per_class=100, max_total=100), 400)
    t["decoder_gaussian_050"] = (_decoder("decoder_gaussian_050", method="gaussian", score_threshold=0.5), 2)
    # 0.01: ~1700 candidates a list.  max_total_size 40, not 200: the 200 best of 1700 noise-tail scores, times 42 lists, lie
    # ~1e-7 apart somewhere whatever the seed; the 40 best leave the gap the condition asks for
    t["decoder_gaussian_001"] = (_decoder("decoder_gaussian_001", method="gaussian", score_threshold=0.01, max_per_class=40,
                                          max_total=40), 2)
    t["decoder_agnostic_hard"] = (_decoder("decoder_agnostic_hard", method="hard", agnostic=True, score_threshold=0.5), 2)
    return t


SEEDS = {"raw_gaussian_0": 107}        # where the search went past the table's first seed: start there

@functools.lru_cache(maxsize=None)
def by_name(name):
    if name.endswith("_below"):
        # the same input as hbm_<method>, cut to one candidate less than the LDS limit
        full = by_name(name[:-len("_below")])
        n = LDS_CANDIDATES - 1
        return full._replace(name=name, boxes=full.boxes[:, :n], scores=full.scores[:, :n])
    build, first = _table()[name]
    first = SEEDS.get(name, first)
    for seed in range(first, first + 64):
        case = build(seed)
        fig = _figures(run(case, np.float64), run(case, np.float32))
        if holds_condition(fig, case.method):
            return case
        if getattr(build, "fixed", False):
            return case
    raise AssertionError("%s: no seed in %d..%d keeps the selection away from near-ties" % (name, first, first + 63))


def names():
    t = list(_table())
    return t + ["hbm_gaussian_below", "hbm_linear_below"]


def cases():
    return [by_name(n) for n in names()]


# ---------------------------------------------------------------------------------------------- the known answer
KNOWN_BOXES = np.array([[[0, 0, 1, 1], [0, 0, 1, 0.5], [2, 2, 3, 3]]], F32)         # A, B (IoU 0.5 with A), C (disjoint)
KNOWN_SCORES = np.array([[[0.9], [0.8], [0.7]]], F32)


def known_answers():
    """[(method, iou_threshold, sigma, [(anchor, score)...])] at score_threshold 0.1, one class."""
    return [("gaussian", 0.5, 0.5, [(0, 0.9), (2, 0.7), (1, 0.8 * np.exp(-0.25))]),
            ("linear", 0.4, 0.5, [(0, 0.9), (2, 0.7), (1, 0.4)]),
            ("linear", 0.5, 0.5, [(0, 0.9), (1, 0.8), (2, 0.7)]),                    # '>' is strict: IoU == 0.5 leaves B alone
            ("hard", 0.4, 0.5, [(0, 0.9), (2, 0.7)])]


# ---------------------------------------------------------------------------------------------- comparing a device result
def check(case, boxes, scores, classes, valid, idx=None, box_tol=0.0):
    """Device outputs (NumPy) against the oracle under the bars of the module docstring; prints the figures first."""
    o = oracle(case)
    bar = score_bar(case)
    top = restatement_figures(case)["top"]
    err = float(np.abs(scores.astype(np.float64) - o.scores).max()) / top if scores.size else 0.0
    berr = float(np.abs(boxes.astype(np.float64) - o.boxes).max()) if boxes.size else 0.0
    print("%s: score error %.3g of the top score (bar %.3g), box error %.3g (bar %.3g), valid %s" % (
        case.name, err, bar, berr, box_tol, o.valid.tolist()))
    np.testing.assert_array_equal(valid, o.valid, err_msg=case.name)
    np.testing.assert_array_equal(classes.astype(np.int64), o.classes, err_msg=case.name)
    if idx is not None:
        np.testing.assert_array_equal(idx.astype(np.int64), o.idx, err_msg=case.name)
    assert err <= bar, "%s: scores off by %.3g of the top score, bar %.3g" % (case.name, err, bar)
    if box_tol == 0.0:
        np.testing.assert_array_equal(boxes, o.boxes.astype(F32), err_msg=case.name)
    else:
        assert berr <= box_tol, "%s: boxes off by %.3g" % (case.name, berr)
    pad = np.arange(scores.shape[1])[None, :] >= o.valid[:, None]
    assert not scores[pad].any() and not boxes[pad].any() and not classes[pad].any(), "%s: padding rows are not zero" % case.name
