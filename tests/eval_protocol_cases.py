"""The oracle and the inputs of the protocol-scoring tests (tests/test_eval_protocol_cpu.py, tests/test_eval_protocol_gpu.py)
and of tests/bench_eval_protocol.py.  NumPy + ``oracle.bbox_oracle`` only: no product code, no device.

The oracle is a serial restatement of the two matching rules and the three AP definitions as include/ssd_hip.h and
``utils.eval_utils`` word them (VOCdevkit's VOCevaldet.m; pycocotools' cocoeval.evaluateImg without crowd boxes and area
ranges), one decision at a time in plain Python; its fp32 IoU is ``oracle.bbox_oracle.generate_iou_map``'s."""
import numpy as np

from oracle import bbox_oracle as bo

TP, FP, IGNORED = 1, 0, -1
COCO_THRESHOLDS = np.float32(np.linspace(.5, .95, 10))
PROTOCOLS = {"voc07": ("voc", np.array([0.5], np.float32)), "voc10": ("voc", np.array([0.5], np.float32)),
             "coco": ("coco", COCO_THRESHOLDS)}
# what ``planted`` plants and ``assert_not_vacuous`` counts
CASES = ("duplicate", "second_best", "ignored_match", "ignored_again", "tied_scores", "iou_at_threshold", "iou_tie",
         "class_without_box", "nan_iou", "all_label0_image", "all_padding_image")


def labels_for(L):
    return ["bg"] + ["c%d" % i for i in range(1, L)]


def iou_map(pb, gt):
    """[B,T,G] float32, image by image through the oracle's IoU."""
    B, T = pb.shape[:2]
    G = gt.shape[1]
    if T == 0:
        return np.zeros((B, 0, G), np.float32)
    return np.stack([bo.generate_iou_map(pb[b], gt[b:b + 1])[0] for b in range(B)]).astype(np.float32)


def _walk_voc(ious, boxes, ignore, thr, events):
    """One (class, threshold) chain of one image under the devkit's rule.  ``ious`` [n,G] of the class's records in walk
    order, ``boxes`` the class's box indices in index order.  Returns the n states."""
    taken, absorbed, states = set(), set(), []
    for row in ious:
        ovmax, jmax = -np.inf, -1
        for g in boxes:
            if np.isnan(row[g]):
                events["nan_iou"] += 1
            if row[g] > ovmax:
                ovmax, jmax = row[g], g
        if len(boxes) == 0:
            events["class_without_box"] += 1
        if jmax < 0 or ovmax < thr:
            states.append(FP)
            continue
        if ovmax == thr:
            events["iou_at_threshold"] += 1
        if any(row[g] == ovmax for g in boxes if g != jmax):
            events["iou_tie"] += 1
        if ignore[jmax]:
            events["ignored_again" if jmax in absorbed else "ignored_match"] += 1
            absorbed.add(jmax)
            states.append(IGNORED)
        elif jmax not in taken:
            taken.add(jmax)
            states.append(TP)
        else:
            events["duplicate"] += 1
            if any(row[g] >= thr and g not in taken and not ignore[g] for g in boxes):
                events["second_best"] += 1
            states.append(FP)
    return states


def _walk_coco(ious, boxes, ignore, thr, events):
    """One (class, threshold) chain of one image under pycocotools' rule."""
    candidates = [g for g in boxes if not ignore[g]] + [g for g in boxes if ignore[g]]
    taken, states = set(), []
    for row in ious:
        best, m = thr, -1
        if len(boxes) == 0:
            events["class_without_box"] += 1
        blocked = [g for g in candidates if g in taken and row[g] >= thr]
        for g in candidates:
            if np.isnan(row[g]):
                events["nan_iou"] += 1
            if g in taken:
                continue
            if m >= 0 and not ignore[m] and ignore[g]:
                break
            if not row[g] >= best:
                continue
            if m >= 0 and row[g] == best:
                events["iou_tie"] += 1
            best, m = row[g], g
        if any(ignore[g] for g in blocked):
            events["ignored_again"] += 1
        if m < 0:
            if blocked:
                events["duplicate"] += 1
            states.append(FP)
            continue
        if best == thr:
            events["iou_at_threshold"] += 1
        if blocked and not ignore[m]:
            events["second_best"] += 1
        taken.add(m)
        if ignore[m]:
            events["ignored_match"] += 1
        states.append(IGNORED if ignore[m] else TP)
    return states


def oracle_records(pb, pl, ps, gt, gl, gi=None, rule="voc", thresholds=(0.5,)):
    """Records of every image: ``(rec_class [B,T] int32, rec_score [B,T] float32, rec_det [B,T] int32, rec_state
    [B,NT,T] int8, rec_count [B] int32, events)``, zeros at and after the count; ``events`` counts, over all chains,
    the situations named in ``CASES`` as the walk met them."""
    assert rule in ("voc", "coco")
    thresholds = np.asarray(thresholds, np.float32).reshape(-1)
    B, T = pl.shape
    G = gl.shape[1]
    gi = np.zeros((B, G), bool) if gi is None else np.asarray(gi).astype(bool)
    iou = iou_map(pb, gt)
    NT = len(thresholds)
    rec_class = np.zeros((B, T), np.int32); rec_score = np.zeros((B, T), np.float32)
    rec_det = np.zeros((B, T), np.int32); rec_state = np.zeros((B, NT, T), np.int8); rec_count = np.zeros((B,), np.int32)
    events = dict.fromkeys(CASES, 0)
    walk = _walk_voc if rule == "voc" else _walk_coco
    for b in range(B):
        order = sorted((t for t in range(T) if pl[b, t] != 0), key=lambda t: (-float(ps[b, t]), t))
        n = len(order)
        rec_count[b] = n
        rec_det[b, :n] = order
        rec_class[b, :n] = [int(pl[b, t]) for t in order]
        rec_score[b, :n] = [ps[b, t] for t in order]
        events["tied_scores"] += sum(1 for i in range(1, n) if ps[b, order[i]] == ps[b, order[i - 1]])
        if T > 0 and n == 0:
            events["all_label0_image"] += 1
        if n > 0 and not (gl[b] > 0).any():
            events["all_padding_image"] += 1
        for c in sorted(set(rec_class[b, :n].tolist())):
            where = [r for r in range(n) if rec_class[b, r] == c]
            boxes = [g for g in range(G) if gl[b, g] == c]
            ious = iou[b][[order[r] for r in where]] if where else np.zeros((0, G), np.float32)
            for ti, thr in enumerate(thresholds):
                rec_state[b, ti, where] = walk(ious, boxes, gi[b], thr, events)
    return rec_class, rec_score, rec_det, rec_state, rec_count, events


# ------------------------------------------------------------------------------------------------ AP, dataset level
def _curve(scores, states, npos):
    """float64 (recall, precision) of one class at one threshold: stable sort by descending score, ignored records
    removed, cumulative sums."""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    kept = [states[i] for i in order if states[i] != IGNORED]
    tp = np.cumsum([1 if s == TP else 0 for s in kept]).astype(np.float64) if kept else np.zeros((0,), np.float64)
    fp = np.cumsum([1 if s == FP else 0 for s in kept]).astype(np.float64) if kept else np.zeros((0,), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return tp / np.float64(npos), tp / (tp + fp)


def ap_voc07(recall, precision):
    total = 0.0
    for t in np.linspace(0, 1, 11):
        total += max([float(p) for r, p in zip(recall, precision) if r >= t], default=0.0)
    return total / 11


def ap_voc10(recall, precision):
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision, [0.0]])
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    return float(sum((mrec[i + 1] - mrec[i]) * mpre[i + 1] for i in range(len(mrec) - 1) if mrec[i + 1] != mrec[i]))


def ap_coco(recall, precision):
    env = np.array(precision, np.float64)
    for i in range(len(env) - 2, -1, -1):
        env[i] = max(env[i], env[i + 1])
    q = np.zeros((101,), np.float64)
    for k, i in enumerate(np.searchsorted(recall, np.linspace(0, 1, 101), side="left")):
        if i < len(env):
            q[k] = env[i]
    return float(np.mean(q))


AP_FUNCTIONS = {"voc07": ap_voc07, "voc10": ap_voc10, "coco": ap_coco}


def oracle_result(batches, labels, protocol):
    """The result dict of a whole dataset: ``batches`` is a list of ``(pb, pl, ps, gt, gl, gi-or-None)``.  Same layout
    as ``utils.eval_utils.DetectionEvaluator.result()``.  Also returns the summed events."""
    rule, thresholds = PROTOCOLS[protocol]
    NT = len(thresholds)
    L = len(labels)
    npos = [0] * L
    per_class = {c: ([], [[] for _ in range(NT)]) for c in range(1, L)}
    events = dict.fromkeys(CASES, 0)
    for pb, pl, ps, gt, gl, gi in batches:
        gl = np.asarray(gl)
        flags = np.zeros(gl.shape, bool) if gi is None else np.asarray(gi).astype(bool)
        for c in gl[(gl > 0) & ~flags].ravel().tolist():
            npos[c] += 1
        rc, rs, _, rst, rn, ev = oracle_records(pb, pl, ps, gt, gl, gi, rule, thresholds)
        for k in ev:
            events[k] += ev[k]
        for b in range(len(rn)):
            for r in range(int(rn[b])):
                scores, states = per_class[int(rc[b, r])]
                scores.append(rs[b, r])
                for ti in range(NT):
                    states[ti].append(int(rst[b, ti, r]))
    classes = {}
    for c in range(1, L):
        scores, states = per_class[c]
        curves = [_curve(scores, states[ti], npos[c]) for ti in range(NT)]
        aps = np.array([AP_FUNCTIONS[protocol](*cv) if npos[c] > 0 else np.nan for cv in curves], np.float64)
        rec = {"label": labels[c], "npos": npos[c], "AP": float(np.mean(aps)) if npos[c] > 0 else float("nan")}
        if protocol == "coco":
            rec.update(recall=[cv[0] for cv in curves], precision=[cv[1] for cv in curves], AP_per_threshold=aps)
        else:
            rec.update(recall=curves[0][0], precision=curves[0][1])
        classes[c] = rec
    counted = [c for c in classes if npos[c] > 0]

    def mean(v):
        return float(np.mean(v)) if len(v) else float("nan")
    out = {"protocol": protocol, "iou_thresholds": thresholds.copy(), "classes": classes,
           "mAP": mean([classes[c]["AP"] for c in counted])}
    if protocol == "coco":
        out["AP_per_threshold"] = np.array([mean([classes[c]["AP_per_threshold"][ti] for c in counted]) for ti in range(NT)])
        out["AP50"], out["AP75"] = float(out["AP_per_threshold"][0]), float(out["AP_per_threshold"][5])
    return out, events


def assert_results_equal(got, ref):
    """Float64 equality throughout (NaN == NaN): mAP, per-class AP / npos / curves, and the COCO extras."""
    def same(a, b, what):
        np.testing.assert_array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), err_msg=str(what))
    assert got["protocol"] == ref["protocol"]
    same(got["iou_thresholds"], ref["iou_thresholds"], "iou_thresholds")
    same(got["mAP"], ref["mAP"], "mAP")
    assert sorted(got["classes"]) == sorted(ref["classes"])
    for c, want in ref["classes"].items():
        have = got["classes"][c]
        assert have["label"] == want["label"] and have["npos"] == want["npos"], c
        same(have["AP"], want["AP"], ("AP", c))
        if ref["protocol"] == "coco":
            assert len(have["recall"]) == len(want["recall"]) == len(have["precision"])
            for ti in range(len(want["recall"])):
                same(have["recall"][ti], want["recall"][ti], ("recall", c, ti))
                same(have["precision"][ti], want["precision"][ti], ("precision", c, ti))
            same(have["AP_per_threshold"], want["AP_per_threshold"], ("AP_per_threshold", c))
        else:
            same(have["recall"], want["recall"], ("recall", c))
            same(have["precision"], want["precision"], ("precision", c))
    if ref["protocol"] == "coco":
        for k in ("AP_per_threshold", "AP50", "AP75"):
            same(got[k], ref[k], k)


# ------------------------------------------------------------------------------------------------ inputs
# The planted scene: six ground-truth boxes and eleven detection rows on a 1/8 grid (every coordinate, area and the
# IoUs 0.5 and 1 exact in fp32).  Classes 1 and 2 have boxes, class 3 has none.
#   g0 A  = [0,0,.5,.5]   class 1        g1 B = [0,.5,.5,1] class 1 (beside A, no overlap)
#   g2 C  = [.5,0,1,.5]   class 2        g3 C2 = [.5,0,1,.75] class 2 (contains C: IoU 2/3)
#   g4 I  = [.5,.75,1,1]  class 2, IGNORED (apart from C and C2)
#   g5 Z  = [0,0,0,0]     class 1, zero area: IoU NaN against a zero-area detection at the origin, else 0
SCENE_GT = np.array([[0, 0, .5, .5], [0, .5, .5, 1], [.5, 0, 1, .5], [.5, 0, 1, .75], [.5, .75, 1, 1], [0, 0, 0, 0]], np.float32)
SCENE_GL = np.array([1, 1, 2, 2, 2, 1], np.int32)
SCENE_GI = np.array([0, 0, 0, 0, 1, 0], np.uint8)
# rows in descending score (rows 4 and 5 tie; row 1 is a label-0 padding row with the highest score of all)
SCENE_ROWS = [
    # box, label, score                       record  VOC@.5  COCO@.5  VOC@.75  COCO@.75
    ([0, 0, .5, 1], 1, .99),                # r0: A u B, IoU .5 with A and with B (tie, exactly at the threshold)
    ([.25, .25, .75, .75], 0, 1.0),         # label 0: no record
    ([0, 0, .5, .5], 1, .98),               # r1: A.  VOC: A went to r0 -> FP.  COCO: r0 took B -> TP
    ([0, .5, .5, 1], 1, .97),               # r2: B.  VOC: free -> TP.  COCO: taken, nothing else -> FP
    ([.5, 0, 1, .5], 2, .96),               # r3: C -> TP
    ([.5, 0, 1, .5], 2, .96),               # r4: C again, tied score.  VOC: duplicate -> FP.  COCO: C2 at 2/3 -> TP
    ([.5, 0, 1, .5], 2, .95),               # r5: C again: a duplicate under both rules
    ([.5, .75, 1, 1], 2, .94),              # r6: I -> ignored
    ([.5, .75, 1, 1], 2, .93),              # r7: I again.  VOC: ignored again.  COCO: I is taken -> FP
    ([.125, .125, .375, .375], 3, .92),     # r8: class 3 has no box -> FP
    ([0, 0, 0, 0], 1, .91),                 # r9: zero area: NaN against Z, 0 against A and B -> FP
]
SCENE_STATES = {            # worked out by hand from the two rules; thresholds (0.5, 0.75)
    "voc": [[1, 0, 1, 1, 0, 0, -1, -1, 0, 0], [0, 1, 1, 1, 0, 0, -1, -1, 0, 0]],
    "coco": [[1, 1, 0, 1, 1, 0, -1, 0, 0, 0], [0, 1, 1, 1, 0, 0, -1, 0, 0, 0]],
}
SCENE_DETS = [0, 2, 3, 4, 5, 6, 7, 8, 9, 10]       # the detection row behind each record
SCENE_MIN = (11, 6, 4)                             # least T, G and class count (background included) the scene needs


def scene():
    """The planted scene alone: ``(pb [1,11,4], pl [1,11], ps [1,11], gt [1,6,4], gl [1,6], gi [1,6])``."""
    pb = np.array([[r[0] for r in SCENE_ROWS]], np.float32)
    pl = np.array([[r[1] for r in SCENE_ROWS]], np.float32)
    ps = np.array([[r[2] for r in SCENE_ROWS]], np.float32)
    return pb, pl, ps, SCENE_GT[None].copy(), SCENE_GL[None].copy(), SCENE_GI[None].copy()


def planted(B, T, G, L, seed=23):
    """A seeded batch ``(pb, pl, ps, gt, gl, gi, names)``.  Every image starts random: jittered copies of its boxes
    (several per box), wrong labels, background boxes, label-0 rows in between, scores on a 1/64 grid (ties), a fifth
    of the boxes ignored, -1 padded ground truth.  Then the cases are written in, as far as the shape has room, and
    ``names`` lists the ones that were:
      image 0 (T >= 11, G >= 6, L >= 4): the scene above, its rows spread over the image's T rows in a seeded order
        that keeps the tied pair's index order; the image's random rows and boxes are relabelled to classes >= 4;
      image B - 2 (B >= 3, T >= 1): every label 0 -> no record;
      image B - 1 (B >= 3, T >= 1): ground truth all padding -> every record an FP."""
    rng = np.random.default_rng(seed)
    pb = np.zeros((B, T, 4), np.float32); pl = np.zeros((B, T), np.float32); ps = np.zeros((B, T), np.float32)
    gt = np.zeros((B, G, 4), np.float32); gl = np.full((B, G), -1, np.int32); gi = np.zeros((B, G), np.uint8)
    for b in range(B):
        g = int(rng.integers(1, G + 1))
        c = rng.uniform(0.15, 0.85, (g, 2)); s = rng.uniform(0.08, 0.5, (g, 2))
        gt[b, :g] = np.clip(np.concatenate([c - s / 2, c + s / 2], -1), 0, 1)
        gl[b, :g] = rng.integers(1, L, g) if L > 1 else 1
        gi[b, :g] = rng.random(g) < 0.2
        for t in range(T):
            u = rng.random()
            if u < 0.1:
                continue                                    # a label-0 row, zeros
            if u < 0.75:
                j = int(rng.integers(0, g))
                pb[b, t] = np.clip(gt[b, j] + rng.normal(0, 0.03, 4), 0, 1)
                pl[b, t] = gl[b, j] if rng.random() < 0.8 or L <= 2 else rng.integers(1, L)
            else:
                c2 = rng.uniform(0.1, 0.9, 2); s2 = rng.uniform(0.05, 0.3, 2)
                pb[b, t] = np.clip(np.concatenate([c2 - s2 / 2, c2 + s2 / 2]), 0, 1)
                pl[b, t] = rng.integers(1, L) if L > 1 else 1
            ps[b, t] = np.float32(rng.integers(1, 64)) / np.float32(64)
    names = []
    if T >= SCENE_MIN[0] and G >= SCENE_MIN[1] and L >= SCENE_MIN[2] and B >= 1:
        rows = np.sort(rng.choice(T, len(SCENE_ROWS), replace=False))
        perm = rng.permutation(len(SCENE_ROWS))
        i4, i5 = int(np.flatnonzero(perm == 4)[0]), int(np.flatnonzero(perm == 5)[0])
        if i4 > i5:                                         # rows 4 and 5 are the same detection: keep 4 in front
            perm[i4], perm[i5] = 5, 4
        # the image's random rows and boxes move to the classes 4.. (L >= 5; else they become padding): the scene's
        # classes 1..3 are left to the scene
        if L >= 5:
            pl[0] = np.where(pl[0] != 0, 4 + pl[0] % (L - 4), 0)
            gl[0] = np.where(gl[0] > 0, 4 + gl[0] % (L - 4), -1)
        else:
            pl[0], gl[0] = 0, -1
        for slot, k in zip(rows, perm):
            pb[0, slot], pl[0, slot], ps[0, slot] = SCENE_ROWS[k]
        gt[0, :6], gl[0, :6], gi[0, :6] = SCENE_GT, SCENE_GL, SCENE_GI
        names += ["duplicate", "second_best", "ignored_match", "ignored_again", "tied_scores", "iou_at_threshold",
                  "iou_tie", "class_without_box", "nan_iou"]
    if B >= 3 and T >= 1:
        pl[B - 2] = 0
        gt[B - 1], gl[B - 1], gi[B - 1] = 0, -1, 0
        pl[B - 1, 0] = max(pl[B - 1, 0], 1)
        names += ["all_label0_image", "all_padding_image"]
    return pb, pl, ps, gt, gl, gi, names


def assert_not_vacuous(names, events_voc, events_coco, thresholds):
    """On the ORACLE's walks: every planted case was met at least once.  ``second_best`` is the case where the rules
    must disagree, so it is counted on the COCO walk (under VOC such a detection is a plain duplicate); ``iou_tie``
    and ``iou_at_threshold`` need the threshold 0.5 among ``thresholds``."""
    missing = []
    for name in names:
        if name in ("iou_tie", "iou_at_threshold") and 0.5 not in [float(t) for t in thresholds]:
            continue
        if name == "second_best":
            ok = events_coco[name] >= 1 and events_voc["duplicate"] >= 1
        else:
            ok = events_voc[name] >= 1 and events_coco[name] >= 1
        if not ok:
            missing.append((name, events_voc[name], events_coco[name]))
    assert not missing, missing
