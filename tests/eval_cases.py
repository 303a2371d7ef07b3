"""Inputs and oracle-side quantities shared by the detection-scoring tests (tests/test_eval_records_cpu.py,
tests/test_eval_gpu.py) and tests/bench_eval.py.  NumPy + the oracle only: no product code, no device."""
import numpy as np

import helpers
from oracle import bbox_oracle as bo
from oracle import eval_oracle as eo


def labels_for(L):
    return ["bg"] + ["c%d" % i for i in range(1, L)]


def detections(B, T, G, L, seed=17, gt_seed=5):
    """The generator of tests/test_bbox_gpu.py::test_eval_update_stats_vs_oracle for any shape: jittered copies of
    the ground truth (several per box), wrong labels, background boxes, label-0 zero padding rows, -1-padded ground
    truth, rows sorted by score like the decoder's output.  Returns (pb, pl, ps, gt, gl)."""
    rng = np.random.default_rng(seed)
    gt, gl = helpers.gt_inputs(B, G=G, L=L, seed=gt_seed)
    pb = np.zeros((B, T, 4), np.float32); pl = np.zeros((B, T), np.float32); ps = np.zeros((B, T), np.float32)
    for b in range(B):
        g = int((gl[b] > 0).sum())
        n = int(rng.integers(T // 2, T)) if T > 1 else 1
        for t in range(n):
            if rng.random() < 0.7:
                j = int(rng.integers(0, g))
                pb[b, t] = np.clip(gt[b, j] + rng.normal(0, 0.03, 4), 0, 1)
                pl[b, t] = gl[b, j] if rng.random() < 0.8 else rng.integers(1, L)
            else:
                c = rng.uniform(0.1, 0.9, 2); s = rng.uniform(0.05, 0.3, 2)
                pb[b, t] = np.clip(np.concatenate([c - s / 2, c + s / 2]), 0, 1)
                pl[b, t] = rng.integers(1, L)
            ps[b, t] = rng.uniform(0.5, 1.0)
        order = np.argsort(-ps[b, :n])
        pb[b, :n], pl[b, :n], ps[b, :n] = pb[b, order], pl[b, order], ps[b, order]
    return pb, pl, ps, gt, gl


def with_edge_cases(pb, pl, ps, gt, gl):
    """Writes the constructed cases into images 0..4 (B >= 5) of a ``detections`` batch, in place, and returns a
    dict naming where they sit:
      image 0: rows 0 and 1 are exact duplicates (box and label) -> tied best IoU, ascending-index order decides;
      image 1: ground truth [0,0,1,1] alone (the rest padding when G > 1), row 0 = [0,0,0.5,1] with its label: IoU
               exactly 0.5 (all three numbers exact in fp32) -> TP by ``>=``; row 1 = [0,0,1,0.5], same label: the
               same IoU -> tie, eligible but the box is taken; the other rows are small boxes (IoU < 0.5);
      image 2: -1 padding in the last ground-truth slot and a zero-size detection with a non-zero label in the last
               row: NaN against the padding box;
      image 3: every detection has label 0 -> no record;
      image 4: ground truth all padding; last row a zero-size detection with a non-zero label: every IoU NaN, best
               -inf -> FP visited last.
    Rows a shape does not have (T == 1) are left out."""
    B, T = pl.shape
    G = gl.shape[1]
    assert B >= 5
    where = {}
    if T >= 2:
        pb[0, 1], pl[0, 1] = pb[0, 0], pl[0, 0]
        where["duplicate"] = (0, 0, 1)
    rng = np.random.default_rng(99)
    gt[1], gl[1] = 0, -1
    gt[1, 0], gl[1, 0] = (0, 0, 1, 1), 3
    for t in range(T):
        c = rng.uniform(0.1, 0.9, 2)
        pb[1, t] = np.concatenate([c - 0.05, c + 0.05]).astype(np.float32)
        pl[1, t] = float(rng.integers(1, 5))
        ps[1, t] = np.float32(0.9 - 0.001 * t)
    pb[1, 0], pl[1, 0] = (0, 0, 0.5, 1), 3
    where["half"] = (1, 0)
    if T >= 2:
        pb[1, 1], pl[1, 1] = (0, 0, 1, 0.5), 3
        where["half_taken"] = (1, 1)
    gt[2, G - 1], gl[2, G - 1] = 0, -1
    pb[2, T - 1], pl[2, T - 1], ps[2, T - 1] = 0, 2, np.float32(0.55)
    where["degenerate_padded"] = (2, T - 1)
    pl[3] = 0
    gt[4], gl[4] = 0, -1
    pb[4, T - 1], pl[4, T - 1], ps[4, T - 1] = 0, 1, np.float32(0.6)
    if T >= 2:
        pl[4, 0] = max(pl[4, 0], 1)            # at least one ordinary record in front of the -inf one
    where["degenerate_all_padding"] = (4, T - 1)
    return where


def case(B, T, G, L, seed=17):
    pb, pl, ps, gt, gl = detections(B, T, G, L, seed=seed)
    where = with_edge_cases(pb, pl, ps, gt, gl)
    return pb, pl, ps, gt, gl, where


def best_and_arg(pb, gt):
    """reference utils/eval_utils.py:20-22 as the oracle states them: IoU map, best IoU from -inf with a strict
    ``>`` (NaN never wins), first arg-max."""
    B, T = pb.shape[:2]
    G = gt.shape[1]
    iou = np.stack([bo.generate_iou_map(pb[b], gt[b:b + 1])[0] for b in range(B)])
    best = np.full((B, T), -np.inf, np.float32)
    arg = np.zeros((B, T), np.int32)
    for g in range(G):
        better = iou[:, :, g] > best
        best = np.where(better, iou[:, :, g], best)
        arg = np.where(better, g, arg)
    return iou, best, arg


def oracle_records(pb, pl, ps, gt, gl):
    """Per-image records READ OFF ``oracle.eval_oracle.update_stats`` itself: the oracle runs on one image at a time
    with the detection index in place of the score and a ``stats`` whose class ids all share ONE record, so its
    appends -- whatever the class -- land in one list in visit order.  Returns (rec_class, rec_score, rec_tp,
    rec_det [B,T] zero-padded, rec_count [B])."""
    B, T = pl.shape
    L = int(max(pl.max(), gl.max())) + 1
    rec_class = np.zeros((B, T), np.int32); rec_score = np.zeros((B, T), np.float32)
    rec_tp = np.zeros((B, T), np.int32); rec_det = np.zeros((B, T), np.int32); rec_count = np.zeros((B,), np.int32)
    index = np.arange(T, dtype=np.float32)[None]
    for b in range(B):
        shared = {"label": "all", "total": 0, "tp": [], "fp": [], "scores": []}
        eo.update_stats(pb[b:b + 1], pl[b:b + 1], index, gt[b:b + 1], gl[b:b + 1], {c: shared for c in range(1, L)})
        det = np.asarray(shared["scores"], np.int64)
        n = len(det)
        assert [1 - v for v in shared["tp"]] == shared["fp"]
        rec_count[b] = n
        rec_det[b, :n] = det
        rec_tp[b, :n] = shared["tp"]
        rec_class[b, :n] = pl[b, det].astype(np.int32)
        rec_score[b, :n] = ps[b, det]
    return rec_class, rec_score, rec_tp, rec_det, rec_count


def assert_stats_equal(got, ref):
    """``total`` / ``tp`` / ``fp`` / ``scores`` of every class, list for list, element types included."""
    assert sorted(got) == sorted(ref)
    for cid in ref:
        assert got[cid]["total"] == ref[cid]["total"], cid
        assert got[cid]["tp"] == ref[cid]["tp"] and got[cid]["fp"] == ref[cid]["fp"], cid
        assert all(type(v) is int for v in got[cid]["tp"] + got[cid]["fp"]), cid
        assert all(isinstance(v, np.float32) for v in got[cid]["scores"]), cid
        assert len(got[cid]["scores"]) == len(ref[cid]["scores"]), cid
        np.testing.assert_array_equal(np.asarray(got[cid]["scores"], np.float32), np.asarray(ref[cid]["scores"], np.float32))


def assert_not_vacuous(pb, pl, gt, gl, rec_tp, rec_det, rec_count, min_tp, min_fp, want_tie=True, want_taken=True):
    """On the ORACLE's records: enough TPs and FPs, at least one eligible-but-taken detection, at least one tie."""
    B, T = pl.shape
    live = np.arange(T)[None] < rec_count[:, None]
    n_tp = int(rec_tp[live].sum())
    n_fp = int(live.sum()) - n_tp
    assert n_tp >= min_tp and n_fp >= min_fp, (n_tp, n_fp)
    _, best, arg = best_and_arg(pb, gt)
    taken = ties = 0
    for b in range(B):
        n = int(rec_count[b])
        det, tp = rec_det[b, :n], rec_tp[b, :n]
        eligible = (best[b, det] >= 0.5) & (pl[b, det].astype(np.int32) == gl[b, arg[b, det]])
        taken += int((eligible & (tp == 0)).sum())
        assert not (tp[~eligible]).any()
        keys = best[b, det]
        ties += int((keys[1:] == keys[:-1]).sum())
        assert (keys[1:] <= keys[:-1]).all()
    assert (not want_taken or taken >= 1) and (not want_tie or ties >= 1), (taken, ties)
    return n_tp, n_fp, taken, ties
