"""Host-side mirror of the reference's ``utils/eval_utils.py`` (VOC2007 11-point mAP; SURVEY.md
8f row N2): same function names, arguments and ``stats`` layout.  ``update_stats`` is the host
form (GPU IoU map, ``bbox_utils.generate_iou_map`` -> ``ssd_iou_map``, then a Python walk over the
detections); ``update_stats_device`` does the whole per-image matching in one kernel
(``match_detections`` -> ``ssd_eval_match``) and appends its records with vectorised NumPy
(``stats_from_records``).  Both keep the reference's quirks, which the docstrings name.  Cited
line numbers are the reference's.  Below them, not in the reference: the VOC devkit's and pycocotools'
matching rules and AP definitions (``match_detections_protocol`` -> ``ssd_eval_match_protocol``,
``DetectionEvaluator``), whose mAP compares with published numbers."""
import numpy as np

from utils import bbox_utils

_IOU_TP = 0.5
# the reference's thresholds are np.arange(0, 1.1, 0.1): 0.30000000000000004, 0.6000000000000001,
# 0.7000000000000001 ... -- a recall of exactly 3/10 does not reach the 4th point (:58)
_RECALL_POINTS = np.arange(0, 1.1, 0.1)


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def init_stats(labels):
    """One record per foreground class id (index 0, the background, is skipped):
    ``{"label", "total", "tp", "fp", "scores"}`` (utils/eval_utils.py:5-17)."""
    return {cid: {"label": name, "total": 0, "tp": [], "fp": [], "scores": []}
            for cid, name in enumerate(labels) if cid != 0}


def update_stats(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, stats):
    """utils/eval_utils.py:19-54.  Quirks kept: detections of an image are visited in descending
    best-IoU order, not score order (:23,33); label 0 marks padding and is skipped (:35-36); a
    detection is a true positive iff best IoU >= 0.5, its label equals the label of that
    ground-truth box, and that box was not matched earlier (:46-48); ground-truth label -1
    is padding and not counted (:27-31)."""
    iou = _host(bbox_utils.generate_iou_map(pred_bboxes, gt_boxes))          # [B, T, G]
    det_label, det_score, gt_label = _host(pred_labels), _host(pred_scores), _host(gt_labels)
    for cid, n in zip(*np.unique(gt_label.ravel(), return_counts=True)):
        if cid != -1:
            stats[int(cid)]["total"] += int(n)
    # [3P] Eigen max / arg-max reducers never select a NaN (0/0 IoU of a degenerate box against padding)
    iou = np.where(np.isnan(iou), -np.inf, iou)
    best_iou, best_gt = iou.max(axis=2), iou.argmax(axis=2)
    visit = np.argsort(-best_iou, axis=1, kind="stable")
    for img in range(best_iou.shape[0]):
        taken = set()
        for t in visit[img]:
            cid = int(det_label[img, t])
            if cid == 0:
                continue
            g = int(best_gt[img, t])
            hit = best_iou[img, t] >= _IOU_TP and cid == int(gt_label[img, g]) and g not in taken
            if hit:
                taken.add(g)
            rec = stats[cid]
            rec["scores"].append(det_score[img, t])
            rec["tp"].append(1 if hit else 0)
            rec["fp"].append(0 if hit else 1)
    return stats


def match_detections(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, stream=None, return_indices=False):
    """The per-image part of ``update_stats`` (utils/eval_utils.py:20-50) in one kernel (``ssd_eval_match``).
    pred_bboxes [B,T,4], pred_labels / pred_scores [B,T], gt_boxes [B,G,4], gt_labels [B,G]: NumPy arrays or
    tensors; device tensors of the right type are used where they are.  ``stream``: the torch stream to enqueue
    on (default: the current one); uploads and output allocations then happen on that stream too.
    Returns device tensors ``(rec_class [B,T] int32, rec_score [B,T] float32, rec_tp [B,T] int32, rec_count [B]
    int32)``: per image its records in the reference's visit order, label-0 rows removed, zeros from the count
    on; ``return_indices`` adds ``rec_det [B,T]``, the detection index behind each record.
    Raises ``ssd_hip.SsdHipUnsupported`` for sizes outside the kernel's limits (include/ssd_hip.h)."""
    import torch
    import ssd_hip as _h
    if stream is not None:
        with torch.cuda.stream(stream):
            return match_detections(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, None, return_indices)
    b, l, s = _h.to_dev(pred_bboxes), _h.to_dev(pred_labels), _h.to_dev(pred_scores)
    g, gl = _h.to_dev(gt_boxes), _h.to_dev(gt_labels, dtype=torch.int32)
    if b.dim() != 3 or b.shape[2] != 4 or g.dim() != 3 or g.shape[2] != 4 or g.shape[0] != b.shape[0] \
            or tuple(l.shape) != tuple(b.shape[:2]) or tuple(s.shape) != tuple(b.shape[:2]) \
            or tuple(gl.shape) != tuple(g.shape[:2]):
        raise ValueError("bad shapes %s / %s / %s / %s / %s" % tuple(tuple(t.shape) for t in (b, l, s, g, gl)))
    B, T, G = b.shape[0], b.shape[1], g.shape[1]
    rec_class = torch.empty((B, T), dtype=torch.int32, device=b.device)
    rec_score = torch.empty((B, T), dtype=torch.float32, device=b.device)
    rec_tp = torch.empty((B, T), dtype=torch.int32, device=b.device)
    rec_det = torch.empty((B, T), dtype=torch.int32, device=b.device) if return_indices else None
    rec_count = torch.empty((B,), dtype=torch.int32, device=b.device)
    _h.check(_h.lib().ssd_eval_match(_h.ptr(b), _h.ptr(l), _h.ptr(s), _h.ptr(g), _h.ptr(gl), B, T, G, _IOU_TP,
                                     _h.ptr(rec_class), _h.ptr(rec_score), _h.ptr(rec_tp), _h.ptr(rec_det),
                                     _h.ptr(rec_count), _h.stream()), "match_detections")
    if return_indices:
        return rec_class, rec_score, rec_tp, rec_count, rec_det
    return rec_class, rec_score, rec_tp, rec_count


def stats_from_records(rec_class, rec_score, rec_tp, rec_count, gt_labels, stats):
    """Appends the records of ``match_detections`` (host arrays: [n,T] each, ``rec_count`` [n]) to ``stats`` in the
    order the reference's loop appends them -- image by image, within an image in record order -- and adds the
    per-class ground-truth totals of ``gt_labels`` (one array, or a list of arrays: padded batches differ in
    width; -1 is padding).  Pure NumPy, one selection per class.  Element types are ``update_stats``'s: Python
    ints in tp / fp, ``np.float32`` scores.  A class id ``stats`` does not hold raises ``KeyError`` before
    anything is appended."""
    rec_class = np.asarray(rec_class)
    rec_score = np.asarray(rec_score, np.float32)
    rec_tp = np.asarray(rec_tp)
    count = np.asarray(rec_count).reshape(-1)
    if rec_class.ndim != 2 or rec_score.shape != rec_class.shape or rec_tp.shape != rec_class.shape \
            or count.shape[0] != rec_class.shape[0]:
        raise ValueError("bad record shapes %s / %s / %s / %s" % (rec_class.shape, rec_score.shape, rec_tp.shape,
                                                                  count.shape))
    parts = gt_labels if isinstance(gt_labels, (list, tuple)) else [gt_labels]
    gt_flat = np.concatenate([_host(p).reshape(-1) for p in parts]) if len(parts) else np.zeros((0,), np.int32)
    gt_ids, gt_n = np.unique(gt_flat[gt_flat != -1], return_counts=True)
    live = np.arange(rec_class.shape[1])[None, :] < count[:, None]      # row-major: image order, then record order
    cls, score, tp = rec_class[live], rec_score[live], rec_tp[live]
    ids = np.unique(cls)
    for cid in list(gt_ids) + list(ids):
        if int(cid) not in stats:
            raise KeyError(int(cid))
    for cid, n in zip(gt_ids, gt_n):
        stats[int(cid)]["total"] += int(n)
    for cid in ids:
        sel = cls == cid
        rec = stats[int(cid)]
        hit = tp[sel].astype(np.int64)
        rec["scores"].extend(list(score[sel]))
        rec["tp"].extend(hit.tolist())
        rec["fp"].extend((1 - hit).tolist())
    return stats


def update_stats_device(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, stats):
    """``update_stats`` with the matching on the GPU: ``match_detections`` + ``stats_from_records``; only the four
    record arrays come back to the host.  Sizes the kernel does not cover take ``update_stats``."""
    import ssd_hip as _h
    try:
        rec = match_detections(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels)
    except _h.SsdHipUnsupported:
        return update_stats(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, stats)
    return stats_from_records(*[t.cpu().numpy() for t in rec], gt_labels, stats)


def calculate_ap(recall, precision):
    """11-point interpolated AP: mean over r in {0, 0.1, .., 1} of the best precision at
    recall >= r, 0 where no such point exists (utils/eval_utils.py:56-64)."""
    recall, precision = np.asarray(recall), np.asarray(precision)
    total = 0.0
    for r in _RECALL_POINTS:
        reachable = precision[recall >= r]
        if reachable.size:
            total += float(np.amax(reachable))
    return total / len(_RECALL_POINTS)


def calculate_mAP(stats):
    """Per class: sort by score, cumulate TP/FP, recall = TP / total, precision = TP / (TP + FP);
    returns ``(stats, mean AP)`` with ``recall``/``precision``/``AP`` added to every record
    (utils/eval_utils.py:66-85).  Kept as in the reference: the sort is ``np.argsort(-scores)`` on
    the float32 score array (NumPy's default, unstable sort decides the order of tied scores);
    a class without ground truth divides by zero (NaN recall -> AP 0) and still enters the mean."""
    per_class = []
    for rec in stats.values():
        scores = np.array(rec["scores"], dtype=np.float32) if len(rec["scores"]) else np.array(rec["scores"])
        order = np.argsort(-scores)
        tp = np.cumsum(np.array(rec["tp"])[order])
        fp = np.cumsum(np.array(rec["fp"])[order])
        with np.errstate(divide="ignore", invalid="ignore"):
            rec["recall"] = tp / rec["total"]
            rec["precision"] = tp / (fp + tp)
        rec["AP"] = calculate_ap(rec["recall"], rec["precision"])
        per_class.append(rec["AP"])
    return stats, np.mean(per_class)


# ---------------------------------------------------------------------------------------------------------------------
# The standard protocols (not in the reference): VOCdevkit's and pycocotools' matching rules and AP definitions.
# Matching runs per batch on the device (``ssd_eval_match_protocol``); the AP reduction runs once per evaluation on
# the host in NumPy, like ``calculate_mAP``.
_RULES = {"voc": 0, "coco": 1}                                  # SSD_EVAL_RULE_*


def protocol_spec(protocol):
    """``(rule, float32 IoU thresholds)`` of ``"voc07"`` / ``"voc10"`` / ``"coco"``; ``ValueError`` for any other name."""
    if protocol in ("voc07", "voc10"):
        return "voc", np.array([0.5], np.float32)
    if protocol == "coco":
        return "coco", np.float32(np.linspace(.5, .95, 10))
    raise ValueError('protocol must be "voc07", "voc10" or "coco", got %r' % (protocol,))


def _check_rule(rule, iou_thresholds):
    if rule not in _RULES:
        raise ValueError('rule must be "voc" or "coco", got %r' % (rule,))
    thr = np.ascontiguousarray(np.asarray(iou_thresholds, np.float32).reshape(-1))
    return _RULES[rule], thr


def match_detections_protocol(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, gt_ignore=None, rule="voc",
                              iou_thresholds=(0.5,), stream=None, return_indices=False):
    """Per-image matching by the devkit's (``rule="voc"``) or pycocotools' (``"coco"``) rule in one kernel
    (``ssd_eval_match_protocol``, include/ssd_hip.h states both rules).  Shapes as ``match_detections``; ``gt_ignore``
    [B,G] (bool / uint8, VOC's "difficult"; ``None``: nothing is ignored); ``iou_thresholds``: 1..10 values.
    Returns device tensors ``(rec_class [B,T] int32, rec_score [B,T] float32, rec_state [B,NT,T] int8 (1 TP, 0 FP, -1
    ignored), rec_count [B] int32)``: per image its records in descending score (equal scores by ascending detection
    index), label-0 rows removed, zeros from the count on; ``return_indices`` adds ``rec_det [B,T]``.
    Raises ``ssd_hip.SsdHipUnsupported`` for sizes outside the kernel's limits, ``ValueError`` for an unknown rule."""
    import ctypes
    import torch
    import ssd_hip as _h
    rule_id, thr = _check_rule(rule, iou_thresholds)
    if stream is not None:
        with torch.cuda.stream(stream):
            return match_detections_protocol(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, gt_ignore, rule,
                                             thr, None, return_indices)
    b, l, s = _h.to_dev(pred_bboxes), _h.to_dev(pred_labels), _h.to_dev(pred_scores)
    g, gl = _h.to_dev(gt_boxes), _h.to_dev(gt_labels, dtype=torch.int32)
    gi = None
    if gt_ignore is not None:
        if not isinstance(gt_ignore, torch.Tensor):
            gt_ignore = np.ascontiguousarray(np.asarray(gt_ignore)).astype(np.uint8)
        gi = _h.to_dev(gt_ignore, dtype=torch.uint8)
    if b.dim() != 3 or b.shape[2] != 4 or g.dim() != 3 or g.shape[2] != 4 or g.shape[0] != b.shape[0] \
            or tuple(l.shape) != tuple(b.shape[:2]) or tuple(s.shape) != tuple(b.shape[:2]) \
            or tuple(gl.shape) != tuple(g.shape[:2]) or (gi is not None and tuple(gi.shape) != tuple(gl.shape)):
        raise ValueError("bad shapes %s" % " / ".join(str(tuple(t.shape)) for t in (b, l, s, g, gl) + ((gi,) if gi is not None else ())))
    B, T, G, NT = b.shape[0], b.shape[1], g.shape[1], int(thr.shape[0])
    rec_class = torch.empty((B, T), dtype=torch.int32, device=b.device)
    rec_score = torch.empty((B, T), dtype=torch.float32, device=b.device)
    rec_det = torch.empty((B, T), dtype=torch.int32, device=b.device) if return_indices else None
    rec_state = torch.empty((B, max(NT, 0), T), dtype=torch.int8, device=b.device)
    rec_count = torch.empty((B,), dtype=torch.int32, device=b.device)
    _h.check(_h.lib().ssd_eval_match_protocol(
        _h.ptr(b), _h.ptr(l), _h.ptr(s), _h.ptr(g), _h.ptr(gl), _h.ptr(gi), B, T, G, rule_id,
        thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), NT, _h.ptr(rec_class), _h.ptr(rec_score), _h.ptr(rec_det),
        _h.ptr(rec_state), _h.ptr(rec_count), _h.stream()), "match_detections_protocol")
    if return_indices:
        return rec_class, rec_score, rec_state, rec_count, rec_det
    return rec_class, rec_score, rec_state, rec_count


def _iou_fp32(boxes, gt):
    """``pair_iou`` of csrc/ssd_bbox.hip on the host, every operation rounded to float32 on its own: boxes [T,4] against
    gt [G,4] -> [T,G], the bits of ``ssd_iou_map``."""
    p = np.asarray(boxes, np.float32).reshape(-1, 1, 4)
    g = np.asarray(gt, np.float32).reshape(1, -1, 4)
    zero = np.float32(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        garea = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
        parea = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
        inter = np.maximum(np.minimum(p[..., 3], g[..., 3]) - np.maximum(p[..., 1], g[..., 1]), zero) \
            * np.maximum(np.minimum(p[..., 2], g[..., 2]) - np.maximum(p[..., 0], g[..., 0]), zero)
        return (inter / (parea + garea - inter)).astype(np.float32)


def match_detections_protocol_host(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, gt_ignore=None, rule="voc",
                                   iou_thresholds=(0.5,), return_indices=False):
    """``match_detections_protocol`` as a plain NumPy walk, for sizes the kernel refuses and for hosts without a device:
    the same records, as NumPy arrays."""
    rule_id, thr = _check_rule(rule, iou_thresholds)
    pb, pl, ps = _host(pred_bboxes).astype(np.float32), _host(pred_labels), _host(pred_scores).astype(np.float32)
    gt, gl = _host(gt_boxes).astype(np.float32), _host(gt_labels).astype(np.int64)
    gi = np.zeros(gl.shape, bool) if gt_ignore is None else _host(gt_ignore).astype(bool)
    B, T = pl.shape
    NT = thr.shape[0]
    rec_class = np.zeros((B, T), np.int32)
    rec_score = np.zeros((B, T), np.float32)
    rec_det = np.zeros((B, T), np.int32)
    rec_state = np.zeros((B, NT, T), np.int8)
    rec_count = np.zeros((B,), np.int32)
    for img in range(B):
        rows = np.flatnonzero(pl[img] != 0)
        rows = rows[np.argsort(-ps[img, rows], kind="stable")]
        n = len(rows)
        rec_count[img] = n
        rec_det[img, :n] = rows
        rec_class[img, :n] = pl[img, rows].astype(np.int32)
        rec_score[img, :n] = ps[img, rows]
        iou = _iou_fp32(pb[img, rows], gt[img])
        valid = gl[img] > 0
        taken = np.zeros((NT, gl.shape[1]), bool)
        for r in range(n):
            boxes = np.flatnonzero(valid & (gl[img] == rec_class[img, r]))
            if rule_id == _RULES["coco"]:
                boxes = np.concatenate([boxes[~gi[img, boxes]], boxes[gi[img, boxes]]])
            for ti in range(NT):
                if rule_id == _RULES["voc"]:
                    ovmax, jmax = -np.inf, -1
                    for j in boxes:
                        if iou[r, j] > ovmax:
                            ovmax, jmax = iou[r, j], j
                    if jmax < 0 or ovmax < thr[ti]:
                        continue
                    if gi[img, jmax]:
                        rec_state[img, ti, r] = -1
                    elif not taken[ti, jmax]:
                        taken[ti, jmax] = True
                        rec_state[img, ti, r] = 1
                else:
                    best, m = thr[ti], -1
                    for j in boxes:
                        if taken[ti, j]:
                            continue
                        if m >= 0 and not gi[img, m] and gi[img, j]:
                            break
                        if not iou[r, j] >= best:
                            continue
                        best, m = iou[r, j], j
                    if m >= 0:
                        taken[ti, m] = True
                        rec_state[img, ti, r] = -1 if gi[img, m] else 1
    if return_indices:
        return rec_class, rec_score, rec_state, rec_count, rec_det
    return rec_class, rec_score, rec_state, rec_count


def _precision_envelope(precision):
    """The monotone envelope: at every point the best precision at that or any later point."""
    return np.maximum.accumulate(precision[::-1])[::-1] if precision.size else precision


def average_precision(recall, precision, protocol):
    """AP of one class at one IoU threshold from its float64 recall / precision curve.
    ``"voc07"``: mean over r in ``np.linspace(0, 1, 11)`` of the best precision at recall >= r (0 where there is none).
    ``"voc10"``: area under the monotone precision envelope, ``mrec = [0, rec, 1]``, as VOC2010+ computes it.
    ``"coco"``: mean over the 101 recalls ``np.linspace(0, 1, 101)`` of the envelope at the first point whose recall
    reaches it (``np.searchsorted(..., side="left")``), 0 beyond the last recall."""
    recall, precision = np.asarray(recall, np.float64), np.asarray(precision, np.float64)
    if protocol == "voc07":
        total = 0.0
        for r in np.linspace(0, 1, 11):
            reachable = precision[recall >= r]
            if reachable.size:
                total += float(reachable.max())
        return total / 11
    if protocol == "voc10":
        mrec = np.concatenate([[0.0], recall, [1.0]])
        mpre = _precision_envelope(np.concatenate([[0.0], precision, [0.0]]))
        step = np.flatnonzero(mrec[1:] != mrec[:-1])
        return float(np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1]))
    if protocol == "coco":
        env = _precision_envelope(precision)
        at = np.searchsorted(recall, np.linspace(0, 1, 101), side="left")
        q = np.zeros((101,), np.float64)
        q[at < env.size] = env[at[at < env.size]]
        return float(q.mean())
    raise ValueError('protocol must be "voc07", "voc10" or "coco", got %r' % (protocol,))


class DetectionEvaluator(object):
    """Dataset-level detection metrics by a standard protocol.  ``labels``: the class names, background first;
    ``protocol``: ``"voc07"`` (devkit rule, IoU 0.5, 11-point AP), ``"voc10"`` (devkit rule, IoU 0.5, area under the
    envelope) or ``"coco"`` (pycocotools rule, IoU .50:.05:.95, 101-point AP).  ``update`` matches one batch on the
    device and keeps the record tensors where they are; nothing is read back before ``result``."""

    def __init__(self, labels, protocol):
        self.rule, self.iou_thresholds = protocol_spec(protocol)
        self.protocol = protocol
        self.labels = list(labels)
        self.npos = np.zeros((len(self.labels),), np.int64)
        self._pending = []          # device records + their ground truth, not yet read back
        self._records = []          # host (class [n], score [n], state [NT,n]) in (image, record) order

    def update(self, pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, gt_ignore=None, stream=None):
        """One batch: ``ssd_eval_match_protocol`` enqueued on ``stream`` (default: the current one); the records and the
        per-class counts of non-ignored ground truth are collected by ``result``.  Sizes the kernel refuses take the
        NumPy walk at once.  Returns the device record tensors (``None`` after the host walk)."""
        import ssd_hip as _h
        try:
            rec = match_detections_protocol(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, gt_ignore,
                                            self.rule, self.iou_thresholds, stream)
        except _h.SsdHipUnsupported:
            rec = match_detections_protocol_host(pred_bboxes, pred_labels, pred_scores, gt_boxes, gt_labels, gt_ignore,
                                                 self.rule, self.iou_thresholds)
            self.update_from_records(*rec, gt_labels, gt_ignore)
            return None
        self._pending.append((rec, gt_labels, gt_ignore))
        return rec

    def update_from_records(self, rec_class, rec_score, rec_state, rec_count, gt_labels, gt_ignore=None):
        """The host form: records of ``match_detections_protocol`` ([B,T], [B,T], [B,NT,T], [B]) and the batch's
        ground-truth labels (-1 = padding) and ignore flags."""
        rec_class, rec_score = _host(rec_class), _host(rec_score).astype(np.float32)
        rec_state, count = _host(rec_state), _host(rec_count).reshape(-1)
        NT = self.iou_thresholds.shape[0]
        if rec_class.ndim != 2 or rec_score.shape != rec_class.shape or count.shape[0] != rec_class.shape[0] \
                or rec_state.shape != (rec_class.shape[0], NT, rec_class.shape[1]):
            raise ValueError("bad record shapes %s / %s / %s / %s" % (rec_class.shape, rec_score.shape, rec_state.shape,
                                                                      count.shape))
        gl = _host(gt_labels).astype(np.int64)
        counted = gl > 0
        if gt_ignore is not None:
            counted &= ~_host(gt_ignore).astype(bool)
        ids = np.concatenate([gl[counted], rec_class[rec_class != 0].astype(np.int64)])
        if ids.size and (ids.min() < 1 or ids.max() >= len(self.labels)):
            raise KeyError(int(ids.max() if ids.max() >= len(self.labels) else ids.min()))
        self.npos += np.bincount(gl[counted], minlength=len(self.labels))
        live = np.arange(rec_class.shape[1])[None, :] < count[:, None]      # row-major: image order, then record order
        state = np.moveaxis(rec_state, 1, 0)[:, live]                        # [NT, n]
        self._records.append((rec_class[live], rec_score[live], state))

    def _collect(self):
        for rec, gt_labels, gt_ignore in self._pending:
            self.update_from_records(*rec[:4], gt_labels, gt_ignore)
        self._pending = []

    def result(self):
        """``{"protocol", "iou_thresholds", "mAP", "classes": {class id: {"label", "npos", "AP", "recall",
        "precision"}}}``.  Per class: stable sort by descending score of its records in (image, record) order, ignored
        records removed, cumulative sums, ``precision = tp / (tp + fp)`` and ``recall = tp / npos`` in float64.  A class
        without counted ground truth has AP NaN and is left out of the mean (NaN when no class is left).  ``"coco"``:
        ``recall`` / ``precision`` are lists (one curve per threshold), ``AP`` is the mean over the thresholds, every
        class also holds ``"AP_per_threshold"``, and the dict adds ``"AP50"``, ``"AP75"`` and ``"AP_per_threshold"``."""
        self._collect()
        NT = self.iou_thresholds.shape[0]
        cls = np.concatenate([r[0] for r in self._records]) if self._records else np.zeros((0,), np.int32)
        score = np.concatenate([r[1] for r in self._records]) if self._records else np.zeros((0,), np.float32)
        state = np.concatenate([r[2] for r in self._records], 1) if self._records else np.zeros((NT, 0), np.int8)
        classes = {}
        per_thr = np.full((len(self.labels), NT), np.nan, np.float64)
        for cid in range(1, len(self.labels)):
            sel = np.flatnonzero(cls == cid)
            order = sel[np.argsort(-score[sel], kind="stable")]
            npos = int(self.npos[cid])
            recalls, precisions = [], []
            for ti in range(NT):
                st = state[ti, order]
                st = st[st >= 0]
                tp = np.cumsum(st == 1).astype(np.float64)
                fp = np.cumsum(st == 0).astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    recalls.append(tp / np.float64(npos))
                    precisions.append(tp / (tp + fp))
                if npos > 0:
                    per_thr[cid, ti] = average_precision(recalls[-1], precisions[-1], self.protocol)
            rec = {"label": self.labels[cid], "npos": npos,
                   "AP": float(np.mean(per_thr[cid])) if npos > 0 else float("nan")}
            if self.protocol == "coco":
                rec.update(recall=recalls, precision=precisions, AP_per_threshold=per_thr[cid].copy())
            else:
                rec.update(recall=recalls[0], precision=precisions[0])
            classes[cid] = rec
        counted = [cid for cid in classes if classes[cid]["npos"] > 0]

        def mean(values):
            return float(np.mean(values)) if len(values) else float("nan")
        out = {"protocol": self.protocol, "iou_thresholds": self.iou_thresholds.copy(), "classes": classes,
               "mAP": mean([classes[cid]["AP"] for cid in counted])}
        if self.protocol == "coco":
            out["AP_per_threshold"] = np.array([mean(per_thr[counted, ti]) for ti in range(NT)], np.float64)
            out["AP50"], out["AP75"] = float(out["AP_per_threshold"][0]), float(out["AP_per_threshold"][5])
        return out


def evaluate_predictions(dataset, pred_bboxes, pred_labels, pred_scores, labels, batch_size):
    """Walks ``dataset`` (batches of ``(images, gt_boxes, gt_labels)``) alongside the prediction
    arrays, prints ``mAP: <value>`` and returns the stats (utils/eval_utils.py:87-97)."""
    stats = init_stats(labels)
    for i, (_, gt_boxes, gt_labels) in enumerate(dataset):
        rows = slice(i * batch_size, (i + 1) * batch_size)
        update_stats_device(pred_bboxes[rows], pred_labels[rows], pred_scores[rows], gt_boxes, gt_labels, stats)
    stats, mean_ap = calculate_mAP(stats)
    print("mAP: {}".format(float(mean_ap)))
    return stats
