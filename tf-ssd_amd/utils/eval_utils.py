"""Host-side mirror of the reference's ``utils/eval_utils.py`` (VOC2007 11-point mAP; SURVEY.md
8f row N2): same function names, arguments and ``stats`` layout.  ``update_stats`` is the host
form (GPU IoU map, ``bbox_utils.generate_iou_map`` -> ``ssd_iou_map``, then a Python walk over the
detections); ``update_stats_device`` does the whole per-image matching in one kernel
(``match_detections`` -> ``ssd_eval_match``) and appends its records with vectorised NumPy
(``stats_from_records``).  Both keep the reference's quirks, which the docstrings name.  Cited
line numbers are the reference's."""
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
