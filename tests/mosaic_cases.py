"""NumPy restatement of the mosaic augmentation (``ssd_augment_mosaic_plan`` / ``ssd_augment_mosaic_pixels``,
include/ssd_hip.h, "augmentation, mosaic") and the cases its two test files share (test_mosaic_cpu.py, test_mosaic_gpu.py).

Written from the header's contract, not from the kernels: the Philox helpers and draw conventions of
tests/augment_plan_cases.py on the slots 128..130, the plan and the ground-truth merge in ``np.float32`` scalars -- one
NumPy scalar operation per fp32 operation, so each rounds on its own like the kernel's (compiled without contraction, with
correctly rounded division) -- in plain sequential loops (tile 0..3, then the source's rows in order: the kernel's ballot and
prefix popcount must give the same rows), and the tile pixels from ``oracle.augment_oracle.resize_bilinear`` of the whole
source image.  Importable without a GPU.

SMALL    8 images of 23 x 37, G = 6, image 1 without a valid row; run at p = 1, at p = 0.5 and at the scale range (0.75, 1.5).
CAP      SMALL at p = 1 with 6 output rows: kept rows are dropped.
STRIDE   17 images of 500 x 500 at p = 1: more pixels than one trip of the pixel kernel's capped grid.
``coverage`` says, from the reference alone, that the cases see what they are for (test_mosaic_cpu.py asserts it)."""
import collections
import functools

import numpy as np

import augment_batch_cases as bc
import augment_plan_cases as pc
from oracle.augment_oracle import resize_bilinear

F32 = np.float32
SEED = pc.SEED
SLOT_DECISIONS = 128    # mosaic?, partner 1, partner 2, partner 3
SLOT_CENTRE = 129       # centre y draw, centre x draw, --, --
SLOT_SCALES = 130       # scale of tile 0, 1, 2, 3
PAD_LABEL = -1          # data_utils.get_padding_values()[2]
FILL = (0.5, 0.5, 0.5)
NAMES = ("plan", "boxes", "labels", "info")
MAX_SIDE, MAX_BOXES, MAX_OUT, MAX_BATCH = 4096, 512, 2048, 65535

Case = collections.namedtuple("Case", "name images boxes labels ids H W p scale max_boxes")
Row = collections.namedtuple("Row", "image tile source row kept clipped written")


def default_rows(G):
    """``max_boxes=None`` of the Python surface."""
    return min(4 * G, 512)


# -------------------------------------------------------------------------------------------------------------- the law
def plan_row(seed, sample_id, b, B, H, W, p, scale):
    """plan_out[b]: {mosaic, yc, xc, 0, then per tile {source, hs, ws}} as a list of 16 ints."""
    d0, d1, d2 = (pc.words(seed, sample_id, s) for s in (SLOT_DECISIONS, SLOT_CENTRE, SLOT_SCALES))
    mosaic = bool(pc.unit(d0[0]) < F32(p))
    fh, fw = F32(H), F32(W)
    yc = min(max(int(F32(fh * F32(F32(0.25) + F32(F32(0.5) * pc.unit(d1[0]))))), 1), H - 1)
    xc = min(max(int(F32(fw * F32(F32(0.25) + F32(F32(0.5) * pc.unit(d1[1]))))), 1), W - 1)
    row = [int(mosaic), yc, xc, 0]
    for t in range(4):
        s = pc.uniform(d2[t], scale[0], scale[1])
        row += [b if t == 0 else pc.below(d0[t], B), max(1, int(np.rint(F32(fh * s)))), max(1, int(np.rint(F32(fw * s))))]
    return row


def placement(row, t, H, W):
    """Tile t of a plan row: (top, left) of the placed image and the tile's rectangle (y_lo, y_hi, x_lo, x_hi)."""
    yc, xc = row[1], row[2]
    hs, ws = row[5 + 3 * t], row[6 + 3 * t]
    lower, right = t >= 2, bool(t & 1)
    return (yc if lower else yc - hs, xc if right else xc - ws), (yc if lower else 0, H if lower else yc, xc if right else 0, W if right else xc)


def _clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def merge(row, b, boxes, labels, H, W, G_out):
    """The ground truth of output image b: (boxes [G_out,4], labels [G_out], info [4], the ``Row`` records of every valid
    source row the rule saw)."""
    G = boxes.shape[1]
    ob, ol = np.zeros((G_out, 4), F32), np.full((G_out,), PAD_LABEL, np.int32)
    if not row[0]:
        ob[:G], ol[:G] = boxes[b], labels[b]
        return ob, ol, np.array([0, 0, G, 0], np.int32), []
    fh, fw = F32(H), F32(W)
    kept = seen = 0
    records = []
    for t in range(4):
        src, hs, ws = row[4 + 3 * t:7 + 3 * t]
        (top, left), (y_lo, y_hi, x_lo, x_hi) = placement(row, t, H, W)
        top, left, fhs, fws = F32(top), F32(left), F32(hs), F32(ws)
        y_lo, y_hi, x_lo, x_hi = F32(y_lo), F32(y_hi), F32(x_lo), F32(x_hi)
        for g in range(G):
            if not labels[src, g] > 0:
                continue
            seen += 1
            y1, x1, y2, x2 = (F32(v) for v in boxes[src, g])
            Y1, X1 = F32(top + F32(y1 * fhs)), F32(left + F32(x1 * fws))
            Y2, X2 = F32(top + F32(y2 * fhs)), F32(left + F32(x2 * fws))
            cy1, cx1, cy2, cx2 = _clip(Y1, y_lo, y_hi), _clip(X1, x_lo, x_hi), _clip(Y2, y_lo, y_hi), _clip(X2, x_lo, x_hi)
            h, w, h0, w0 = F32(cy2 - cy1), F32(cx2 - cx1), F32(Y2 - Y1), F32(X2 - X1)
            keep = bool(h >= F32(2) and w >= F32(2) and F32(w * h) >= F32(F32(0.1) * F32(w0 * h0))
                        and w < F32(F32(100) * h) and h < F32(F32(100) * w))
            written = keep and kept < G_out
            if written:
                ob[kept] = [F32(cy1 / fh), F32(cx1 / fw), F32(cy2 / fh), F32(cx2 / fw)]
                ol[kept] = labels[src, g]
            records.append(Row(b, t, src, g, keep, bool(keep and (cy1 != Y1 or cx1 != X1 or cy2 != Y2 or cx2 != X2)), bool(written)))
            kept += int(keep)
    return ob, ol, np.array([1, kept, min(kept, G_out), seen], np.int32), records


def pixels(row, b, images, fill=FILL):
    """Output image b [H,W,3]: every tile's source resized as a whole (``resize_bilinear``), placed with one corner on the
    centre and cut to the tile's rectangle; ``fill`` elsewhere; not a mosaic: the image itself."""
    _, H, W, _ = images.shape
    if not row[0]:
        return images[b].copy()
    out = np.empty((H, W, 3), F32)
    out[...] = np.asarray(fill, F32)
    for t in range(4):
        src, hs, ws = row[4 + 3 * t:7 + 3 * t]
        (top, left), (y_lo, y_hi, x_lo, x_hi) = placement(row, t, H, W)
        y0, y1, x0, x1 = max(top, y_lo), min(top + hs, y_hi), max(left, x_lo), min(left + ws, x_hi)
        if y0 < y1 and x0 < x1:
            out[y0:y1, x0:x1] = resize_bilinear(images[src], hs, ws)[y0 - top:y1 - top, x0 - left:x1 - left]
    return out


def mosaic_batch(seed, ids, boxes, labels, H, W, p, scale, G_out, images=None, fill=FILL):
    """The four arrays of ``ssd_augment_mosaic_plan`` for a padded batch, ``rows`` (the records of ``merge``) and, with
    ``images``, ``pixels`` [B,H,W,3]."""
    boxes, labels = np.asarray(boxes, F32), np.asarray(labels, np.int32)
    B = boxes.shape[0]
    plan = np.array([plan_row(seed, ids[b], b, B, H, W, p, scale) for b in range(B)], np.int32).reshape(B, 16)
    merged = [merge([int(v) for v in plan[b]], b, boxes, labels, H, W, G_out) for b in range(B)]
    out = {"plan": plan, "boxes": np.stack([m[0] for m in merged]), "labels": np.stack([m[1] for m in merged]),
           "info": np.stack([m[2] for m in merged]), "rows": [r for m in merged for r in m[3]]}
    if images is not None:
        out["pixels"] = np.stack([pixels([int(v) for v in plan[b]], b, images, fill) for b in range(B)])
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
SMALL_B, SMALL_H, SMALL_W, SMALL_G = 8, 23, 37, 6
# sample ids 1000003 * k + 7 with k = the image, but image 5: no image of that batch draws itself as a partner, so image 5
# takes k = 10, the first k beyond 7 at which it does and every other entry of ``coverage`` still holds (found by a search
# with the restatement, as augment_plan_cases.LATE_IDS was)
SELF_PARTNER_IMAGE, SELF_PARTNER_K = 5, 10
SMALL_IDS = np.array([1000003 * (SELF_PARTNER_K if k == SELF_PARTNER_IMAGE else k) + 7 for k in range(SMALL_B)], np.int64)
STRIDE_B, STRIDE_S = 17, 500


def _small_inputs():
    boxes, labels = pc.ground_truth(SMALL_B, SMALL_G, seed=31)
    labels[1][labels[1] > 0] = 0                    # image 1: boxes, but no valid row
    return bc.images(SMALL_B, SMALL_H, SMALL_W, seed=400), boxes, labels


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "STRIDE":
        boxes, labels = pc.ground_truth(STRIDE_B, SMALL_G, seed=32)
        ids = np.array([1000003 * k + 7 for k in range(STRIDE_B)], np.int64) + (1 << 33)
        return Case(name, bc.images(STRIDE_B, STRIDE_S, STRIDE_S, seed=401), boxes, labels, ids, STRIDE_S, STRIDE_S, 1.0, (0.5, 1.0), None)
    images, boxes, labels = _small_inputs()
    p, scale, rows = {"SMALL": (1.0, (0.5, 1.0), None), "SMALL_HALF": (0.5, (0.5, 1.0), None), "SMALL_UP": (1.0, (0.75, 1.5), None),
                      "CAP": (1.0, (0.5, 1.0), SMALL_G)}[name]
    return Case(name, images, boxes, labels, SMALL_IDS, SMALL_H, SMALL_W, p, scale, rows)


CASES = ("SMALL", "SMALL_HALF", "SMALL_UP", "CAP", "STRIDE")


def empty_mosaic_batch(B=4, S=64):
    """(images, boxes, labels): one valid box of well under a pixel a side in every image, so every mosaic of this batch keeps
    NO row -- the law allows it, and whatever runs behind the mosaic has to take an image without a valid row."""
    boxes, labels = np.zeros((B, 1, 4), F32), np.full((B, 1), 5, np.int32)
    boxes[:, 0] = [0.4, 0.4, 0.41, 0.41]
    return bc.images(B, S, S, seed=402), boxes, labels


def rows_out(c):
    return default_rows(c.boxes.shape[1]) if c.max_boxes is None else c.max_boxes


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once and shared; the arrays are read-only."""
    c = case(name)
    ref = mosaic_batch(SEED, c.ids, c.boxes, c.labels, c.H, c.W, c.p, c.scale, rows_out(c), c.images)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def coverage():
    """What the cases hold, from the reference alone: a dict of booleans, every one of which must be True."""
    small, half, up, cap = (mosaic_batch(SEED, case(n).ids, case(n).boxes, case(n).labels, SMALL_H, SMALL_W, case(n).p, case(n).scale,
                                         rows_out(case(n))) for n in ("SMALL", "SMALL_HALF", "SMALL_UP", "CAP"))
    c = case("SMALL")
    rows, plan = small["rows"], small["plan"]
    out = {}
    for t in range(4):
        out["tile %d keeps a row" % t] = any(r.tile == t and r.kept for r in rows)
        out["tile %d drops a row" % t] = any(r.tile == t and not r.kept for r in rows)
    out["a kept row was clipped"] = any(r.clipped for r in rows)

    def shows(row, t):          # (fill visible, source cropped) of tile t
        (top, left), (y_lo, y_hi, x_lo, x_hi) = placement(row, t, c.H, c.W)
        hs, ws = row[5 + 3 * t], row[6 + 3 * t]
        fill = top > y_lo or top + hs < y_hi or left > x_lo or left + ws < x_hi
        crop = top < y_lo or top + hs > y_hi or left < x_lo or left + ws > x_hi
        return fill, crop
    seen = [shows([int(v) for v in plan[b]], t) for b in range(SMALL_B) for t in range(4)]
    out["a tile shows fill"] = any(f for f, _ in seen)
    out["a tile crops its source"] = any(k for _, k in seen)
    out["a source has no valid row"] = not (c.labels[1] > 0).any() and bool((plan[:, 4::3] == 1).any())
    partners = plan[:, 7::3]
    out["a partner repeats"] = any(len(set(partners[b])) < 3 for b in range(SMALL_B))
    out["a partner is the image itself"] = any(b in partners[b] for b in range(SMALL_B))
    out["p = 0.5 gives both kinds"] = bool((half["plan"][:, 0] == 1).any() and (half["plan"][:, 0] == 0).any())
    out["CAP drops a kept row"] = bool((cap["info"][:, 1] > cap["info"][:, 2]).any())
    out["the default rows drop nothing"] = bool((small["info"][:, 1] == small["info"][:, 2]).all())
    out["the upsampling range leaves no fill"] = not any(shows([int(v) for v in up["plan"][b]], t)[0] for b in range(SMALL_B) for t in range(4))
    return out
