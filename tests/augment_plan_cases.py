"""NumPy restatement of ``ssd_augment_plan`` (include/ssd_hip.h) and the cases its two test files share
(test_augment_plan_cpu.py, test_augment_plan_gpu.py).

Three pieces, written from the header's contract and the reference's ``augmentation.py``, not from the kernel:
a Philox4x32-10 in NumPy uint64 arithmetic, the fixed slot table, and the plan arithmetic in ``np.float32`` scalars with
plain Python loops over the sampler's 100 attempts (sequential "first one that satisfies": the kernel's wave ballot must
give the same window).  Every fp32 operation is one NumPy scalar operation, so it rounds on its own like the kernel's
(compiled without contraction, correctly rounded division and square root)."""
import numpy as np

F32 = np.float32
U64 = np.uint64
M32 = U64(0xffffffff)

PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)

# the slot table: slot -> what its four words are
SLOT_BOOLS_A = 0        # patch?, expand?, flip?, brightness?
SLOT_BOOLS_B = 1        # contrast?, hue?, saturation?, min-overlap index (n = 5)
SLOT_EXPAND = 2         # expansion ratio U[1,4), u_left, u_top, --
SLOT_COLOUR = 3         # brightness U[-0.12,0.12), contrast U[0.5,1.5), hue U[-0.08,0.08), saturation U[0.5,1.5)
SLOT_ATTEMPT0 = 16      # + a: aspect ratio U[0.5,2), height draw, y draw, x draw
ATTEMPTS = 100
MIN_OVERLAPS = np.array([0.1, 0.3, 0.5, 0.7, 0.9], F32)
MAX_BOXES = 512         # the kernel's G limit


def philox4x32_10(counter, key):
    """Random123's Philox4x32 with 10 rounds: counter = 4 words, key = 2 words -> 4 words (Python ints)."""
    c = [U64(int(v) & 0xffffffff) for v in counter]
    k = [U64(int(v) & 0xffffffff) for v in key]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]                 # 32 x 32 -> 64 bits: no overflow in uint64
        c = [((p1 >> U64(32)) ^ c[1] ^ k[0]) & M32, p1 & M32, ((p0 >> U64(32)) ^ c[3] ^ k[1]) & M32, p0 & M32]
        k = [(k[0] + PHILOX_W0) & M32, (k[1] + PHILOX_W1) & M32]
    return [int(v) for v in c]


def words(seed, sample_id, slot):
    seed, sample_id = int(seed) & (2 ** 64 - 1), int(sample_id) & (2 ** 64 - 1)
    return philox4x32_10((sample_id & 0xffffffff, sample_id >> 32, slot, 0), (seed & 0xffffffff, seed >> 32))


def unit(word):
    """u = (word >> 8) * 2^-24 in [0, 1), exact in fp32."""
    return F32(word >> 8) * F32(2.0 ** -24)


def boolean(word):
    return bool(unit(word) > F32(0.5))


def uniform(word, lo, hi):
    return F32(F32(lo) + F32(unit(word) * F32(F32(hi) - F32(lo))))


def below(word, n):
    """An integer in [0, n)."""
    return (int(word) * int(n)) >> 32


def _rint(v):
    return int(np.rint(F32(v)))


def valid_rows(boxes, labels):
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    if labels is not None:
        return np.asarray(labels).reshape(-1) > 0
    return np.array([bool(F32(F32(F32(abs(r[0]) + abs(r[1])) + abs(r[2])) + abs(r[3])) > 0) for r in boxes], bool).reshape(-1)


def _renormalize(box, y_min, x_min, y_max, x_max):
    dy, dx = F32(y_max - y_min), F32(x_max - x_min)
    out = [F32(F32(box[0] - y_min) / dy), F32(F32(box[1] - x_min) / dx), F32(F32(box[2] - y_min) / dy), F32(F32(box[3] - x_min) / dx)]
    return [F32(0) if v < 0 else (F32(1) if v > 1 else v) for v in out]


def rectangles(boxes, ch, cw):
    """Pixel rectangles on a ch x cw canvas: the truncated fp32 product."""
    fch, fcw = F32(ch), F32(cw)
    return [(int(F32(b[0] * fch)), int(F32(b[1] * fcw)), int(F32(b[2] * fch)), int(F32(b[3] * fcw))) for b in boxes]


def attempt(seed, sample_id, a, ch, cw):
    """Attempt ``a`` of the sampler on a ch x cw canvas: (y, x, h, w) or None when the attempt is rejected before the
    overlap test (outside the area range or the canvas)."""
    d = words(seed, sample_id, SLOT_ATTEMPT0 + a)
    fcw = F32(cw)
    area = F32(F32(ch) * fcw)
    min_area, max_area = F32(F32(0.05) * area), F32(F32(1.0) * area)
    aspect = uniform(d[0], 0.5, 2.0)
    min_h = _rint(np.sqrt(F32(min_area / aspect)))
    max_h = _rint(np.sqrt(F32(max_area / aspect)))
    if _rint(F32(max_h) * aspect) > cw:
        max_h = int(F32(F32(F32(fcw + F32(0.5)) - F32(1e-7)) / aspect))
        if _rint(F32(max_h) * aspect) > cw:
            max_h -= 1
    max_h = min(max_h, ch)
    min_h = min(min_h, max_h)
    h = min_h
    if min_h < max_h:
        h += below(d[1], max_h - min_h + 1)
    w = _rint(F32(h) * aspect)
    if F32(w * h) < min_area:
        h += 1
        w = _rint(F32(h) * aspect)
    if F32(w * h) > max_area:
        h -= 1
        w = _rint(F32(h) * aspect)
    wh = F32(w * h)
    if wh < min_area or wh > max_area or w > cw or h > ch or w <= 0 or h <= 0:
        return None
    y = below(d[2], ch - h) if h < ch else 0
    x = below(d[3], cw - w) if w < cw else 0
    return y, x, h, w


def satisfies(window, rects, min_overlap):
    y, x, h, w = window
    for r0, r1, r2, r3 in rects:
        box_area = (r2 - r0) * (r3 - r1)
        if box_area < 1:
            continue
        iy = max(min(r2, y + h) - max(r0, y), 0)
        ix = max(min(r3, x + w) - max(r1, x), 0)
        if F32(F32(iy * ix) / F32(box_area)) >= F32(min_overlap):
            return True
    return False


def plan(seed, sample_id, H, W, boxes, labels=None):
    """One image's plan as a dict: geom [10] int32, color [4] float32, flags, add, info [4] int32, boxes [G,4] float32,
    and, for the tests, ``rects`` (the valid rows' pixel rectangles the sampler saw; None without a patch), ``canvas_boxes``
    (the valid rows after expand) and ``window``."""
    boxes = np.array(boxes, F32).reshape(-1, 4)
    valid = valid_rows(boxes, labels)
    a, b = words(seed, sample_id, SLOT_BOOLS_A), words(seed, sample_id, SLOT_BOOLS_B)
    e, c = words(seed, sample_id, SLOT_EXPAND), words(seed, sample_id, SLOT_COLOUR)
    patch = boolean(a[0]) and bool(valid.any())
    expand = patch and boolean(a[1])
    flip, brightness = boolean(a[2]), boolean(a[3])
    contrast, hue, saturation = boolean(b[0]), boolean(b[1]), boolean(b[2])
    overlap_index = below(b[3], 5)
    ch, cw, pt, pl = H, W, 0, 0
    window, accepted, rects = (0, 0, H, W), -1, None
    g = [[F32(v) for v in row] for row in boxes]
    rows = [i for i in range(len(g)) if valid[i]]
    if patch:
        if expand:
            ratio, fh, fw = uniform(e[0], 1.0, 4.0), F32(H), F32(W)
            final_h, final_w = np.rint(F32(fh * ratio)), np.rint(F32(fw * ratio))
            pad_left = np.rint(F32(unit(e[1]) * F32(final_w - fw)))
            pad_top = np.rint(F32(unit(e[2]) * F32(final_h - fh)))
            ch, cw, pt, pl = int(final_h), int(final_w), int(pad_top), int(pad_left)
            pad_bottom, pad_right = F32(F32(ch) - F32(fh + F32(pt))), F32(F32(cw) - F32(fw + F32(pl)))
            mm = (F32(-F32(pt) / fh), F32(-F32(pl) / fw), F32(F32(pad_bottom + fh) / fh), F32(F32(pad_right + fw) / fw))
            for i in rows:
                g[i] = _renormalize(g[i], *mm)
        canvas_boxes = np.array([g[i] for i in rows], F32).reshape(-1, 4)
        rects = rectangles([g[i] for i in rows], ch, cw)
        window, accepted = (0, 0, ch, cw), ATTEMPTS
        for k in range(ATTEMPTS):                   # sequential: the first attempt that satisfies wins
            win = attempt(seed, sample_id, k, ch, cw)
            if win is not None and satisfies(win, rects, MIN_OVERLAPS[overlap_index]):
                window, accepted = win, k
                break
        y, x, h, w = window
        fch, fcw = F32(ch), F32(cw)
        mm = (F32(F32(y) / fch), F32(F32(x) / fcw), F32(F32(y + h) / fch), F32(F32(x + w) / fcw))
        for i in rows:
            g[i] = _renormalize(g[i], *mm)
    else:
        canvas_boxes = None
    if flip:
        for i in rows:
            g[i] = [g[i][0], F32(F32(1) - g[i][3]), g[i][2], F32(F32(1) - g[i][1])]
    delta = uniform(c[0], -0.12, 0.12) if brightness else F32(0)
    return {
        "geom": np.array([ch, cw, pt, pl, window[0], window[1], window[2], window[3], int(flip), int(patch)], np.int32),
        "color": np.array([delta, uniform(c[1], 0.5, 1.5) if contrast else F32(1), uniform(c[2], -0.08, 0.08) if hue else F32(0),
                           uniform(c[3], 0.5, 1.5) if saturation else F32(1)], F32),
        "flags": np.int32(int(brightness) | 2 * int(contrast) | 4 * int(hue) | 8 * int(saturation)),
        "add": F32(delta),
        "info": np.array([accepted, overlap_index, int(expand), 0], np.int32),
        "boxes": np.array(g, F32).reshape(-1, 4),
        "rects": rects, "canvas_boxes": canvas_boxes, "window": window, "valid": valid,
    }


def plan_batch(seed, sample_ids, H, W, boxes, labels=None):
    """The six arrays of ``ssd_augment_plan`` for a padded batch (boxes [B,G,4], labels [B,G] or None)."""
    boxes = np.asarray(boxes, F32)
    B, G = boxes.shape[0], boxes.shape[1]
    ps = [plan(seed, sample_ids[i], H, W, boxes[i], None if labels is None else np.asarray(labels)[i]) for i in range(B)]
    return {"geom": np.stack([p["geom"] for p in ps]).reshape(B, 10), "color": np.stack([p["color"] for p in ps]).reshape(B, 4),
            "flags": np.array([p["flags"] for p in ps], np.int32), "add": np.array([p["add"] for p in ps], F32),
            "info": np.stack([p["info"] for p in ps]).reshape(B, 4), "boxes": np.stack([p["boxes"] for p in ps]).reshape(B, G, 4),
            "plans": ps}


NAMES = ("geom", "color", "flags", "add", "info", "boxes")


def host_plans(arrays):
    """The device plan's arrays (NumPy) as the list of dicts ``augmentation.run_plans`` takes."""
    out = []
    for q, c, fl, info in zip(arrays["geom"], arrays["color"], arrays["flags"], arrays["info"]):
        out.append({"canvas": tuple(int(v) for v in q[:4]), "crop": tuple(int(v) for v in q[4:8]) if q[9] else None, "flip": bool(q[8]),
                    "expand": bool(info[2]),
                    "brightness": float(c[0]) if fl & 1 else None, "contrast": float(c[1]) if fl & 2 else None,
                    "hue": float(c[2]) if fl & 4 else None, "saturation": float(c[3]) if fl & 8 else None})
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
SEED = 0x5EEDC0DE12345678          # both key words in use


def ground_truth(B, G, seed, n_valid=None):
    """A padded batch: per image 1..min(G, 7) VOC-like boxes (or ``n_valid``), the rest padding -- rows of label -1 with
    all-zero boxes (padded_batch) and rows of label 0 with a non-zero box (a row the label, not the box, marks)."""
    rng = np.random.default_rng(seed)
    boxes, labels = np.zeros((B, G, 4), F32), np.full((B, G), -1, np.int32)
    for b in range(B):
        n = int(rng.integers(1, min(G, 7) + 1)) if n_valid is None else n_valid
        c, s = rng.uniform(0.15, 0.85, (G, 2)), rng.uniform(0.03, 0.35, (G, 2))
        bx = np.clip(np.concatenate([c - s, c + s], 1), 0, 1).astype(F32)
        rows = rng.permutation(G)
        boxes[b, rows[:n]], labels[b, rows[:n]] = bx[rows[:n]], rng.integers(1, 21, n)
        for r in rows[n:n + max((G - n) // 2, 0)]:                      # label 0 over a real-looking box: not valid
            boxes[b, r], labels[b, r] = bx[r], 0
    return boxes, labels


def tiny_ground_truth(G=1):
    """One box of a few thousandths of the image a side: most windows miss it, the sampler runs long or fails."""
    boxes, labels = np.zeros((1, G, 4), F32), np.full((1, G), -1, np.int32)
    boxes[0, 0], labels[0, 0] = [0.481, 0.522, 0.489, 0.531], 7
    return boxes, labels


def edge_ground_truth(G=5):
    """One thin box on the top edge: a window has to start in the first rows to hold it, about one attempt in a hundred
    does -- the accepted attempt is often late, sometimes none is."""
    boxes, labels = np.zeros((1, G, 4), F32), np.full((1, G), -1, np.int32)
    boxes[0, G - 1], labels[0, G - 1] = [0.0, 0.45, 0.03, 0.55], 3
    return boxes, labels


# Sampler outcomes every run must see, found by a search with the restatement (seed SEED, 300 x 300, edge_ground_truth):
# sample id -> the accepted attempt.  64 is the first attempt of the lanes' second pass, 98 close to the last one, 100 the
# fallback to the whole canvas.
LATE_IDS = {49: 70, 91: 66, 206: 64, 213: 98, 17: 100, 384: 100}


def outcome_batch():
    """(H, W, boxes [B,G,4], labels [B,G], ids [B]): the LATE_IDS images, one image with no valid row, and ordinary images
    of both expand values."""
    G = 5
    eb, el = edge_ground_truth(G)
    ob, ol = ground_truth(8, G, seed=41)
    ids = list(LATE_IDS) + [5] + list(range(1000, 1008))
    boxes = np.concatenate([np.repeat(eb, len(LATE_IDS), 0), np.zeros((1, G, 4), F32), ob])
    labels = np.concatenate([np.repeat(el, len(LATE_IDS), 0), np.array([[-1, 0, -1, 0, -1]], np.int32), ol])
    boxes[len(LATE_IDS), 1] = [0.2, 0.2, 0.6, 0.7]            # label 0 over a box: still not a valid row
    return 300, 300, boxes, labels, np.array(ids, np.int64)


# (name, H, W, G, B, ground-truth seed): every listed size occurs -- (H, W) in {(300,300), (37,53), (7,5)}, G in {1, 5, 65},
# B in {1, 3, 70}; ids mix small values and values above 2^32
BIT_CASES = [
    ("300x300_G5_B70", 300, 300, 5, 70, 11),
    ("37x53_G65_B3", 37, 53, 65, 3, 12),
    ("7x5_G1_B1", 7, 5, 1, 1, 13),
    ("7x5_G5_B70", 7, 5, 5, 70, 14),
    ("37x53_G1_B3", 37, 53, 1, 3, 15),
]


def case_ids(B, name):
    base = {"300x300_G5_B70": 0, "37x53_G65_B3": (1 << 32) + 5, "7x5_G1_B1": (1 << 40) + 123, "7x5_G5_B70": (1 << 33) - 35,
            "37x53_G1_B3": (1 << 62) + 9}[name]
    return np.arange(base, base + B, dtype=np.int64)
