"""Cases and oracles for the drawing tests (tests/test_drawing_cpu.py, tests/test_drawing_gpu.py,
tests/golden/make_drawing_golden.py).

Two independent statements of what ``draw_bboxes_with_labels`` must produce:
  * ``pillow(case)``: the reference's own PIL call sequence (drawing_utils.py:56-69) -- ``ImageDraw.text`` then
    ``ImageDraw.rectangle(outline, width=3)`` per box, 4-tuple colours on an RGB image -- with the legacy bitmap font;
  * ``restate(case)``: a NumPy painter that replays Pillow's primitives SEQUENTIALLY (glyph boxes pasted in string order,
    the 4 x width strokes of the rectangle), so it shares no rule with the kernel's order-free last-writer walk.
Both start from ``array_to_img``: Keras' ``scale=True`` steps in separately rounded float32 (Keras itself is not
installed here; [3P], restated from its published source).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drawing.npz")

VOC = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse",
       "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]
LABELS = ["bg"] + VOC
WIDTH = 3
PROBS = (0.5, 0.987, 1.0)
FIXTURE_NAMES = ("basic", "thin", "outside", "constant")


def colors(seed=5, n=len(LABELS)):
    """``[n,4]`` like the reference's table (the alpha is dropped on an RGB image)."""
    return np.random.default_rng(seed).integers(0, 256, size=(n, 4), dtype=np.int64)


def image(h, w, kind="unit", seed=0):
    rng = np.random.default_rng([seed, h, w])
    if kind == "constant":
        return np.full((h, w, 3), 0.375, np.float32)
    # multiples of 1/1024: exact in float32, and the committed inputs compress
    x = rng.integers(0, 1025, size=(h, w, 3)).astype(np.float32) / np.float32(1024)
    if kind == "wide":                       # values outside [0, 1]
        x = x * np.float32(6.25) - np.float32(2.5)
    return x


def _case(name, h, w, boxes, labels=None, probs=None, kind="unit", seed=0):
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    T = len(boxes)
    if labels is None:
        labels = [(3 * i + 1) % len(LABELS) for i in range(T)]
    if probs is None:
        probs = [PROBS[i % 3] if i % 4 else 0.001 * ((i * 37) % 1000) for i in range(T)]
    return {"name": name, "img": image(h, w, kind, seed), "boxes": boxes, "labels": np.asarray(labels, np.int32).reshape(T),
            "probs": np.asarray(probs, np.float32).reshape(T), "colors": colors()}


def _random_boxes(rng, n, h, w, lo, hi, margin):
    y1 = rng.integers(-margin, h + margin, n)
    x1 = rng.integers(-margin, w + margin, n)
    return np.stack([y1, x1, y1 + rng.integers(lo, hi + 1, n), x1 + rng.integers(lo, hi + 1, n)], -1)


def cases():
    """boxes are (y1, x1, y2, x2) in pixels, as ``denormalize_bboxes`` hands them to ``draw_bboxes_with_labels``"""
    rng = np.random.default_rng(11)
    out = [
        _case("basic", 32, 48, [(2, 3, 20, 40), (10, 8, 30, 30), (14, 20, 22, 47)]),
        # smaller side 1 and 2, both orientations, at the borders too; sides 3..6 around the 2 * width threshold
        _case("thin", 24, 24, [(3, 2, 4, 20), (8, 2, 10, 20), (12, 3, 22, 4), (12, 8, 22, 10), (0, 0, 1, 1), (22, 21, 24, 23),
                               (15, 12, 18, 16), (5, 14, 9, 19), (16, 17, 21, 23), (-1, 10, 0, 30), (23, 0, 24, 12)]),
        # partly outside on every side, wholly outside, and one that swallows the image
        _case("outside", 32, 48, [(-5, -7, 10, 12), (25, 40, 40, 60), (-4, 20, 8, 60), (20, -10, 45, 9), (-40, -40, -5, -5),
                                  (40, 5, 60, 30), (5, 50, 20, 70), (-2, -2, 33, 49), (-100, -100, 200, 200)]),
        _case("constant", 32, 48, [(4, 4, 28, 44), (9, 10, 11, 30)], kind="constant"),
        _case("wide_range", 36, 52, [(3, 5, 30, 45), (6, 2, 33, 20)], kind="wide", seed=2),
        # zero and negative extents are skipped, whatever their label (drawing_utils.py:63)
        _case("degenerate", 32, 48, [(5, 5, 5, 30), (5, 5, 20, 5), (10, 30, 4, 40), (10, 30, 20, 12), (0, 0, 0, 0), (6, 6, 26, 40),
                                     (12, 20, 12, 20)], labels=[1, 2, 3, 4, 99, 5, -3]),
        # order matters: the same rectangles in two orders, text under and over frames
        _case("overlap", 40, 64, [(4, 4, 30, 50), (6, 6, 28, 48), (2, 20, 38, 34), (5, 8, 17, 60), (5, 8, 17, 60), (4, 4, 30, 50)],
              labels=[1, 2, 3, 4, 5, 6]),
        # the text rectangle leaves the image on the right, at the bottom, at the top and on the left
        _case("text_edges", 40, 60, [(5, 30, 25, 58), (33, 3, 39, 50), (-8, 6, 10, 50), (12, -20, 30, 40), (-12, -3, 4, 20),
                                     (31, 44, 50, 80), (1, 55, 30, 59)]),
        # all 21 names with the three pinned probabilities
        _case("all_labels", 300, 272, [(2 + 14 * i, 3 + (i % 3) * 80, 14 + 14 * i, 110 + (i % 3) * 80) for i in range(21)],
              labels=list(range(21)), probs=[PROBS[i % 3] for i in range(21)]),
        _case("all_labels_shifted", 120, 130, [(1 + 5 * i, 2 + i, 40 + 5 * i, 125 - i) for i in range(21)],
              labels=list(range(21)), probs=[PROBS[(i + 1) % 3] for i in range(21)]),
        _case("t0", 20, 28, np.zeros((0, 4))),
        _case("nonsquare_tall", 91, 37, _random_boxes(rng, 12, 91, 37, -2, 40, 8)),
        _case("nonsquare_wide", 37, 91, _random_boxes(rng, 12, 37, 91, -2, 40, 8)),
        _case("one_pixel_rows", 1, 64, [(0, 2, 1, 30), (-1, 20, 0, 50)]),
        # a storm of small boxes: sides -1..8, every thin shape at every offset to the 64 x 16 tiles
        _case("small_storm", 70, 140, _random_boxes(rng, 200, 70, 140, -1, 8, 4)),
        _case("t200", 300, 300, np.concatenate([_random_boxes(rng, 150, 300, 300, 1, 200, 30),
                                                _random_boxes(rng, 50, 300, 300, 0, 6, 5)])[rng.permutation(200)], seed=4),
    ]
    return out


def array_to_img(img):
    """[3P] Keras ``array_to_img(scale=True)``: float32 throughout, ``astype(uint8)`` truncates."""
    x = np.asarray(img, dtype=np.float32)
    x = x - np.min(x)
    x_max = np.max(x)
    if x_max != 0:
        x = x / x_max
    x = x * np.float32(255)
    return x.astype(np.uint8)


def label_text(case, i):
    return "{0} {1:0.3f}".format(LABELS[int(case["labels"][i])], case["probs"][i])


def drawn(case, i):
    y1, x1, y2, x2 = (int(v) for v in case["boxes"][i])
    return x2 - x1 > 0 and y2 - y1 > 0


# ---- Pillow itself ---------------------------------------------------------------------------------------------------
def pillow_available():
    try:
        import PIL  # noqa: F401
        return True
    except Exception:
        return False


def font():
    from PIL import ImageFont
    return (getattr(ImageFont, "load_default_imagefont", None) or ImageFont.load_default)()


def pillow(case, width=WIDTH):
    from PIL import Image, ImageDraw
    image_ = Image.fromarray(array_to_img(case["img"]), "RGB")
    draw = ImageDraw.Draw(image_)
    f = font()
    for i in range(len(case["boxes"])):
        if not drawn(case, i):
            continue
        y1, x1, y2, x2 = (int(v) for v in case["boxes"][i])
        color = tuple(int(v) for v in case["colors"][int(case["labels"][i])])
        draw.text((x1 + 4, y1 + 2), label_text(case, i), fill=color, font=f)
        draw.rectangle((x1, y1, x2, y2), outline=color, width=width)
    return np.asarray(image_).copy()


def pillow_mask(s):
    """``font.getmask(s)`` as a bool array ``[11, 6 * len(s)]``"""
    from PIL import Image, ImageDraw
    m = font().getmask(s)
    im = Image.new("L", m.size, 0)
    ImageDraw.Draw(im).draw.draw_bitmap((0, 0), m, 255)
    return np.asarray(im) != 0


# ---- the NumPy painter -----------------------------------------------------------------------------------------------
def text_mask(atlas, s):
    """``font.getmask(s)`` from the atlas, the way Pillow builds it: every glyph's ink box pasted opaquely, in order."""
    rows = np.asarray(atlas).view(np.uint8).reshape(96, 16)
    out = np.zeros((11, 6 * len(s)), bool)
    for i, ch in enumerate(s.encode("latin-1")):
        g = ch - 32 if 32 <= ch <= 126 else 95
        bits = (rows[g, :11, None] >> np.arange(7)) & 1                    # [11,7]: columns -1 .. 5
        ys, xs = np.nonzero(bits)
        if not len(ys):
            continue
        r0, r1, c0, c1 = ys.min(), ys.max() + 1, xs.min() - 1, xs.max() - 1
        for c in range(c0, c1 + 1):
            if 0 <= 6 * i + c < out.shape[1]:
                out[r0:r1, 6 * i + c] = bits[r0:r1, c + 1] != 0
    return out


def _paste(canvas, mask, x, y, ink):
    H, W = canvas.shape[:2]
    h, w = mask.shape
    ya, yb, xa, xb = max(y, 0), min(y + h, H), max(x, 0), min(x + w, W)
    if ya < yb and xa < xb:
        canvas[ya:yb, xa:xb][mask[ya - y:yb - y, xa - x:xb - x]] = ink


def _hline(canvas, xa, y, xb, ink):
    H, W = canvas.shape[:2]
    if 0 <= y < H:
        xa, xb = min(xa, xb), max(xa, xb)
        if xb >= 0 and xa < W:
            canvas[y, max(xa, 0):min(xb, W - 1) + 1] = ink


def _vline(canvas, x, ya, yb, ink):
    """Pillow's vertical line from ``ya`` towards ``yb`` in either direction, WITHOUT its end point ``yb`` (measured on
    Pillow 12.2.0; inside a frame of ordinary size the horizontal strokes cover that row, so it only shows on boxes
    thinner than twice the width)."""
    H, W = canvas.shape[:2]
    if 0 <= x < W and ya != yb:
        lo, hi = (ya, yb - 1) if ya < yb else (yb + 1, ya)
        if hi >= 0 and lo < H:
            canvas[max(lo, 0):min(hi, H - 1) + 1, x] = ink


def rectangle(canvas, x0, y0, x1, y1, ink, width=WIDTH):
    """``ImageDraw.rectangle(outline=, width=)``: Pillow's four strokes per unit of width, in its order."""
    for i in range(width):
        _hline(canvas, x0, y0 + i, x1, ink)
        _hline(canvas, x0, y1 - i, x1, ink)
        _vline(canvas, x1 - i, y0 + width, y1 - width + 1, ink)
        _vline(canvas, x0 + i, y0 + width, y1 - width + 1, ink)


def restate(case, atlas, width=WIDTH):
    canvas = array_to_img(case["img"]).copy()
    for i in range(len(case["boxes"])):
        if not drawn(case, i):
            continue
        y1, x1, y2, x2 = (int(v) for v in case["boxes"][i])
        ink = np.asarray(case["colors"][int(case["labels"][i])][:3], np.uint8)
        _paste(canvas, text_mask(atlas, label_text(case, i)), x1 + 4, y1 + 2, ink)
        rectangle(canvas, x1, y1, x2, y2, ink, width)
    return canvas


def draw_bounding_boxes(imgs, boxes, colors_):
    """[3P] ``tf.image.draw_bounding_boxes`` restated from the TF 2.0 kernel (unpinned: TF is not installed here)."""
    out = np.array(imgs, np.float32, copy=True)
    B, H, W, _ = out.shape
    for b in range(B):
        for t in range(boxes.shape[1]):
            c = np.asarray(colors_[t % len(colors_)][:3], np.float32)
            q = boxes[b, t].astype(np.float32)
            r0, r1 = int(q[0] * np.float32(H - 1)), int(q[2] * np.float32(H - 1))
            c0, c1 = int(q[1] * np.float32(W - 1)), int(q[3] * np.float32(W - 1))
            if r0 > r1 or c0 > c1 or r0 >= H or r1 < 0 or c0 >= W or c1 < 0:
                continue
            r0c, r1c, c0c, c1c = max(r0, 0), min(r1, H - 1), max(c0, 0), min(c1, W - 1)
            if r0 >= 0:
                out[b, r0, c0c:c1c + 1] = c
            if r1 < H:
                out[b, r1, c0c:c1c + 1] = c
            if c0 >= 0:
                out[b, r0c:r1c + 1, c0] = c
            if c1 < W:
                out[b, r0c:r1c + 1, c1] = c
    return out


# ---- the ragged batch of the GPU tests -------------------------------------------------------------------------------
def ragged_batch(B=64, size=300, T=200, seed=21):
    """``B`` images with 0..T detections each, padded with zero boxes like ``predict``'s output: normalised float32 boxes,
    float labels and scores.  Returns (imgs, boxes, labels, scores)."""
    rng = np.random.default_rng(seed)
    imgs = np.stack([image(size, size, "unit", seed=100 + b) for b in range(B)])
    boxes = np.zeros((B, T, 4), np.float32)
    labels = np.zeros((B, T), np.float32)
    scores = np.zeros((B, T), np.float32)
    for b in range(B):
        n = [0, T, 1][b] if b < 3 else int(rng.integers(0, T + 1))
        px = _random_boxes(rng, n, size, size, -1, 160 if b % 2 else 12, 20)
        boxes[b, :n] = px.astype(np.float32) / np.float32(size)
        labels[b, :n] = rng.integers(1, len(LABELS), n)
        scores[b, :n] = np.sort(rng.random(n).astype(np.float32))[::-1]
    return imgs, boxes, labels, scores


def batch_case(imgs, boxes, labels, scores, b, cols):
    """image ``b`` of a normalised batch as a case (``denormalize_bboxes``: float32 product, round half to even)"""
    H, W = imgs.shape[1:3]
    scale = np.asarray([H, W, H, W], np.float32)
    return {"name": "batch%d" % b, "img": imgs[b], "boxes": np.rint(boxes[b] * scale).astype(np.int32),
            "labels": labels[b].astype(np.int32), "probs": scores[b], "colors": cols}


def load_fixture():
    """-> ({name: (case, pillow bytes)}, Pillow version that wrote it)"""
    with np.load(GOLDEN) as z:
        out = {}
        for name in FIXTURE_NAMES:
            case = {"name": name, "img": z["img_" + name], "boxes": z["boxes_" + name], "labels": z["labels_" + name],
                    "probs": z["probs_" + name], "colors": z["colors_" + name]}
            out[name] = (case, z["out_" + name])
        return out, str(z["pillow_version"])
