"""The batches test_augment_batch_cpu.py and test_augment_batch_gpu.py share: seeded images, ground truth and one plan per
image (the dicts ``augmentation.run_plans`` takes), the plans as the four arrays the kernels read, and the NumPy reference
of every image (oracle/augment_oracle.apply_plan).  Importable without a GPU.

MIXED    16 images of 23 x 37, all plans different: every colour flag value once, every geometry kind of ``KINDS``.
STRIDE   17 images of 500 x 500 = 4 250 000 pixels, more than the 16384 blocks x 256 threads one trip of the geometry and
         colour kernels' grid covers: the pixels from 4 194 304 on are written in the grid-stride loop's second trip.
RESIZED  3 images of 24 x 31 straight through ``ssd_augment_geometry`` at other output sizes."""
import collections
import functools

import numpy as np

from oracle import augment_oracle as ao

F32 = np.float32
Case = collections.namedtuple("Case", "name images boxes plans kinds draws")
ONE_TRIP = 16384 * 256              # pixels the capped grid covers in one trip (csrc/ssd_data.hip)
INPUTS = ("geometry", "fill", "colour", "flags", "pivot")       # the per-image state the kernels index with b

# geometry kinds: a copy, b flip only, c crop, d crop + flip, e expand + crop across the image border, f = e + flip,
# g expand with the window wholly in the fill region, h expand with the whole canvas as the window, i a 1 x 1 window,
# j expand with pad_top = pad_left = 0
KINDS = {"a": 2, "b": 2, "c": 2, "d": 2, "e": 2, "f": 2, "g": 1, "h": 1, "i": 1, "j": 1}       # at least so many in MIXED

MIXED_H, MIXED_W = 23, 37
# (kind, canvas (final_h, final_w, pad_top, pad_left) or None, window (y, x, h, w) or None, flip, colour flags)
_MIXED = [
    ("a", None, None, False, 6),
    ("a", None, None, False, 9),
    ("b", None, None, True, 0),
    ("b", None, None, True, 3),
    ("c", None, (3, 5, 11, 20), False, 5),
    ("c", None, (0, 10, 23, 19), False, 10),
    ("d", None, (6, 2, 15, 30), True, 12),
    ("d", None, (1, 1, 9, 35), True, 7),
    ("e", (52, 80, 10, 20), (4, 12, 20, 30), False, 11),        # image at rows 10..32, columns 20..56
    ("e", (35, 56, 7, 3), (15, 25, 20, 31), False, 14),         # rows 7..29, columns 3..39: across the bottom right corner
    ("f", (70, 111, 40, 60), (30, 50, 25, 40), True, 15),
    ("f", (46, 74, 0, 30), (10, 20, 30, 40), True, 2),
    ("g", (92, 148, 60, 100), (5, 5, 30, 50), False, 1),        # 4 x 4 times the image, the window far from it
    ("h", (40, 60, 9, 14), (0, 0, 40, 60), False, 13),
    ("i", None, (11, 17, 1, 1), False, 4),
    ("j", (50, 70, 0, 0), (10, 15, 30, 45), False, 8),
]


def images(B, H, W, seed):
    """Random images with the special pixels of test_augment.py's colour test in every one: black, white, grey (hue
    undefined, saturation 0) and one saturated colour."""
    x = np.random.default_rng(seed).random((B, H, W, 3), dtype=np.float32)
    x[:, 0, 0] = [0.0, 0.0, 0.0]
    x[:, 0, 1] = [1.0, 1.0, 1.0]
    x[:, 0, 2] = [0.3, 0.3, 0.3]
    x[:, 0, 3] = [1.0, 0.0, 0.5]
    return x


def ground_truth(B, seed, n=5):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.2, 0.8, (B, n, 2))
    s = rng.uniform(0.05, 0.3, (B, n, 2))
    return np.clip(np.concatenate([c - s, c + s], -1), 0, 1).astype(F32)


def _plan(H, W, canvas, window, flip, flags, draws):
    """``draws`` = (brightness, contrast, hue, saturation) of this image; ``flags`` picks the ones that run."""
    return {"canvas": tuple(canvas) if canvas is not None else (H, W, 0, 0), "crop": window, "flip": bool(flip),
            "expand": canvas is not None,
            "brightness": float(draws[0]) if flags & 1 else None, "contrast": float(draws[1]) if flags & 2 else None,
            "hue": float(draws[2]) if flags & 4 else None, "saturation": float(draws[3]) if flags & 8 else None}


def _colour_draws(B, seed):
    """Per image four draws from the ranges of ``augmentation.draw_plan``, none of them an operation's identity."""
    rng = np.random.default_rng(seed)
    sign = rng.choice([-1.0, 1.0], (B, 4))
    mag = rng.uniform(0.25, 1.0, (B, 4))
    return np.stack([0.12 * sign[:, 0] * mag[:, 0], 1.0 + 0.5 * sign[:, 1] * mag[:, 1], 0.08 * sign[:, 2] * mag[:, 2],
                     1.0 + 0.5 * sign[:, 3] * mag[:, 3]], 1).astype(F32)


@functools.lru_cache(maxsize=None)
def mixed():
    B, H, W = len(_MIXED), MIXED_H, MIXED_W
    draws = _colour_draws(B, seed=101)
    plans = [_plan(H, W, canvas, window, flip, flags, draws[b]) for b, (_, canvas, window, flip, flags) in enumerate(_MIXED)]
    return Case("MIXED", images(B, H, W, seed=100), ground_truth(B, seed=102), plans, tuple(k for k, _, _, _, _ in _MIXED), draws)


@functools.lru_cache(maxsize=None)
def stride():
    B, S = 17, 500
    assert B * S * S > ONE_TRIP
    rng = np.random.default_rng(201)
    draws = _colour_draws(B, seed=202)
    plans = []
    for b in range(B):
        y, x = int(rng.integers(0, 200)), int(rng.integers(0, 200))
        h, w = int(rng.integers(100, 301)), int(rng.integers(100, 301))
        plans.append(_plan(S, S, None, (y, x, h, w), True, 15, draws[b]))
    return Case("STRIDE", images(B, S, S, seed=200), ground_truth(B, seed=203), plans, ("d",) * B, draws)


RESIZED_SIZES = ((40, 17), (9, 50))


@functools.lru_cache(maxsize=None)
def resized():
    """use_crop = 1 on every image, no colour: the second image expands, the third flips."""
    H, W = 24, 31
    rows = [(None, (2, 3, 19, 22), False), ((61, 70, 20, 11), (9, 1, 40, 55), False), (None, (0, 0, 24, 31), True)]
    draws = np.tile(np.array([0, 1, 0, 1], F32), (3, 1))
    plans = [_plan(H, W, canvas, window, flip, 0, draws[b]) for b, (canvas, window, flip) in enumerate(rows)]
    return Case("RESIZED", images(3, H, W, seed=300), ground_truth(3, seed=301), plans, ("c", "e", "d"), draws)


def resized_reference(case, b, out_h, out_w, fill=None):
    """The canvas (filled with ``fill`` or the image's mean), its window resized to out_h x out_w, flipped: the pieces of
    ``apply_plan`` at another output size."""
    p = case.plans[b]
    x, g = case.images[b], case.boxes[b]
    if p["expand"]:
        x, g, _ = ao.expand_canvas(x, g, *p["canvas"], fill=fill)
    x, g, _ = ao.crop_and_resize(x, g, p["crop"][:2], p["crop"][2:], out_h, out_w)
    if p["flip"]:
        x, g = ao.flip_horizontally(x, g)
    return x


# ---------------------------------------------------------------------------------------- plans <-> the kernels' arrays
def arrays(case):
    """A case's plans in the layouts of include/ssd_hip.h: geom int32 [B,10], color float32 [B,4], flags int32 [B], add
    float32 [B] (the brightness delta ``ssd_image_mean`` adds for contrast's pivot, 0 without brightness).  A colour row
    holds ALL FOUR draws of its image, whatever its flags: the kernel reads the flagged ones only (``run_plans`` writes
    0 / 1 / 0 / 1 into the others, an operation's identity, and must give the same pixels), and an image under another
    image's flags runs operations that change it."""
    B = len(case.plans)
    geom, flags = np.zeros((B, 10), np.int32), np.zeros((B,), np.int32)
    for b, p in enumerate(case.plans):
        ch, cw, pt, pl = p["canvas"]
        y, x, h, w = p["crop"] if p["crop"] is not None else (0, 0, ch, cw)
        geom[b] = [ch, cw, pt, pl, y, x, h, w, int(p["flip"]), int(p["crop"] is not None)]
        for i, name in enumerate(("brightness", "contrast", "hue", "saturation")):
            flags[b] |= (1 << i) if p[name] is not None else 0
    color = np.array(case.draws, F32).reshape(B, 4)
    add = np.where(flags & 1, color[:, 0], F32(0)).astype(F32)
    return geom, color, flags, add


def plan_of(geom_row, color_row, flag, H, W):
    """One image's rows back as a plan dict (what a kernel that reads these rows executes)."""
    q = [int(v) for v in geom_row]
    flag = int(flag)
    return {"canvas": tuple(q[:4]) if q[9] else (H, W, 0, 0), "crop": tuple(q[4:8]) if q[9] else None, "flip": bool(q[8]),
            "expand": bool(q[9]) and tuple(q[:4]) != (H, W, 0, 0),
            "brightness": float(color_row[0]) if flag & 1 else None, "contrast": float(color_row[1]) if flag & 2 else None,
            "hue": float(color_row[2]) if flag & 4 else None, "saturation": float(color_row[3]) if flag & 8 else None}


def host_boxes(aug, gt_boxes, plan, H, W):
    """The boxes of the product's host path for a given plan: the box steps of ``augmentation.draw_plan`` in its order."""
    g = np.asarray(gt_boxes, F32)
    ch, cw, pt, pl = plan["canvas"]
    if plan["crop"] is not None:
        if plan["expand"]:
            g = aug.expand_boxes(g, H, W, ch, cw, pt, pl)
        y, x, h, w = plan["crop"]
        g = aug.renormalize(g, np.array([F32(y) / F32(ch), F32(x) / F32(cw), F32(y + h) / F32(ch), F32(x + w) / F32(cw)], F32))
    if plan["flip"]:
        g = aug.flip_boxes(g)
    return g


# ------------------------------------------------------------------------------------------------------------ references
def reference(case, fills=None, pivots=None):
    """``apply_plan`` image by image: (pixels [B,H,W,3], boxes [B,G,4]).  ``fills`` / ``pivots`` [B,3]: the means to force."""
    px, bx = [], []
    for b, p in enumerate(case.plans):
        o, g, _, _ = ao.apply_plan(case.images[b], case.boxes[b], p, fill=None if fills is None else fills[b],
                                   pivot=None if pivots is None else pivots[b])
        px.append(o)
        bx.append(g)
    return np.stack(px), np.stack(bx)


def geometry_output(case, fills=None):
    """The geometry half alone (no colour operation, no clip): what the second ``ssd_image_mean`` launch reads."""
    out = []
    for b, p in enumerate(case.plans):
        if p["crop"] is None:
            out.append(ao.flip_horizontally(case.images[b], case.boxes[b])[0] if p["flip"] else case.images[b])
        else:
            out.append(resized_reference(case, b, case.images.shape[1], case.images.shape[2], None if fills is None else fills[b]))
    return np.stack(out)


def mean_reference(x, add=None):
    """[B,C]: the float64 mean over H, W of the float32 ``x + add[b]``, rounded once to float32."""
    x = np.asarray(x, F32)
    if add is not None:
        x = x + np.asarray(add, F32).reshape(-1, 1, 1, 1)
    return np.stack([ao.channel_mean(v) for v in x])


@functools.lru_cache(maxsize=None)
def own_means(name):
    """(fills, pivots) [B,3] of a case from the oracle alone: every image's mean, and the mean of its geometry output plus
    its brightness delta (0 without brightness) -- the two tensors ``run_plan_device`` computes for the whole batch."""
    case = {"MIXED": mixed, "STRIDE": stride}[name]()
    fills = mean_reference(case.images)
    return fills, mean_reference(geometry_output(case, fills), arrays(case)[3])
