"""The batched augmentation cases (tests/augment_batch_cases.py) and the oracle function they go through
(oracle/augment_oracle.apply_plan), without a GPU: ``apply_plan`` is the existing ``geometry`` then ``color`` bit for bit
and keeps test_augment.py's known answers; the case lists hold the flag values, geometry kinds and counts the GPU test
relies on; and the cases cannot pass by accident -- handing image b any OTHER image's geometry row, fill colour, colour
row, flags or pivot changes its reference pixels whenever the two differ in something b's plan reads, every one of the
five is read by at least four images, and a STRIDE output whose pixels past the grid's first trip were left unwritten
differs from the reference."""
import numpy as np
import pytest

import augment_batch_cases as bc
from oracle import augment_oracle as ao

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ apply_plan
@pytest.mark.parametrize("case", [
    # test_augment.py's geometry cases: (H, W, expand (ratio, u_left, u_top) or None, window or None, flip)
    (40, 56, None, None, True),
    (40, 56, None, (3, 7, 20, 33), False),
    (40, 56, (2.37, 0.31, 0.77), (11, 20, 55, 70), False),
    (40, 56, (3.9, 0.0, 0.999), (0, 0, 156, 218), True),
    (37, 29, (1.5, 0.2, 0.4), (5, 3, 41, 37), True),
    (37, 29, None, None, False),
])
@pytest.mark.parametrize("draws", [
    dict(), dict(contrast=1.37), dict(brightness=-0.12, contrast=0.5, hue=0.05, saturation=1.2), dict(hue=0.08, saturation=1.5),
])
def test_apply_plan_is_geometry_then_color(case, draws):
    H, W, expand, window, flip = case
    x = bc.images(1, H, W, seed=H + W)[0]
    g = bc.ground_truth(1, seed=1)[0]
    plan = {"canvas": ao.expand_geometry(H, W, *expand) if expand is not None else (H, W, 0, 0), "crop": window, "flip": flip,
            "expand": expand is not None, "brightness": None, "contrast": None, "hue": None, "saturation": None}
    plan.update(draws)
    ref_img, ref_g = ao.geometry(x, g, expand=expand, crop=window, flip=flip)
    want = ao.color(ref_img, **draws)
    got, gg, fill, pivot = ao.apply_plan(x, g, plan)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    np.testing.assert_array_equal(_bits(gg), _bits(ref_g))
    assert (fill is None) == (expand is None) and (pivot is None) == ("contrast" not in draws)
    if fill is not None:
        np.testing.assert_array_equal(fill, x.astype(np.float64).mean((0, 1)).astype(F32))
    if pivot is not None:
        lit = ref_img + F32(draws["brightness"]) if "brightness" in draws else ref_img
        np.testing.assert_array_equal(pivot, lit.astype(np.float64).mean((0, 1)).astype(F32))
    # the means handed back in reproduce the pixels; other means give other pixels
    again = ao.apply_plan(x, g, plan, fill=fill, pivot=pivot)[0]
    np.testing.assert_array_equal(_bits(again), _bits(got))
    if pivot is not None:
        assert (_bits(ao.apply_plan(x, g, plan, fill=fill, pivot=pivot + F32(0.01))[0]) != _bits(got)).any()


def test_apply_plan_known_answers():
    """The hand-computed answers of test_augment.py::test_oracle_known_answers, through ``apply_plan``."""
    none = {"brightness": None, "contrast": None, "hue": None, "saturation": None}
    g = np.array([[0.1, 0.2, 0.5, 0.6]], F32)
    x = np.random.default_rng(0).random((10, 20, 3), dtype=np.float32)
    fi, fg, _, _ = ao.apply_plan(x, g, dict(none, canvas=(10, 20, 0, 0), crop=None, flip=True, expand=False))
    np.testing.assert_array_equal(fi[:, 0], x[:, 19])
    np.testing.assert_allclose(fg, [[0.1, 0.4, 0.5, 0.8]], rtol=0, atol=1e-7)          # (y1, 1 - x2, y2, 1 - x1)
    # ratio 2, u = 0.5: a 20 x 40 canvas with the image at (5, 10); its own rectangle as the window gives the image back
    assert ao.expand_geometry(10, 20, 2.0, 0.5, 0.5) == (20, 40, 5, 10)
    back, bg, fill, _ = ao.apply_plan(x, g, dict(none, canvas=(20, 40, 5, 10), crop=(5, 10, 10, 20), flip=False, expand=True))
    np.testing.assert_array_equal(back, x)
    np.testing.assert_allclose(bg, g, atol=1e-6)
    np.testing.assert_array_equal(fill, ao.expand_image(x, g, 2.0, 0.5, 0.5)[2])
    # the canvas's top left quarter is fill except its last pixel: resized 10 x 20 -> 10 x 20, the corner is the fill colour
    corner, cg, _, _ = ao.apply_plan(x, g, dict(none, canvas=(20, 40, 5, 10), crop=(0, 0, 10, 20), flip=False, expand=True),
                                     fill=[0.25, 0.5, 0.75])
    np.testing.assert_array_equal(corner[0, 0], [0.25, 0.5, 0.75])
    np.testing.assert_array_equal(corner[5:, 10:], x[:5, :10])
    # a box at (0.1, 0.2, 0.5, 0.6) of the image sits at (0.3, 0.35, 0.5, 0.55) of the canvas, (0.6, 0.7, 1, 1) of its quarter
    np.testing.assert_allclose(cg, [[0.6, 0.7, 1.0, 1.0]], atol=1e-6)
    # the final clip runs without any colour operation; brightness is not clipped before contrast
    wide = x * F32(1.5) - F32(0.2)
    out = ao.apply_plan(wide, g, dict(none, canvas=(10, 20, 0, 0), crop=None, flip=False, expand=False))[0]
    np.testing.assert_array_equal(out, np.clip(wide, 0, 1))
    with pytest.raises(ValueError):
        ao.apply_plan(x, g, dict(none, canvas=(20, 40, 5, 10), crop=None, flip=False, expand=True))


# ------------------------------------------------------------------------------------------------------------- the cases
def test_mixed_holds_what_it_promises():
    case = bc.mixed()
    B, H, W = case.images.shape[:3]
    assert (B, H, W) == (16, 23, 37) and case.boxes.shape == (16, 5, 4) and len(case.plans) == 16
    geom, color, flags, add = bc.arrays(case)
    assert sorted(flags.tolist()) == list(range(16))                               # every colour flag value once
    for k, n in bc.KINDS.items():
        assert case.kinds.count(k) >= n, k
    assert len({tuple(r) for r in geom.tolist()}) >= 13 and len({tuple(r) for r in color.tolist()}) == 16
    assert all(case.plans[a] != case.plans[b] for a in range(B) for b in range(a))     # all plans different
    for b, (k, p) in enumerate(zip(case.kinds, case.plans)):
        ch, cw, pt, pl = p["canvas"]
        top, left, bottom, right = pt, pl, pt + H, pl + W                          # the image on its canvas
        assert H <= ch <= 4 * H and W <= cw <= 4 * W and 0 <= pt <= ch - H and 0 <= pl <= cw - W
        assert p["expand"] == (k in "efghj") and (p["crop"] is None) == (k in "ab") and p["flip"] == (k in "bdf")
        assert p["expand"] or (ch, cw, pt, pl) == (H, W, 0, 0)
        if p["crop"] is None:
            continue
        y, x, h, w = p["crop"]
        assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= ch and x + w <= cw
        inside = top <= y and left <= x and y + h <= bottom and x + w <= right
        apart = y + h <= top or y >= bottom or x + w <= left or x >= right
        if k in "ef":                                                              # across the border: fill and pixels
            assert not inside and not apart
        if k == "g":
            assert apart
        if k == "h":
            assert (y, x, h, w) == (0, 0, ch, cw)
        if k == "i":
            assert (h, w) == (1, 1)
        if k == "j":
            assert (pt, pl) == (0, 0) and not inside and not apart
        assert not (p["expand"] and inside)                                        # an expanding plan reads its fill colour
    assert sum(p["expand"] for p in case.plans) >= 4
    assert sum(p["contrast"] is not None and p["brightness"] is not None for p in case.plans) >= 4
    assert (add[(flags & 1) != 0] != 0).all() and (add[(flags & 1) == 0] == 0).all()
    for b in range(B):                                                             # black, white, grey, one saturated colour
        np.testing.assert_array_equal(case.images[b, 0, :4], np.array([[0, 0, 0], [1, 1, 1], [0.3, 0.3, 0.3], [1, 0, 0.5]], F32))
    # the arrays and the plans are the same thing (the draws are float32 values)
    for b in range(B):
        assert bc.plan_of(geom[b], color[b], flags[b], H, W) == case.plans[b]


def test_stride_and_resized_hold_what_they_promise():
    case = bc.stride()
    B, H, W = case.images.shape[:3]
    assert B * H * W > bc.ONE_TRIP == 4194304 and (B - 1) * H * W < bc.ONE_TRIP       # the smallest batch of this size
    geom, color, flags, add = bc.arrays(case)
    assert (flags == 15).all() and (geom[:, 8] == 1).all() and (geom[:, 9] == 1).all()
    assert len({tuple(r) for r in geom.tolist()}) == B and all(len(set(color[:, i].tolist())) == B for i in range(4))
    assert (geom[:, 4] + geom[:, 6] <= H).all() and (geom[:, 5] + geom[:, 7] <= W).all() and (geom[:, 4:6] >= 0).all()
    r = bc.resized()
    assert r.images.shape == (3, 24, 31, 3) and all(p["crop"] is not None for p in r.plans)
    assert sum(p["expand"] for p in r.plans) == 1 and bc.RESIZED_SIZES == ((40, 17), (9, 50))
    for b, p in enumerate(r.plans):
        y, x, h, w = p["crop"]
        assert 0 <= y and 0 <= x and y + h <= p["canvas"][0] and x + w <= p["canvas"][1]


def _expected_to_differ(kind, mine, other, H, W, constant):
    """Do image ``mine``'s pixels depend on the difference between its own input ``kind`` and image ``other``'s?  From the
    plans alone.  (geom, color, flags) rows of the two images; ``constant``: the geometry output of ``mine`` is one colour
    (a window in the fill region, a 1 x 1 window)."""
    (g, c, f), (g2, c2, f2) = mine, other
    if kind == "geometry":          # without use_crop the kernel reads the flip bit and nothing else of the row
        return tuple(g) != tuple(g2) if g[9] or g2[9] else g[8] != g2[8]
    if kind == "fill":              # read by a plan that expands (test_mixed_holds...: its window is never all image)
        return bool(g[9]) and tuple(g[:4]) != (H, W, 0, 0)
    if kind == "colour":            # the entries its flags select; all draws differ
        return f != 0
    if kind == "flags":             # b's own four draws under other flags: another set of operations, none an identity
        return (f & ~2) != (f2 & ~2) if constant else f != f2       # a one-colour image is its own pivot: contrast keeps it
    if kind == "pivot":
        return bool(f & 2)
    raise AssertionError(kind)


def test_mixed_swapping_any_per_image_input_shows():
    """A kernel that indexes a per-image array with the wrong b -- image 0's row for everyone, the neighbour's, any other
    -- cannot give MIXED's reference pixels: for every image b and every other image o, b's plan with o's geometry row /
    fill / colour row / flags / pivot in place of its own changes at least one output word, except where the plans say
    that nothing b reads differs (two copy-path or two flip-only images swap geometry rows; contrast is switched on or off
    for an image of one colour, which is its own pivot).  The colour rows hold all four
    draws of their image, so other flags run other operations on it."""
    case = bc.mixed()
    B, H, W = case.images.shape[:3]
    geom, color, flags, add = bc.arrays(case)
    fills, pivots = bc.own_means("MIXED")
    want, _ = bc.reference(case)
    forced, _ = bc.reference(case, fills, pivots)                 # the oracle's own means handed back: the same bits
    np.testing.assert_array_equal(_bits(forced), _bits(want))
    readers = dict.fromkeys(bc.INPUTS, 0)
    for b in range(B):
        rows = (geom[b], color[b], int(flags[b]))
        read = dict.fromkeys(bc.INPUTS, False)
        for o in range(B):
            if o == b:
                continue
            other = (geom[o], color[o], int(flags[o]))
            swapped = {
                "geometry": (bc.plan_of(geom[o], color[b], flags[b], H, W), fills[b], pivots[b]),
                "fill": (case.plans[b], fills[o], pivots[b]),
                "colour": (bc.plan_of(geom[b], color[o], flags[b], H, W), fills[b], pivots[b]),
                "flags": (bc.plan_of(geom[b], color[b], flags[o], H, W), fills[b], pivots[b]),
                "pivot": (case.plans[b], fills[b], pivots[o]),
            }
            for kind, (plan, fill, pivot) in swapped.items():
                got = ao.apply_plan(case.images[b], case.boxes[b], plan, fill=fill, pivot=pivot)[0]
                differs = bool((_bits(got) != _bits(want[b])).any())
                assert differs == _expected_to_differ(kind, rows, other, H, W, case.kinds[b] in "gi"), (kind, b, o, case.kinds[b], case.kinds[o])
                read[kind] |= differs
        for kind in bc.INPUTS:
            readers[kind] += read[kind]
    assert readers["geometry"] == B and readers["flags"] == B
    assert all(n >= 4 for n in readers.values()), readers


def test_stride_second_trip_shows():
    """Pixels from 4 194 304 on are written in the kernels' second trip: a geometry kernel that leaves them unwritten (here:
    zeros, or the input's pixels, under the colour pass) and a colour kernel that does (the geometry output, clipped) both
    differ from the reference there, in most words."""
    case = bc.stride()
    B, H, W = case.images.shape[:3]
    b, first = divmod(bc.ONE_TRIP, H * W)
    assert b == B - 1 and 0 < first < H * W                    # the second trip starts inside the last image
    p = case.plans[b]
    want, _, _, pivot = ao.apply_plan(case.images[b], case.boxes[b], p)
    geo = bc.resized_reference(case, b, H, W)                  # the window resized and flipped, no colour operation
    draws = {k: p[k] for k in ("brightness", "contrast", "hue", "saturation")}
    np.testing.assert_array_equal(_bits(ao.color(geo, pivot=pivot, **draws)), _bits(want))
    tail = want.reshape(-1, 3)[first:]
    for stale in (np.zeros_like(geo), case.images[b]):
        left = geo.reshape(-1, 3).copy()
        left[first:] = stale.reshape(-1, 3)[first:]
        got = ao.color(left.reshape(H, W, 3), pivot=pivot, **draws).reshape(-1, 3)
        np.testing.assert_array_equal(_bits(got[:first]), _bits(want.reshape(-1, 3)[:first]))
        assert (got[first:] != tail).any(-1).mean() > 0.9
    assert (np.clip(geo, 0, 1).reshape(-1, 3)[first:] != tail).any(-1).mean() > 0.9
