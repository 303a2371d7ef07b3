"""The device augmentation plan (``ssd_augment_plan``, include/ssd_hip.h) without a GPU: the NumPy restatement the GPU
tests compare the kernel with (tests/augment_plan_cases.py) is pinned here -- Philox4x32-10 against the published
Random123 known answers, the draw helpers' ranges, the fairness of the seven booleans, the sampler's invariants against the
package's own acceptance rule, and the box arithmetic against the package's ``expand_boxes`` / ``renormalize`` /
``flip_boxes`` bit for bit.  The C entry point and the Python surface are checked for presence (no device needed)."""
import numpy as np

import augment_plan_cases as pc

F32 = np.float32


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    ones = 0xffffffff
    assert pc.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert pc.philox4x32_10((ones,) * 4, (ones,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert pc.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # the counter / key layout of the plan: id and seed split into their 32-bit halves, the slot in word 2
    assert pc.words(0xa4093822 | (0x299f31d0 << 32), 0x243f6a88 | (0x85a308d3 << 32), 0x13198a2e) == \
        pc.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    assert pc.words(-1, -1, 3) == pc.philox4x32_10((ones, ones, 3, 0), (ones, ones))     # int64 ids / seeds wrap to uint64


def test_draw_ranges():
    for w in (0, 1, 0xff, 0x100, 0x7fffffff, 0x80000000, 0x800000ff, 0x80000100, 0xfffffeff, 0xffffff00, 0xffffffff):
        u = pc.unit(w)
        assert u.dtype == F32 and 0.0 <= u < 1.0 and float(u) == (w >> 8) / 2.0 ** 24
        for n in (1, 2, 5, 100, 301, 65536):
            assert 0 <= pc.below(w, n) < n
        assert F32(-0.12) <= pc.uniform(w, -0.12, 0.12) < F32(0.12)
        assert F32(1.0) <= pc.uniform(w, 1.0, 4.0) < F32(4.0)
        assert F32(0.5) <= pc.uniform(w, 0.5, 2.0) < F32(2.0)
    assert pc.unit(0xffffffff) == F32(1.0 - 2.0 ** -24)
    assert pc.below(0xffffffff, 5) == 4 and pc.below(0, 5) == 0 and pc.below(0x33333333, 5) == 0 and pc.below(0x33333334, 5) == 1
    assert not pc.boolean(0x80000000) and not pc.boolean(0x800000ff) and pc.boolean(0x80000100)      # u > 0.5, strictly


def test_branch_fractions():
    """Seven fair coins over sample ids 0..4095: each fraction within 0.5 +- 0.032 (four standard deviations at n = 4096);
    the min-overlap index takes all five values."""
    n = 4096
    counts, idx = np.zeros(7), np.zeros(5)
    for i in range(n):
        a, b = pc.words(pc.SEED, i, pc.SLOT_BOOLS_A), pc.words(pc.SEED, i, pc.SLOT_BOOLS_B)
        counts += [pc.boolean(w) for w in a + b[:3]]
        idx[pc.below(b[3], 5)] += 1
    frac = counts / n
    print("boolean fractions", frac, "overlap index counts", idx)
    assert (np.abs(frac - 0.5) <= 0.032).all(), frac
    assert (idx > n / 5 * 0.8).all(), idx


def _search_cases():
    H, W = 300, 300
    gt, gl = pc.ground_truth(48, 5, seed=21)
    out = [pc.plan(pc.SEED, i, H, W, gt[i], gl[i]) for i in range(48)]
    tb, tl = pc.tiny_ground_truth()
    out += [pc.plan(pc.SEED, i, H, W, tb[0], tl[0]) for i in range(24)]
    gt, gl = pc.ground_truth(24, 5, seed=22)
    out += [pc.plan(pc.SEED, (1 << 35) + i, 7, 5, gt[i], gl[i]) for i in range(24)]
    eb, el = pc.edge_ground_truth()
    out += [pc.plan(pc.SEED, i, 300, 300, eb[0], el[0]) for i in pc.LATE_IDS]
    return out


def test_sampler_invariants():
    """Every accepted window passes the package's own acceptance rule on the restatement's rectangles, holds 5 % .. 100 %
    of the canvas and keeps its aspect ratio within [0.5, 2] up to the rounding of its width to whole pixels."""
    import augmentation as aug
    accepted = fallback = 0
    for p in _search_cases():
        a = int(p["info"][0])
        if a < 0:
            assert p["geom"][9] == 0 and p["rects"] is None
            continue
        ch, cw = int(p["geom"][0]), int(p["geom"][1])
        y, x, h, w = [int(v) for v in p["geom"][4:8]]
        assert p["geom"][9] == 1 and 0 <= y and 0 <= x and y + h <= ch and x + w <= cw and h >= 1 and w >= 1
        if a == pc.ATTEMPTS:
            assert (y, x, h, w) == (0, 0, ch, cw)
            fallback += 1
            continue
        accepted += 1
        assert 0 <= a < pc.ATTEMPTS
        mo = pc.MIN_OVERLAPS[int(p["info"][1])]
        assert aug.window_satisfies((y, x, y + h, x + w), np.array(p["rects"], np.int64).reshape(-1, 4), mo)
        # the restatement's rectangles are the package's (float64 product there, fp32 here: equal or one pixel apart)
        assert np.abs(aug.pixel_rectangles(p["canvas_boxes"], ch, cw) - np.array(p["rects"]).reshape(-1, 4)).max() <= 1
        assert F32(0.05) * F32(ch * cw) <= h * w <= ch * cw
        # w = rint(h * aspect) with aspect in [0.5, 2): |w - h * aspect| <= 0.5
        assert 0.5 * h - 0.5 <= w <= 2.0 * h + 0.5
    assert accepted >= 20 and fallback >= 1, (accepted, fallback)


def test_required_sampler_outcomes_are_in_the_case_list():
    """What the GPU test relies on: the hard-coded ids give a late accepted attempt (>= 64, the lanes' second pass), the
    fallback (100), an image without a valid row (no patch) and both expand values."""
    H, W, boxes, labels, ids = pc.outcome_batch()
    ref = pc.plan_batch(pc.SEED, ids, H, W, boxes, labels)
    info = ref["info"]
    for k, (i, want) in enumerate(pc.LATE_IDS.items()):
        assert ids[k] == i and info[k, 0] == want, (i, info[k])
    assert ((info[:, 0] >= 64) & (info[:, 0] < 100)).sum() >= 3 and (info[:, 0] == 100).sum() >= 1 and (info[:, 0] == 64).any()
    none = len(pc.LATE_IDS)
    assert not (labels[none] > 0).any() and info[none, 0] == -1
    patched = info[:, 0] >= 0
    assert (info[patched, 2] == 1).any() and (info[patched, 2] == 0).any()


def test_box_arithmetic_matches_the_package():
    """The restatement's plan integers through the package's ``expand_boxes`` / ``renormalize`` / ``flip_boxes`` give the
    restatement's boxes bit for bit; rows that are not valid come through unchanged."""
    import augmentation as aug
    seen = set()
    for H, W, G, gseed in ((300, 300, 5, 31), (37, 53, 65, 32), (7, 5, 5, 33)):
        gt, gl = pc.ground_truth(24, G, seed=gseed)
        for i in range(24):
            p = pc.plan(pc.SEED, (1 << 33) + i, H, W, gt[i], gl[i])
            valid = gl[i] > 0
            g = gt[i][valid]
            ch, cw, pt, pl, y, x, h, w, flip, use_crop = [int(v) for v in p["geom"]]
            if use_crop:
                if p["info"][2]:
                    g = aug.expand_boxes(g, H, W, ch, cw, pt, pl)
                else:
                    assert (ch, cw, pt, pl) == (H, W, 0, 0)
                g = aug.renormalize(g, np.array([F32(y) / F32(ch), F32(x) / F32(cw), F32(y + h) / F32(ch), F32(x + w) / F32(cw)], F32))
            else:
                assert (ch, cw, pt, pl, y, x, h, w) == (H, W, 0, 0, 0, 0, H, W) and p["info"][0] == -1
            if flip:
                g = aug.flip_boxes(g)
            np.testing.assert_array_equal(p["boxes"][valid].view(np.uint32), np.asarray(g, F32).view(np.uint32))
            np.testing.assert_array_equal(p["boxes"][~valid].view(np.uint32), gt[i][~valid].view(np.uint32))
            seen.add((bool(use_crop), bool(p["info"][2]), bool(flip)))
    assert len(seen) >= 5, seen                     # patch with and without expand, with and without flip, no patch


def test_expand_geometry_matches_the_package():
    import augmentation as aug
    for i in range(64):
        e = pc.words(pc.SEED, i, pc.SLOT_EXPAND)
        for H, W in ((300, 300), (37, 53), (7, 5)):
            gt, gl = pc.ground_truth(1, 1, seed=i)
            p = pc.plan(pc.SEED, i, H, W, gt[0], gl[0])
            if p["info"][2]:
                want = aug.expand_geometry(H, W, pc.uniform(e[0], 1.0, 4.0), pc.unit(e[1]), pc.unit(e[2]))
                assert tuple(int(v) for v in p["geom"][:4]) == want
                assert H <= want[0] <= 4 * H and W <= want[1] <= 4 * W and 0 <= want[2] <= want[0] - H and 0 <= want[3] <= want[1] - W


def test_no_valid_row_and_label_free_validity():
    """No valid row: no patch, whatever the draw; without labels a row is valid iff its box is not all zero."""
    boxes = np.zeros((3, 4), F32)
    for i in range(16):
        p = pc.plan(pc.SEED, i, 300, 300, boxes, np.array([-1, 0, -1]))
        assert p["info"][0] == -1 and p["geom"][9] == 0 and not p["info"][2]
        np.testing.assert_array_equal(p["boxes"], boxes)
        q = pc.plan(pc.SEED, i, 300, 300, boxes, None)
        assert q["info"][0] == -1
    gt, gl = pc.ground_truth(1, 5, seed=3, n_valid=2)
    by_box = gt[0].copy()
    by_box[gl[0] <= 0] = 0
    for i in range(8):
        a, b = pc.plan(pc.SEED, i, 300, 300, by_box, np.where(gl[0] > 0, gl[0], -1)), pc.plan(pc.SEED, i, 300, 300, by_box, None)
        for n in pc.NAMES:
            np.testing.assert_array_equal(a[n], b[n])


def test_the_entry_point_and_the_python_surface_exist():
    import augmentation as aug
    import ssd_hip
    assert ssd_hip.lib().ssd_augment_plan is not None
    for name in ("plan_batch_device", "run_plan_device", "apply_batch_device", "device_draws"):
        assert callable(getattr(aug, name))
