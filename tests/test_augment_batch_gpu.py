"""The training input path as it runs on a batch: the four launches of ``augmentation.run_plans`` / ``run_plan_device``
(``ssd_image_mean``, ``ssd_augment_geometry``, ``ssd_image_mean`` with ``add``, ``ssd_augment_color``: csrc/ssd_data.hip)
driven through the C ABI on the cases of tests/augment_batch_cases.py, image by image against oracle/augment_oracle.py.
For B = 1 see test_augment.py; that the cases cannot pass by accident is test_augment_batch_cpu.py's business.

Means: float64 sums in another order than NumPy's, both rounded once to float32 -- within one float32 ulp of the reference
(they can differ only where the exact mean sits at a rounding boundary), and the same bits on every run.
Pixels: BIT-EQUAL to ``apply_plan`` given the device's own fill colour and pivot (teacher forcing): the same fp32 operations
in the same order, every one rounded on its own (-ffp-contract=off).  Boxes of the host path bit-equal too.
Then: ``run_plans``, ``run_plan_device`` and ``apply_batch_device`` give the bits of the test's own launches; an image's
pixels do not depend on its place in the batch; nothing is written outside the output; other output sizes.

Measured on the MI355X (ROCm 7, gfx950):
  means    927 compared (MIXED and STRIDE fills and pivots 198, the sweep 720, RESIZED's fills 9): none differs from the
           float64 reference, 0 ulp everywhere (a rounding boundary is a ~1e-8 event per mean; the bar stays one ulp).
  pixels   every word equal on the first run, 40 848 of MIXED and 12 750 000 of STRIDE, the geometry output on its own
           too; boxes equal; no guard word touched.  No kernel or wrapper bug was found.
  STRIDE   the launches with their copies (in the means test, which runs first) 0.40 s, the pixel test with the
           oracle's 17 images 0.60 s; the whole file 16 tests in under 5 s.
  Two deliberately wrong builds were run once against this file: ``fill[c]`` for ``fill[b * C + c]`` with a colour kernel
  that makes one trip only fails the MIXED, RESIZED and STRIDE pixel tests; ``add[0]`` for ``add[b]`` fails the means
  tests and the position test (the pixel tests are teacher-forced with the device's pivot and cannot see it)."""
import functools
import time

import numpy as np
import pytest

import augment_batch_cases as bc
import augment_plan_cases as pc
from oracle import augment_oracle as ao

pytestmark = pytest.mark.gpu
F32 = np.float32
PAYLOAD = 0x7FC5A5A5            # a quiet NaN no kernel produces (test_conv_geometry_gpu.py)
CASES = {"MIXED": bc.mixed, "STRIDE": bc.stride}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _guarded(shape):
    """A [B, ...] float32 tensor in the middle of a buffer one image longer on each side, every word the payload NaN."""
    import torch
    import ssd_hip as h
    n = int(np.prod(shape))
    per = n // int(shape[0])
    buf = torch.full((n + 2 * per,), PAYLOAD, dtype=torch.int32, device=h.device())
    return buf, buf[per:per + n].view(torch.float32).view(*shape)


def _stray(buf, shape):
    """Words outside the tensor of ``_guarded`` that no longer hold the payload."""
    n = int(np.prod(shape))
    per = n // int(shape[0])
    return int((buf[:per] != PAYLOAD).sum()) + int((buf[per + n:] != PAYLOAD).sum())


def _launches(images, geom, color, flags, add, out_size=None, colour=True):
    """The four launches the way ``run_plan_device`` makes them, every intermediate kept: the fill colours, the geometry
    output, the pivots, the final pixels (NumPy), and the guard words that changed after the geometry and after the
    colour kernel.  ``out_size``: another output size for the geometry kernel (then no colour pass)."""
    import torch
    import ssd_hip as h
    lib = h.lib()
    x = h.to_dev(images)
    B, H, W, C = (int(v) for v in x.shape)
    Ho, Wo = out_size if out_size is not None else (H, W)
    gd, cd = h.to_dev(geom, torch.int32), h.to_dev(color)
    fd, ad = h.to_dev(flags, torch.int32), h.to_dev(add)
    fill = torch.empty((B, C), dtype=torch.float32, device=x.device)
    pivot = torch.empty((B, C), dtype=torch.float32, device=x.device)
    buf, out = _guarded((B, Ho, Wo, C))
    h.check(lib.ssd_image_mean(h.ptr(x), B, H, W, C, None, h.ptr(fill), h.stream()), "ssd_image_mean")
    h.check(lib.ssd_augment_geometry(h.ptr(x), B, H, W, C, Ho, Wo, h.ptr(gd), h.ptr(fill), h.ptr(out), h.stream()), "ssd_augment_geometry")
    res = {"fill": fill.cpu().numpy(), "geo": out.cpu().numpy(), "stray_geometry": _stray(buf, out.shape)}
    if colour and out_size is None:
        h.check(lib.ssd_image_mean(h.ptr(out), B, H, W, C, h.ptr(ad), h.ptr(pivot), h.stream()), "ssd_image_mean")
        h.check(lib.ssd_augment_color(h.ptr(out), B, H, W, h.ptr(cd), h.ptr(fd), h.ptr(pivot), h.stream()), "ssd_augment_color")
        res.update(pivot=pivot.cpu().numpy(), out=out.cpu().numpy(), stray_colour=_stray(buf, out.shape))
    return res


@functools.lru_cache(maxsize=None)
def _run(name):
    case = CASES[name]()
    return _launches(case.images, *bc.arrays(case))


_GEOMETRY = {}


def _geometry_reference(name, fill):
    """The oracle's geometry output with the device's fill colours; computed once per case and fill."""
    key = (name, _bits(fill).tobytes())
    if key not in _GEOMETRY:
        _GEOMETRY[key] = bc.geometry_output(CASES[name](), fill)
    return _GEOMETRY[key]


def _assert_images_bit_equal(got, want, what):
    """Image by image, so that a failure names the images and the first word."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = [(b, int((_bits(got[b]) != _bits(want[b])).sum())) for b in range(len(got)) if (_bits(got[b]) != _bits(want[b])).any()]
    if bad:
        b = bad[0][0]
        i = np.argwhere(_bits(got[b]) != _bits(want[b]))[0]
        raise AssertionError("%s: images (index, words that differ) %r; image %d at %s: %r != %r" % (
            what, bad, b, i.tolist(), got[b][tuple(i)], want[b][tuple(i)]))


def _within_one_ulp(got, want, what):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    n = int((d > 0).sum())
    print("%s: %d of %d means differ from the float64 reference, by at most %.3g ulp" % (what, n, d.size, (d / ulp).max()))
    assert (d <= ulp).all(), "%s: %d means beyond one ulp, the worst by %.3g ulp" % (what, int((d > ulp).sum()), (d / ulp).max())


# ----------------------------------------------------------------------------------------------------------------- means
@pytest.mark.parametrize("name", list(CASES))
def test_batched_means_within_one_ulp(name):
    """Image b's fill colour and pivot (``add[b]`` = its brightness delta, 0 without brightness) at B > 1."""
    case = CASES[name]()
    r = _run(name)
    add = bc.arrays(case)[3]
    _within_one_ulp(r["fill"], bc.mean_reference(case.images), name + " fill")
    # an expanding image's pivot is the mean of pixels that hold the DEVICE's fill colour
    _within_one_ulp(r["pivot"], bc.mean_reference(_geometry_reference(name, r["fill"]), add), name + " pivot")
    # and against the device's own geometry output: the second launch reads what the first wrote, with its own add
    _within_one_ulp(r["pivot"], bc.mean_reference(r["geo"], add), name + " pivot of the device's geometry output")
    again = _launches(case.images, *bc.arrays(case))
    np.testing.assert_array_equal(_bits(again["fill"]), _bits(r["fill"]))
    np.testing.assert_array_equal(_bits(again["pivot"]), _bits(r["pivot"]))


@pytest.mark.parametrize("C", [1, 3, 4, 16])
def test_mean_sweep(C):
    """B = 3 at image sizes around the workgroup's 1024 threads, every channel count class; with and without ``add``."""
    import torch
    import ssd_hip as h
    B = 3
    rng = np.random.default_rng(400 + C)
    for H, W in ((1, 1), (7, 9), (31, 33), (32, 32), (25, 41)):
        x = rng.random((B, H, W, C), dtype=np.float32)
        add = np.array([-0.11, 0.0, 0.07], F32)
        xd, ad = h.to_dev(x), h.to_dev(add)
        for a, an in ((None, None), (ad, add)):
            outs = []
            for _ in range(2):
                buf, m = _guarded((B, C))
                h.check(h.lib().ssd_image_mean(h.ptr(xd), B, H, W, C, h.ptr(a), h.ptr(m), h.stream()), "ssd_image_mean")
                outs.append(m.cpu().numpy())
                assert _stray(buf, (B, C)) == 0
            np.testing.assert_array_equal(_bits(outs[0]), _bits(outs[1]))
            _within_one_ulp(outs[0], bc.mean_reference(x, an), "B 3, %d x %d x %d, add %s" % (H, W, C, an is not None))
            if H * W == 1:                                          # one value: nothing to round
                np.testing.assert_array_equal(_bits(outs[0]), _bits(bc.mean_reference(x, an)))


# ---------------------------------------------------------------------------------------------------------------- pixels
@pytest.mark.parametrize("name", list(CASES))
def test_every_image_bit_equal_to_the_oracle(name):
    """MIXED: every geometry kind beside every other, every colour flag value.  STRIDE: the grid-stride loops' second trip.
    No kernel or wrapper bug was found: every word was equal on the first run."""
    import augmentation as aug
    t0 = time.perf_counter()
    case = CASES[name]()
    H, W = case.images.shape[1:3]
    r = _run(name)
    t1 = time.perf_counter()
    _assert_images_bit_equal(r["geo"], _geometry_reference(name, r["fill"]), name + " geometry output")
    want, boxes = bc.reference(case, r["fill"], r["pivot"])
    _assert_images_bit_equal(r["out"], want, name + " pixels")
    got_boxes = np.stack([bc.host_boxes(aug, case.boxes[b], p, H, W) for b, p in enumerate(case.plans)])
    np.testing.assert_array_equal(_bits(got_boxes), _bits(boxes))
    o = r["out"]
    assert np.isfinite(o).all() and o.min() >= 0.0 and o.max() <= 1.0
    print("%s: %d pixel words equal; device %.2f s, oracle and comparison %.2f s" % (name, o.size, t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("name", list(CASES))
def test_nothing_written_outside_the_output(name):
    """The geometry output / the colour kernel's in-place tensor sit between two images' worth of payload NaNs."""
    r = _run(name)
    assert r["stray_geometry"] == 0 and r["stray_colour"] == 0, (r["stray_geometry"], r["stray_colour"])
    assert not (_bits(r["geo"]) == PAYLOAD).any() and not (_bits(r["out"]) == PAYLOAD).any()       # every word inside written


# --------------------------------------------------------------------------------------------------------- product paths
@pytest.mark.parametrize("name", list(CASES))
def test_run_plans_and_run_plan_device_give_the_same_bits(name):
    """``run_plans`` builds its own arrays (0 / 1 / 0 / 1 where the test's colour rows hold a draw the flags switch off,
    no fill launch without an expand, ``clone()`` without a crop or flip); ``run_plan_device`` reads uploaded ones."""
    import torch
    import augmentation as aug
    import ssd_hip as h
    case = CASES[name]()
    r = _run(name)
    _assert_images_bit_equal(aug.run_plans(case.images, case.plans).cpu().numpy(), r["out"], name + " run_plans")
    geom, color, flags, add = bc.arrays(case)
    plan = (h.to_dev(geom, torch.int32), h.to_dev(color), h.to_dev(flags, torch.int32), h.to_dev(add))
    _assert_images_bit_equal(aug.run_plan_device(case.images, plan).cpu().numpy(), r["out"], name + " run_plan_device")
    if name == "MIXED":             # subsets without an expand / without a crop or flip: run_plans' other branches
        for idx in ([0, 1, 2, 3, 4, 5, 6, 7, 14], [0, 1]):
            got = aug.run_plans(case.images[idx], [case.plans[b] for b in idx]).cpu().numpy()
            _assert_images_bit_equal(got, r["out"][idx], "run_plans on images %r" % (idx,))


def test_apply_batch_device_pixels_and_boxes_against_the_oracle():
    """The plan ``ssd_augment_plan`` draws, read back (``augment_plan_cases.host_plans``) and handed to ``apply_plan`` with
    the means of the test's own launches on that plan: the pixels and boxes ``apply_batch_device`` returns."""
    import augmentation as aug
    B, H, W = 3, 24, 40
    imgs = bc.images(B, H, W, seed=500)
    boxes, labels = pc.ground_truth(B, 5, seed=61)
    ids = np.arange((1 << 32) + 2, (1 << 32) + 5, dtype=np.int64)       # test_augment_plan_gpu.py: expand + crop, flip, copy, every colour op
    out, gb = aug.apply_batch_device(imgs, boxes, labels, ids, seed=pc.SEED)
    dev = aug.plan_batch_device(boxes, labels, ids, H, W, pc.SEED)
    arrays = {n: t.cpu().numpy() for n, t in zip(pc.NAMES, dev)}
    plans = pc.host_plans(arrays)
    assert any(p["expand"] for p in plans) and any(p["crop"] is None and not p["flip"] for p in plans)
    assert np.bitwise_or.reduce(arrays["flags"]) == 15
    r = _launches(imgs, arrays["geom"], arrays["color"], arrays["flags"], arrays["add"])
    assert r["stray_geometry"] == 0 and r["stray_colour"] == 0
    _assert_images_bit_equal(out.cpu().numpy(), r["out"], "apply_batch_device against the four launches")
    want_boxes = boxes.copy()
    for b, p in enumerate(plans):
        valid = labels[b] > 0
        px, g, _, _ = ao.apply_plan(imgs[b], boxes[b][valid], p, fill=r["fill"][b], pivot=r["pivot"][b])
        _assert_images_bit_equal(out[b:b + 1].cpu().numpy(), px[None], "apply_batch_device image %d" % b)
        want_boxes[b][valid] = g
    np.testing.assert_array_equal(_bits(gb.cpu().numpy()), _bits(want_boxes))


# -------------------------------------------------------------------------------------------------------------- position
def test_pixels_do_not_depend_on_the_place_in_the_batch():
    """Image b alone (B = 1), inside MIXED and inside a permutation of MIXED: the same bits, means included."""
    case = bc.mixed()
    r = _run("MIXED")
    geom, color, flags, add = bc.arrays(case)
    B = len(case.plans)
    for b in range(B):
        one = _launches(case.images[b:b + 1], geom[b:b + 1], color[b:b + 1], flags[b:b + 1], add[b:b + 1])
        for k in ("fill", "pivot", "geo", "out"):
            np.testing.assert_array_equal(_bits(one[k][0]), _bits(r[k][b]), err_msg="image %d alone, %s" % (b, k))
    perm = np.random.default_rng(7).permutation(B)
    assert (perm != np.arange(B)).sum() >= B - 2
    moved = _launches(case.images[perm], geom[perm], color[perm], flags[perm], add[perm])
    for k in ("fill", "pivot", "geo", "out"):
        np.testing.assert_array_equal(_bits(moved[k]), _bits(r[k][perm]), err_msg="permuted, %s" % k)


# --------------------------------------------------------------------------------------------------- another output size
@pytest.mark.parametrize("size", bc.RESIZED_SIZES)
def test_geometry_at_another_output_size(size):
    """``ssd_augment_geometry`` with out_h x out_w != H x W at B = 3 (use_crop = 1 on every image, the caller's contract):
    the oracle's canvas, its window through ``resize_bilinear`` to that size, the flip."""
    case = bc.resized()
    geom, color, flags, add = bc.arrays(case)
    assert (geom[:, 9] == 1).all()
    r = _launches(case.images, geom, color, flags, add, out_size=size)
    assert r["geo"].shape == (3,) + tuple(size) + (3,) and r["stray_geometry"] == 0
    _within_one_ulp(r["fill"], bc.mean_reference(case.images), "RESIZED fill")
    want = np.stack([bc.resized_reference(case, b, size[0], size[1], fill=r["fill"][b]) for b in range(3)])
    _assert_images_bit_equal(r["geo"], want, "RESIZED %d x %d" % size)
