"""CPU tests of the LANCZOS resize's host half: ``data_utils.lanczos_coefficients`` must be the tables of Pillow's 8-bit
resampler.  The tables drive a NumPy integer two-pass (tests/lanczos_cases.two_pass: horizontal, uint8 intermediate,
vertical, ``clamp((2^21 + sum px k) >> 22)``) whose bytes must EQUAL Pillow's -- the committed fixture
(tests/golden/lanczos.npz, written by Pillow) and, when PIL imports, Pillow run here.  No tolerance anywhere."""
import math

import numpy as np
import pytest

import lanczos_cases as lc
from utils import data_utils


def test_two_pass_on_the_coefficients_equals_the_pillow_fixture():
    cases, version = lc.load_fixture()
    assert version and len(cases) == len(lc.FIXTURE_SOURCES) * len(lc.FIXTURE_OUT)
    kinds = set()
    for (name, oh, ow), (src, want) in cases.items():
        h, w = src.shape[:2]
        assert want.shape == (oh, ow, 3) and want.dtype == np.uint8
        kinds.add((np.sign(oh - h), np.sign(ow - w)))
        got = lc.two_pass(src, oh, ow)
        assert np.array_equal(got, want), "%s %dx%d -> %dx%d: %d bytes differ from Pillow %s" % (
            name, h, w, oh, ow, int((got != want).sum()), version)
    # downscale, upscale, mixed, one axis equal, both equal are all in the fixture
    assert {(-1, -1), (1, 1), (-1, 1), (1, -1), (0, 0)} <= kinds and any(0 in k and k != (0, 0) for k in kinds)


@pytest.mark.parametrize("size", lc.CPU_LIVE_SIZES, ids=lambda s: "%dx%d" % s)
def test_two_pass_on_the_coefficients_equals_live_pillow(size):
    if not lc.pillow_available():
        pytest.skip("PIL does not import here: the fixture test pins the same bits")
    h, w = size
    for content in lc.CONTENTS:
        img = lc.image(h, w, content)
        got, want = lc.two_pass(img, 300, 300), lc.pillow(img, 300, 300)
        assert np.array_equal(got, want), "%dx%d %s: %d bytes differ" % (h, w, content, int((got != want).sum()))


@pytest.mark.parametrize("in_size,out_size,ksize", [(500, 300, 11), (300, 300, 7), (87, 300, 7)])
def test_bounds_and_ksize_match_the_closed_forms(in_size, out_size, ksize):
    bounds, k = data_utils.lanczos_coefficients(in_size, out_size)
    assert bounds.dtype == np.int32 and k.dtype == np.int32
    assert bounds.shape == (out_size, 2) and k.shape == (out_size, ksize)
    scale = in_size / out_size
    support = 3.0 * max(scale, 1.0)
    assert ksize == int(math.ceil(support)) * 2 + 1
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        assert (int(bounds[i, 0]), int(bounds[i, 1])) == (xmin, xmax)
        assert 1 <= xmax <= ksize and xmin + xmax <= in_size
        assert not k[i, xmax:].any()                                   # taps past xmax stay empty
        assert abs(int(k[i].sum()) - (1 << 22)) <= ksize               # normalised to 1.0 in 22-bit fixed point
    if in_size == out_size:                                            # the centre tap carries (almost) everything
        assert (k.max(1) >= (1 << 22) - 8).all()


def test_coefficients_are_cached_and_read_only():
    a = data_utils.lanczos_coefficients(123, 45)
    assert data_utils.lanczos_coefficients(123, 45) is a
    with pytest.raises(ValueError):
        a[1][0, 0] = 1
    with pytest.raises(ValueError):
        data_utils.lanczos_coefficients(0, 10)


def test_accumulator_stays_inside_int32():
    """``sum |k| * 255 + 2^21 < 2^31`` for the worst rows of strong down- and upscales (the kernels accumulate in int32)."""
    for in_size, out_size in [(16384, 300), (8000, 1), (5, 300), (1, 512), (3000, 512), (301, 300)]:
        _, k = data_utils.lanczos_coefficients(in_size, out_size)
        assert int(np.abs(k.astype(np.int64)).sum(1).max()) * 255 + (1 << 21) < 2 ** 31


def test_resize_lanczos_batch_rejects_wrong_dtype_and_rank_before_touching_the_device():
    for bad in (np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.uint8), np.zeros((1, 4, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            data_utils.resize_lanczos_batch([bad], 20, 20)
