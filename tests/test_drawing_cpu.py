"""CPU tests of the drawing feature's host half (utils/drawing_utils.py) and of its oracles (tests/drawing_cases.py): the
glyph atlas read out of Pillow must reproduce ``font.getmask``; the NumPy painter that replays Pillow's primitives on
that atlas must EQUAL Pillow's bytes -- the committed fixture (tests/golden/drawing.npz, written by Pillow) and Pillow
run here on the full case list; the text encoding validates before anything reaches the device.  No tolerance anywhere."""
import numpy as np
import pytest

import drawing_cases as dc
from utils import drawing_utils as du


def test_painter_on_the_atlas_equals_the_pillow_fixture():
    cases, version = dc.load_fixture()
    assert version and set(cases) == set(dc.FIXTURE_NAMES)
    atlas = du.glyph_atlas()
    for name, (case, want) in cases.items():
        assert want.dtype == np.uint8 and want.shape == case["img"].shape
        got = dc.restate(case, atlas)
        assert np.array_equal(got, want), "%s: %d pixels differ from Pillow %s" % (name, int((got != want).any(-1).sum()), version)


def test_fixture_inputs_are_the_listed_cases():
    cases, _ = dc.load_fixture()
    by_name = {c["name"]: c for c in dc.cases()}
    for name, (case, _) in cases.items():
        for key in ("img", "boxes", "labels", "probs", "colors"):
            assert np.array_equal(case[key], by_name[name][key]), (name, key)


def test_case_list_covers_what_it_must():
    cases = dc.cases()
    sides, labels, probs = set(), set(), set()
    for c in cases:
        H, W = c["img"].shape[:2]
        for i, (y1, x1, y2, x2) in enumerate(c["boxes"].tolist()):
            if dc.drawn(c, i):
                sides.add(min(x2 - x1, y2 - y1))
                labels.add(int(c["labels"][i]))
                probs.add(float(c["probs"][i]))
    assert {1, 2, 3, 4, 5, 6} <= sides and labels >= set(range(21))
    assert {float(np.float32(p)) for p in dc.PROBS} <= probs
    assert any(len(c["boxes"]) == 0 for c in cases) and any(len(c["boxes"]) == 200 for c in cases)
    assert any(c["img"].min() == c["img"].max() for c in cases)                        # max after the subtraction is 0
    assert any(c["img"].min() < 0 and c["img"].max() > 1 for c in cases)
    assert any(c["img"].shape[0] != c["img"].shape[1] and c["img"].shape[1] % 4 for c in cases)
    assert any(not dc.drawn(c, i) for c in cases for i in range(len(c["boxes"])))


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c["name"])
def test_painter_on_the_atlas_equals_live_pillow(case):
    got, want = dc.restate(case, du.glyph_atlas()), dc.pillow(case)
    assert np.array_equal(got, want), "%s: %d pixels differ" % (case["name"], int((got != want).any(-1).sum()))


def test_rectangle_strokes_equal_pillow_for_every_small_box():
    """Boxes thinner than twice the width paint outside themselves; every (width, w, h) up to 14, inside and across the
    border."""
    from PIL import Image, ImageDraw
    for width in (1, 2, 3, 4, 5):
        for w in range(1, 15):
            for h in range(1, 15):
                for ox, oy in ((6, 6), (-2, -3), (17, 16)):
                    im = Image.new("L", (24, 24), 0)
                    ImageDraw.Draw(im).rectangle((ox, oy, ox + w, oy + h), outline=255, width=width)
                    mine = np.zeros((24, 24), np.uint8)
                    dc.rectangle(mine, ox, oy, ox + w, oy + h, 255, width)
                    assert np.array_equal(np.asarray(im), mine), (width, w, h, ox, oy)


def test_atlas_reproduces_getmask_for_label_strings_and_random_strings():
    atlas = du.glyph_atlas()
    assert atlas.dtype == np.uint32 and atlas.shape == (96, 4) and not atlas.flags.writeable
    assert du.glyph_atlas() is atlas
    assert not atlas[0].any() and not atlas[95].any()                                  # the space and the blank glyph
    rng = np.random.default_rng(0)
    strings = [du.format_label(name, np.float32(p)) for name in dc.LABELS for p in dc.PROBS + (0.0, 0.0415)]
    strings += ["".join(chr(c) for c in rng.integers(32, 127, rng.integers(1, 40))) for _ in range(1500)]
    strings += [chr(a) + chr(b) for a in range(32, 127) for b in range(32, 127)]       # every ordered pair
    for s in strings:
        assert np.array_equal(dc.text_mask(atlas, s), dc.pillow_mask(s)), repr(s)
    # the overhang the issue names: these glyphs reach one column left of their origin
    left = {chr(32 + g) for g in range(95) if (atlas[g, 3] >> 16) & 1}
    assert set("bhkmnpuvwy") <= left and len(left) == 29


def test_text_encoding_and_validation():
    tb, tl = du.encode_texts(["cat 0.500", "", "diningtable 1.000"])
    assert tb.dtype == np.uint8 and tb.shape == (3, 17) and tl.tolist() == [9, 0, 17]
    assert bytes(tb[0, :9]) == b"cat 0.500" and not tb[0, 9:].any() and not tb[1].any()
    assert du.encode_texts([], maxlen=None)[0].shape == (0, 0)
    assert du.encode_texts(["ab"], maxlen=8)[0].shape == (1, 8)
    assert du.format_label("dog", np.float32(0.987)) == "dog 0.987" and du.format_label("bg", np.float32(1.0)) == "bg 1.000"
    for bad in ("café 0.5", "a\nb", "tab\t", "\x7f", "Ā"):
        with pytest.raises(ValueError):
            du.encode_texts([bad])
    with pytest.raises(ValueError):
        du.encode_texts(["x" * (du.MAX_TEXT + 1)])
    with pytest.raises(ValueError):
        du.encode_texts(["abc"], maxlen=2)


def test_label_texts_follow_the_reference_loop():
    boxes = np.asarray([[[0, 0, 10, 10], [5, 5, 5, 9], [3, 9, 8, 2], [1, 1, 2, 2]]], np.int32)
    li = np.asarray([[1, 99, -4, 20]])
    pr = np.asarray([[0.5, 0.1, 0.2, 1.0]], np.float32)
    assert du.label_texts(boxes, li, pr, dc.LABELS) == [["aeroplane 0.500", "", "", "tvmonitor 1.000"]]
    with pytest.raises(IndexError):
        du.label_texts(boxes, np.asarray([[21, 0, 0, 0]]), pr, dc.LABELS)


def test_colors_come_from_the_seeded_generator_or_the_argument():
    du.seed(3)
    a = du.random_colors(21)
    du.seed(3)
    assert np.array_equal(du.random_colors(21), a) and a.shape == (21, 4) and a.min() >= 0 and a.max() <= 255
    c = du._colors_u8(dc.colors(), 21)
    assert c.dtype == np.uint8 and c.shape == (21, 3) and np.array_equal(c, dc.colors()[:, :3])
    for bad in (np.zeros((20, 3)), np.full((21, 3), 256), np.zeros((21, 2))):
        with pytest.raises(ValueError):
            du._colors_u8(bad, 21)


def test_bad_arguments_are_rejected_before_touching_the_device():
    with pytest.raises(ValueError):
        du.draw_detections_batch(np.zeros((4, 5, 3), np.float32), np.zeros((1, 1, 4)), np.zeros((1, 1)), np.zeros((1, 1)), dc.LABELS)
    with pytest.raises(ValueError):
        du.draw_grid_map(np.zeros((8, 8, 3), np.float32), np.zeros((1, 4)), 8)
    with pytest.raises(ValueError):
        du.draw_grid_map(np.zeros((8, 8, 3), np.uint8), np.asarray([[5, 5, -9, 5]]), 8)
