"""Drawing on the device: ``ssd_image_minmax`` + ``ssd_draw_detections`` (utils/drawing_utils.py) against Pillow itself --
the committed fixture (tests/golden/drawing.npz, written by the reference's PIL call sequence), the NumPy painter the
CPU tests hold to that fixture, and Pillow run here on the full case list.  Byte equality everywhere, no tolerance.
``ssd_draw_bounding_boxes`` against its NumPy restatement; ``predictor.main(draw=True)`` against the host PIL pipeline."""
import importlib

import numpy as np
import pytest
import torch

import drawing_cases as dc
import ssd_hip
from utils import drawing_utils as du

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _draw(case, **kw):
    return _np(du.draw_bboxes_with_labels(case["img"], case["boxes"], case["labels"], case["probs"], dc.LABELS,
                                          colors=case["colors"], **kw))


def _diff(got, want):
    return int((got != want).any(-1).sum())


def test_equals_the_pillow_fixture():
    cases, version = dc.load_fixture()
    for name, (case, want) in cases.items():
        got = _draw(case)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), "%s: %d pixels differ from Pillow %s" % (name, _diff(got, want), version)


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c["name"])
def test_equals_the_painter_and_live_pillow(case):
    got = _draw(case)
    want = dc.restate(case, du.glyph_atlas())
    assert np.array_equal(got, want), "%s: %d pixels differ from the NumPy painter" % (case["name"], _diff(got, want))
    live = dc.pillow(case)
    assert np.array_equal(got, live), "%s: %d pixels differ from live Pillow" % (case["name"], _diff(got, live))


def test_min_max_of_every_case():
    lib = ssd_hip.lib()
    for case in dc.cases():
        x = ssd_hip.to_dev(case["img"][None])
        H, W = case["img"].shape[:2]
        mm = torch.empty((1, 2), dtype=torch.float32, device=x.device)
        ws = ssd_hip.workspace(lib.ssd_image_minmax_workspace_bytes(1))
        ssd_hip.check(lib.ssd_image_minmax(ssd_hip.ptr(x), 1, H, W, 3, ssd_hip.ptr(mm), ssd_hip.ptr(ws), ws.numel(),
                                           ssd_hip.stream()), "minmax")
        assert _np(mm).tolist() == [[float(case["img"].min()), float(case["img"].max())]], case["name"]


def test_ragged_batch_of_64_twice_with_identical_bytes():
    """64 images at 300 x 300 with 0..200 detections each, through the batched entry point (normalised boxes), twice."""
    imgs, boxes, labels, scores = dc.ragged_batch()
    cols = dc.colors(9)
    x = ssd_hip.to_dev(imgs)
    a = _np(du.draw_detections_batch(x, boxes, labels, scores, dc.LABELS, colors=cols))
    b = _np(du.draw_detections_batch(x, boxes, labels, scores, dc.LABELS, colors=cols))
    assert a.shape == (64, 300, 300, 3) and a.dtype == np.uint8
    assert np.array_equal(a, b)
    atlas = du.glyph_atlas()
    for i in range(64):
        case = dc.batch_case(imgs, boxes, labels, scores, i, cols)
        want = dc.pillow(case)
        assert np.array_equal(a[i], want), "image %d: %d pixels differ from live Pillow" % (i, _diff(a[i], want))
        if i < 8:
            assert np.array_equal(a[i], dc.restate(case, atlas)), "image %d differs from the NumPy painter" % i


def test_out_view_into_a_larger_tensor_leaves_the_neighbours_alone():
    cases, _ = dc.load_fixture()
    names = [n for n in dc.FIXTURE_NAMES if cases[n][0]["img"].shape == (32, 48, 3)]
    assert len(names) >= 3
    dev = ssd_hip.device()
    big = torch.full((len(names) + 3, 32, 48, 3), 77, dtype=torch.uint8, device=dev)
    for i, n in enumerate(names):
        case = cases[n][0]
        got = du.draw_bboxes_with_labels(case["img"], case["boxes"], case["labels"], case["probs"], dc.LABELS,
                                         colors=case["colors"], out=big[2 + i])
        assert got.data_ptr() == big[2 + i].data_ptr()
    host = _np(big)
    for i, n in enumerate(names):
        assert np.array_equal(host[2 + i], cases[n][1]), n
    assert (host[:2] == 77).all() and (host[2 + len(names):] == 77).all()
    with pytest.raises(ValueError):
        _draw(cases[names[0]][0], out=torch.empty((32, 49, 3), dtype=torch.uint8, device=dev))
    # the batched call into a slice of a larger batch
    imgs = np.stack([cases[n][0]["img"] for n in names])
    big2 = torch.full((len(names) + 2, 32, 48, 3), 9, dtype=torch.uint8, device=dev)
    nb = np.zeros((len(names), 2, 4), np.float32)
    nb[:, 0] = (0.125, 0.125, 0.75, 0.875)
    du.draw_detections_batch(imgs, nb, np.ones((len(names), 2)), np.full((len(names), 2), 0.5), dc.LABELS, colors=dc.colors(),
                             out=big2[1:1 + len(names)])
    host = _np(big2)
    assert (host[0] == 9).all() and (host[-1] == 9).all()
    for i, n in enumerate(names):
        case = dc.batch_case(imgs, nb, np.ones((len(names), 2), np.float32), np.full((len(names), 2), 0.5, np.float32), i, dc.colors())
        assert np.array_equal(host[1 + i], dc.pillow(case)), n


def test_empty_batch_and_no_boxes():
    out = du.draw_detections_batch(np.zeros((0, 20, 28, 3), np.float32), np.zeros((0, 5, 4)), np.zeros((0, 5)), np.zeros((0, 5)),
                                   dc.LABELS, colors=dc.colors())
    assert tuple(out.shape) == (0, 20, 28, 3) and out.dtype == torch.uint8
    assert ssd_hip.lib().ssd_draw_detections(None, None, 0, 20, 28, 3, None, None, None, None, 0, 0, None, 0, None, 3, 0, None,
                                             ssd_hip.stream()) == 0
    imgs = np.stack([dc.image(20, 28, "unit", 1), dc.image(20, 28, "wide", 2), dc.image(20, 28, "constant")])
    got = _np(du.draw_detections_batch(imgs, np.zeros((3, 0, 4)), np.zeros((3, 0)), np.zeros((3, 0)), dc.LABELS, colors=dc.colors()))
    for b in range(3):
        assert np.array_equal(got[b], dc.array_to_img(imgs[b])), b                   # T = 0: the plain converted image


def test_unsupported_shapes_return_their_status_before_any_launch():
    lib = ssd_hip.lib()
    dev = ssd_hip.device()
    s = ssd_hip.stream()
    sentinel = torch.full((1, 16, 16, 3), 5, dtype=torch.uint8, device=dev)
    fsentinel = torch.full((1, 16, 16, 3), 5.0, dtype=torch.float32, device=dev)
    img = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev)
    mm = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    ints = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    col = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = ssd_hip.ptr

    def draw(H=16, W=16, C=3, T=1, maxlen=8, width=3, image=img):
        return lib.ssd_draw_detections(p(image), p(mm), 1, H, W, C, p(ints), p(ints), p(col), p(ints), T, maxlen, p(col), 21,
                                       p(ints), width, 0, p(sentinel), s)

    for kw in (dict(C=4), dict(C=1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(T=du.MAX_BOXES + 1),
               dict(maxlen=du.MAX_TEXT + 1)):
        assert draw(**kw) == -3, (kw, lib.ssd_last_error())
    for kw in (dict(width=0), dict(width=65), dict(T=-1), dict(image=None)):
        assert draw(**kw) == -1, (kw, lib.ssd_last_error())
    ws = ssd_hip.workspace(lib.ssd_image_minmax_workspace_bytes(1))
    for C, H, W in ((4, 16, 16), (3, 0, 16), (3, 16, 16385)):
        assert lib.ssd_image_minmax(p(img), 1, H, W, C, p(mm), p(ws), ws.numel(), s) == -3
        assert lib.ssd_draw_bounding_boxes(p(img), 1, H, W, C, p(mm), 1, p(mm), 1, p(fsentinel), s) == -3
    assert lib.ssd_draw_bounding_boxes(p(img), 1, 16, 16, 3, p(mm), 1025, p(mm), 1, p(fsentinel), s) == -3
    assert lib.ssd_image_minmax(p(img), 1, 16, 16, 3, p(mm), p(ws), 8, s) == -1       # workspace too small
    torch.cuda.synchronize()
    assert (_np(sentinel) == 5).all() and (_np(fsentinel) == 5.0).all() and (_np(mm) == 0).all()
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        du.draw_detections_batch(np.zeros((1, 8, 8, 4), np.float32), np.zeros((1, 1, 4)), np.zeros((1, 1)), np.zeros((1, 1)),
                                 dc.LABELS, colors=dc.colors())
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        du.draw_bboxes(np.zeros((1, 8, 8, 1), np.float32), np.zeros((1, 1, 4)))


def test_draw_bounding_boxes_equals_its_restatement():
    rng = np.random.default_rng(4)
    for (B, H, W, T) in ((3, 37, 53, 9), (2, 64, 64, 1), (1, 20, 31, 0), (2, 300, 300, 40)):
        imgs = rng.random((B, H, W, 3)).astype(np.float32)
        boxes = rng.uniform(-0.3, 1.3, (B, T, 4)).astype(np.float32)
        if T:
            boxes[:, ::3, 2:] = boxes[:, ::3, :2] + rng.uniform(0, 0.6, (B, len(range(0, T, 3)), 2)).astype(np.float32)
        if T > 4:
            boxes[0, 1] = (0.0, 0.0, 1.0, 1.0)
            boxes[0, 2] = (0.5, 0.5, 0.5, 0.5)
            boxes[0, 4] = (0.6, 0.1, 0.2, 0.9)                                        # inverted
        cols = np.asarray([[1, 0, 0, 1], [0.25, 0.5, 0.75, 1], [0, 0, 1, 1]], np.float32)
        got = _np(du.draw_bboxes(imgs, boxes, colors=cols))
        want = dc.draw_bounding_boxes(imgs, boxes, cols)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, H, W, T)
    red = _np(du.draw_bboxes(imgs, boxes))                                            # the reference's default colour
    assert np.array_equal(red, dc.draw_bounding_boxes(imgs, boxes, np.asarray([[1, 0, 0, 1]], np.float32)))


def test_grid_map_squares():
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (75, 100, 3), dtype=np.uint8)
    stride = 8
    ys, xs = np.meshgrid(np.arange(-8, 80, stride), np.arange(-8, 104, stride), indexing="ij")
    grid = np.stack([xs.ravel(), ys.ravel(), xs.ravel(), ys.ravel()], -1)
    want = Image.fromarray(img)
    d = ImageDraw.Draw(want)
    for g in grid:
        d.rectangle((g[0] + stride // 2 - 2, g[1] + stride // 2 - 2, g[2] + stride // 2 + 2, g[3] + stride // 2 + 2),
                    fill=(255, 255, 255, 0))
    got = _np(du.draw_grid_map(img, grid, stride))
    assert np.array_equal(got, np.asarray(want))
    assert np.array_equal(_np(du.draw_grid_map(img, np.zeros((0, 4)), stride)), img)


def _predictor_args(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "6")
    return importlib.import_module("predictor")


def test_predictor_draw_writes_one_png_per_image_equal_to_the_host_pipeline(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from utils import data_utils
    predictor = _predictor_args(tmp_path, monkeypatch)
    du.seed(17)
    cols = du.random_colors(21)
    du.seed(17)
    out_dir = tmp_path / "drawn"
    b, l, s = predictor.main(["--backbone", "mobilenet_v2"], batch_size=4, draw=True, draw_dir=str(out_dir))
    assert b.shape == (6, 200, 4) and "predicted 6 images" in capsys.readouterr().out
    files = sorted(f.name for f in out_dir.iterdir())
    assert files == ["img_%05d.png" % i for i in range(6)]
    assert ((l > 0).sum(-1) > 0).all()                                               # something was drawn on every image
    # the same images, as predictor.main prepares them
    raw = data_utils.synthetic_voc_items(6, 21)
    items = (data_utils.preprocessing(x, 300, 300) for x in raw)
    imgs = np.concatenate([_np(batch[0]) for batch in data_utils.padded_batch(items, 4, data_utils.get_padding_values())])
    for i in range(6):
        case = dc.batch_case(imgs, b, l, s, i, cols)
        got = np.asarray(Image.open(str(out_dir / ("img_%05d.png" % i))))
        want = dc.pillow(case)
        assert np.array_equal(got, want), "image %d: %d pixels differ from the host PIL pipeline" % (i, _diff(got, want))


def test_predictor_without_the_knobs_is_unchanged(tmp_path, monkeypatch, capsys):
    predictor = _predictor_args(tmp_path, monkeypatch)
    r0 = predictor.main(["--backbone", "mobilenet_v2"], batch_size=4)
    out0 = capsys.readouterr().out
    assert not list(tmp_path.rglob("*.png"))                                         # nothing is drawn without the knob
    r1 = predictor.main(["--backbone", "mobilenet_v2"], batch_size=4, draw=True, draw_dir=str(tmp_path / "d"))
    assert len(r0) == 3 and len(r1) == 3
    for a, c in zip(r0, r1):
        np.testing.assert_array_equal(a, c)
    assert sorted(str(f.relative_to(tmp_path)) for f in tmp_path.rglob("*.png")) == ["d/img_%05d.png" % i for i in range(6)]
    lines = [ln for ln in out0.splitlines() if ln.strip()]
    assert any(ln.startswith("predicted 6 images") for ln in lines) and not any("draw" in ln or "wrote" in ln for ln in lines)
