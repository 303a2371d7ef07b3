"""The device half of the JPEG encoder (``ssd_jpeg_forward``) against the NumPy restatement of tests/jpeg_encode_cases.py,
and the whole road -- ``data_utils.encode_jpeg_batch``, ``drawing_utils`` with ``out_format="jpeg"`` -- against the
Pillow-written fixture and live Pillow.  Byte equality is the bar: no tolerance anywhere.  (The quantiser divides with
a true integer division, so there is no reciprocal to test exhaustively.)"""
import io

import numpy as np
import pytest
import torch

import drawing_cases as dc
import jpeg_encode_cases as jc
import ssd_hip
from utils import data_utils
from utils import drawing_utils as du

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")

NAMES = [c[0] for c in jc.cases()]


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


def _pack(arrays):
    return torch.as_tensor(np.concatenate([a.reshape(-1) for a in arrays])).to(ssd_hip.device())


def _forward(arrays, subs, qualities):
    """One ``ssd_jpeg_forward`` call -> per image (Geometry, int16 coefficient storage) on the host."""
    tables = np.stack([jc.quality_tables(q) for q in qualities])
    coef, desc = data_utils.jpeg_forward_batch(_pack(arrays), [a.shape[:2] for a in arrays], [jc.SAMPLING[s] for s in subs], tables)
    host = coef.cpu().numpy()
    out = []
    for a, s, d in zip(arrays, subs, desc):
        g = jc.Geometry(a.shape[0], a.shape[1], *jc.SAMPLING[s])
        at = int(d["coef_offset"])
        out.append((g, host[at:at + g.n * 2].view(np.int16)))
    return out


def test_forward_equals_the_restatement_for_every_fixture_case(fixture):
    arrays = [fixture[n][0] for n in NAMES]
    qualities = [fixture[n][1] for n in NAMES]
    subs = [fixture[n][2] for n in NAMES]
    runs = [_forward(arrays, subs, qualities) for _ in range(2)]
    for n, a, q, s, (g, got), (_, again) in zip(NAMES, arrays, qualities, subs, runs[0], runs[1]):
        _, want = jc.forward(a, s, jc.quality_tables(q))
        assert got.dtype == np.int16 and got.size == want.size, n
        assert np.array_equal(g.real(got), g.real(want)), (n, np.flatnonzero(g.real(got) != g.real(want))[:8])
        assert np.array_equal(got, again), n


def test_one_ragged_call_reproduces_the_fixture_bytes(fixture):
    """All three subsamplings, two qualities, 1x1 through 37x53 in one call; the host half turns each image's
    coefficients into the bytes Pillow wrote."""
    picked = [n for n in NAMES if fixture[n][1] in (30, 95) and fixture[n][0].shape[0] <= 37]
    assert set(fixture[n][2] for n in picked) == set(jc.SUBSAMPLINGS) and set(fixture[n][1] for n in picked) == {30, 95}
    assert {(1, 1), (37, 53)} <= set(fixture[n][0].shape[:2] for n in picked)
    arrays = [fixture[n][0] for n in picked]
    got = _forward(arrays, [fixture[n][2] for n in picked], [fixture[n][1] for n in picked])
    for n, (g, coef) in zip(picked, got):
        rgb, q, s, blob = fixture[n]
        rc, info = jc.lib_info(rgb.shape[0], rgb.shape[1], s, jc.quality_tables(q))
        rc2, out, intact = jc.lib_entropy_encode(coef, info)
        assert rc == 0 and rc2 == 0 and intact and out == blob, n


@pytest.mark.parametrize("setting", [None, "1", "0"])
def test_encode_jpeg_batch_equals_the_fixture(fixture, monkeypatch, setting):
    if setting == "0" and not jc.pillow_is_turbo():
        pytest.skip("the Pillow leg reproduces the fixture only on libjpeg-turbo")
    if setting is None:
        monkeypatch.delenv("SSD_JPEG_ENCODE_GPU", raising=False)
    else:
        monkeypatch.setenv("SSD_JPEG_ENCODE_GPU", setting)
    dev = ssd_hip.device()
    images = [torch.as_tensor(fixture[n][0]).to(dev) for n in NAMES]
    blobs = data_utils.encode_jpeg_batch(images, quality=[fixture[n][1] for n in NAMES], subsampling=[fixture[n][2] for n in NAMES],
                                         workers=4)
    assert len(blobs) == len(NAMES)
    for n, b in zip(NAMES, blobs):
        assert isinstance(b, bytes) and b == fixture[n][3], n
    # the uniform [B,H,W,3] tensor the drawing kernels write
    same = [n for n in NAMES if n.startswith("37x53_")]
    assert len(same) == 9
    x = torch.stack([torch.as_tensor(fixture[n][0]).to(dev) for n in same])
    got = data_utils.encode_jpeg_batch(x, quality=[fixture[n][1] for n in same], subsampling=[fixture[n][2] for n in same])
    assert got == [fixture[n][3] for n in same]


def _drawn_batch():
    rng = np.random.default_rng(3)
    B, H, W, T = 3, 40, 56, 4
    imgs = np.stack([dc.image(H, W, seed=i) for i in range(B)])
    y1, x1 = rng.uniform(0, 0.6, (B, T)), rng.uniform(0, 0.6, (B, T))
    boxes = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.4, (B, T)), x1 + rng.uniform(0.1, 0.4, (B, T))], -1).astype(np.float32)
    labels = rng.integers(1, len(dc.LABELS), (B, T))
    probs = rng.uniform(0.3, 1.0, (B, T)).astype(np.float32)
    return imgs, boxes, labels, probs


def test_drawn_detections_are_written_as_pillow_would_write_them(tmp_path, monkeypatch):
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("live comparison needs a Pillow built on libjpeg-turbo")
    monkeypatch.setenv("SSD_JPEG_ENCODE_GPU", "1")                                   # the GPU road, whatever the default
    imgs, boxes, labels, probs = _drawn_batch()
    drawn = du.draw_detections_batch(ssd_hip.to_dev(imgs), boxes, labels, probs, dc.LABELS, colors=dc.colors())
    host = drawn.cpu().numpy()
    du._present(drawn, str(tmp_path / "j"), 5, False, out_format="jpeg", out_quality=90)
    du._present(drawn, str(tmp_path / "d"), 5, False, out_format="jpeg")
    assert sorted(f.name for f in (tmp_path / "j").iterdir()) == ["img_%05d.jpg" % (5 + i) for i in range(3)]
    for i in range(3):
        for d, opts in (("j", {"quality": 90}), ("d", {"quality": 75})):
            buf = io.BytesIO()
            Image.fromarray(host[i]).save(buf, "JPEG", **opts)                     # Pillow's own default subsampling
            with open(str(tmp_path / d / ("img_%05d.jpg" % (5 + i))), "rb") as f:
                assert f.read() == buf.getvalue(), (d, i)
    # the public functions pass the knobs through
    case = dc.cases()[0]
    out = du.draw_bboxes_with_labels(case["img"], case["boxes"], case["labels"], case["probs"], dc.LABELS, colors=case["colors"],
                                     out_dir=str(tmp_path / "one"), out_format="jpeg", out_quality=30)
    buf = io.BytesIO()
    Image.fromarray(out.cpu().numpy()).save(buf, "JPEG", quality=30)
    with open(str(tmp_path / "one" / "img_00000.jpg"), "rb") as f:
        assert f.read() == buf.getvalue()
    with pytest.raises(ValueError):
        du._present(drawn, str(tmp_path / "x"), 0, False, out_format="gif")


def test_png_output_is_byte_identical_to_before(tmp_path):
    from PIL import Image
    imgs, boxes, labels, probs = _drawn_batch()
    drawn = du.draw_detections_batch(ssd_hip.to_dev(imgs), boxes, labels, probs, dc.LABELS, colors=dc.colors())
    du._present(drawn, str(tmp_path / "a"), 0, False)
    du._present(drawn, str(tmp_path / "b"), 0, False, out_format="png", out_quality=10)
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["img_%05d.png" % i for i in range(3)]
    for i, a in enumerate(drawn.cpu().numpy()):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "PNG")                                        # what _present always did
        for d in ("a", "b"):
            with open(str(tmp_path / d / ("img_%05d.png" % i)), "rb") as f:
                assert f.read() == buf.getvalue(), (d, i)


def test_predictor_draw_format_jpeg_writes_files_pillow_opens(tmp_path, monkeypatch):
    import importlib
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "2")
    monkeypatch.setenv("SSD_JPEG_ENCODE_GPU", "1")                                   # the GPU road, whatever the default
    predictor = importlib.import_module("predictor")
    out_dir = tmp_path / "drawn"
    predictor.main(["--backbone", "mobilenet_v2"], batch_size=2, draw=True, draw_dir=str(out_dir), draw_format="jpeg")
    assert sorted(f.name for f in out_dir.iterdir()) == ["img_00000.jpg", "img_00001.jpg"]
    for f in out_dir.iterdir():
        im = Image.open(str(f))
        assert im.format == "JPEG" and im.size == (300, 300) and np.asarray(im.convert("RGB")).shape == (300, 300, 3)
    with pytest.raises(ValueError):
        predictor.main(["--backbone", "mobilenet_v2"], batch_size=2, draw=True, draw_dir=str(out_dir), draw_format="gif")


def _call(desc, B, rgb, tables, coef, ws, coef_bytes=None, ws_bytes=None):
    return ssd_hip.lib().ssd_jpeg_forward(ssd_hip.ptr(rgb), rgb.numel(), ssd_hip.ptr(tables), tables.numel(), desc.ctypes.data,
                                          ssd_hip.ptr(tables), B, ssd_hip.ptr(coef), coef.numel() if coef_bytes is None else coef_bytes,
                                          ssd_hip.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, ssd_hip.stream())


def test_argument_validation_launches_nothing_and_an_empty_batch_is_a_no_op():
    dev = ssd_hip.device()
    lib = ssd_hip.lib()
    assert lib.ssd_jpeg_forward(None, 0, None, 0, None, None, 0, None, 0, None, 0, ssd_hip.stream()) == 0
    assert data_utils.encode_jpeg_batch([]) == []
    assert lib.ssd_jpeg_forward_workspace_bytes(None, 0) == 0
    shapes, samplings = [(17, 15), (8, 8)], [(2, 2), (1, 1)]
    layout = data_utils._jpeg_encode_layout(shapes, samplings)
    good = layout["desc"]
    assert lib.ssd_jpeg_forward_workspace_bytes(good.ctypes.data, 2) == layout["plane_bytes"] == (12 + 3) * 64
    host = np.zeros(layout["total"], np.uint8)
    host[:good.nbytes] = good.view(np.uint8)
    host[layout["tables_at"]:] = np.tile(jc.quality_tables(75).reshape(-1), 2).view(np.uint8)
    tables = torch.as_tensor(host).to(dev)
    rgb = torch.zeros(17 * 15 * 3 + 8 * 8 * 3, dtype=torch.uint8, device=dev)
    coef = torch.full((layout["coef_bytes"],), 0x5A, dtype=torch.uint8, device=dev)
    ws = torch.full((layout["plane_bytes"],), 0x5A, dtype=torch.uint8, device=dev)

    def edited(**fields):
        d = good.copy()
        for k, (b, v) in fields.items():
            d[b][k] = v
        return d

    invalid = [edited(src_offset=(1, 17 * 15 * 3 + 1)), edited(src_offset=(0, -1)), edited(coef_offset=(1, 8)),
               edited(coef_offset=(1, 0)), edited(quant_offset=(0, layout["total"] - 128)), edited(quant_offset=(1, 4)),
               edited(plane_offset=(1, 0)), edited(plane_offset=(1, 12 * 64 - 16)), edited(block_start=(1, 5)),
               edited(item_start=(1, 15))]
    unsupported = [edited(H=(0, 0)), edited(W=(1, 16385)), edited(h_samp=(0, 1), v_samp=(0, 2)), edited(h_samp=(1, 4))]
    for d in invalid:
        assert _call(d, 2, rgb, tables, coef, ws) == -1, d
        assert lib.ssd_last_error().decode().startswith("ssd_jpeg_forward")
    for d in unsupported:
        assert _call(d, 2, rgb, tables, coef, ws) == -3, d
    assert _call(good, 2, rgb, tables, coef, ws, coef_bytes=layout["coef_bytes"] - 16) == -1
    assert _call(good, 2, rgb, tables, coef, ws, ws_bytes=layout["plane_bytes"] - 16) == -1
    assert _call(good, 70000, rgb, tables, coef, ws) == -3
    assert _call(good, -1, rgb, tables, coef, ws) == -1
    assert lib.ssd_jpeg_forward(ssd_hip.ptr(rgb), rgb.numel(), ssd_hip.ptr(tables), tables.numel(), good.ctypes.data, None, 2,
                                ssd_hip.ptr(coef), coef.numel(), ssd_hip.ptr(ws), ws.numel(), ssd_hip.stream()) == -1
    torch.cuda.synchronize()
    assert bool((coef == 0x5A).all()) and bool((ws == 0x5A).all())                  # nothing was launched
    assert _call(good, 2, rgb, tables, coef, ws) == 0
    torch.cuda.synchronize()
    g = jc.Geometry(17, 15, 2, 2)
    black = jc.forward(np.zeros((17, 15, 3), np.uint8), "4:2:0", jc.quality_tables(75))[1]
    assert np.array_equal(g.real(coef.cpu().numpy()[:g.n * 2].view(np.int16)), g.real(black))
    with pytest.raises(ValueError):
        data_utils.encode_jpeg_batch([torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev)], subsampling="4:1:1")
    with pytest.raises(ValueError):
        data_utils.encode_jpeg_batch([torch.zeros((4, 4, 3), dtype=torch.float32, device=dev)])
