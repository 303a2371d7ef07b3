"""The device PNG encoder (``ssd_png_encode`` through ``data_utils.png_pack_batch`` / ``encode_png_batch``) against its
host model, bit for bit, and -- independently, so that a mistake both share cannot pass on equality alone -- against
Pillow's decode of the device's own bytes.  Then the roads around it: guard regions, repeatability, the Pillow fallback
outside the kernel's limits, and ``drawing_utils`` with and without ``SSD_PNG_GPU=1``."""
import io

import numpy as np
import pytest
import torch

import drawing_cases as dc
import png_cases as pc
import ssd_hip
from utils import data_utils
from utils import drawing_utils as du

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")

CASES = pc.cases()


@pytest.fixture(scope="module")
def host_files():
    """name -> the host model's file, encoded once for all tests."""
    out = {}
    for name, rgb, mode in CASES:
        rc, blob, _, intact, _ = pc.host_encode(rgb, mode)
        assert rc == 0 and intact, name
        out[name] = blob
    return out


def _pack(arrays):
    return torch.as_tensor(np.concatenate([a.reshape(-1) for a in arrays])).to(ssd_hip.device())


def _decode(blob):
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "RGB"
    return np.asarray(im)


def _files(out, offsets):
    host, off = out.cpu().numpy(), offsets.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) > 0).all()
    return [host[off[b]:off[b + 1]].tobytes() for b in range(len(off) - 1)]


@pytest.fixture(scope="module")
def ragged(host_files):
    """The ragged batch that holds every case at once, through ONE call: (the device's files, out, offsets)."""
    out, offsets = data_utils.png_pack_batch(_pack([c[1] for c in CASES]), [c[1].shape[:2] for c in CASES], [c[2] for c in CASES])
    return _files(out, offsets), out, offsets


def test_ragged_batch_equals_the_host_model_bit_for_bit(ragged, host_files):
    got = ragged[0]
    assert len(got) == len(CASES)
    for (name, rgb, mode), blob in zip(CASES, got):
        assert blob == host_files[name], name


def test_pillow_decodes_the_devices_bytes_to_the_input_pixels(ragged):
    for (name, rgb, mode), blob in zip(CASES, ragged[0]):
        assert np.array_equal(_decode(blob), rgb), name
    small = {c[0] for c in pc.small_cases()}
    for (name, rgb, mode), blob in zip(CASES, ragged[0]):
        if name in small:
            pc.check_file(blob, rgb, mode)                                          # chunk walk, strict zlib, the restated F


def test_every_case_alone_and_the_reversed_batch_give_the_same_files(ragged, host_files):
    rev = CASES[::-1]
    out, offsets = data_utils.png_pack_batch(_pack([c[1] for c in rev]), [c[1].shape[:2] for c in rev], [c[2] for c in rev])
    for (name, _, _), blob in zip(rev, _files(out, offsets)):
        assert blob == host_files[name], name
    for name, rgb, mode in pc.small_cases():
        got = data_utils.encode_png_batch([torch.as_tensor(rgb).to(ssd_hip.device())], filter=pc.FILTERS[mode])
        assert got == [host_files[name]], name


def test_two_calls_give_equal_bytes_and_the_4d_tensor_road(host_files):
    smooth = next(c for c in CASES if c[0] == "smooth_300_adaptive")[1]
    flat = next(c for c in CASES if c[0] == "flat_300")[1]
    batch = torch.as_tensor(np.stack([smooth, flat, smooth])).to(ssd_hip.device())
    first = data_utils.encode_png_batch(batch)
    assert first == data_utils.encode_png_batch(batch)
    assert first == [host_files["smooth_300_adaptive"], host_files["flat_300"], host_files["smooth_300_adaptive"]]
    per_image = data_utils.encode_png_batch(batch, filter=["sub", "adaptive", "paeth"])
    assert per_image == [host_files["smooth_300_sub"], host_files["flat_300"], host_files["smooth_300_paeth"]]
    assert data_utils.encode_png_batch([]) == []
    out, offsets = data_utils.png_pack_batch(None, [])
    assert out.numel() == 0 and offsets.cpu().tolist() == [0]


def test_nothing_is_written_past_the_files_or_outside_the_buffer(host_files):
    lib = ssd_hip.lib()
    dev = ssd_hip.device()
    picked = [c for c in CASES if c[0] in ("shape_2x3", "cut_w5462_smooth", "run_1_2_50_n173", "stored_noise_64", "flat_300")]
    shapes, filters = [c[1].shape[:2] for c in picked], [c[2] for c in picked]
    layout = data_utils._png_layout(shapes, filters)
    desc, B, guard = layout["desc"], len(picked), 4096
    rgb = _pack([c[1] for c in picked])
    store = torch.full((guard + layout["out_bytes"] + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = store[guard:guard + layout["out_bytes"]]
    assert out.data_ptr() % 16 == 0
    offsets = torch.full((B + 1 + 2,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.ssd_png_encode_workspace_bytes(desc.ctypes.data, B)), dtype=torch.uint8, device=dev)
    dd = torch.as_tensor(desc.view(np.uint8)).to(dev)
    ssd_hip.check(lib.ssd_png_encode(ssd_hip.ptr(rgb), rgb.numel(), desc.ctypes.data, ssd_hip.ptr(dd), B, ssd_hip.ptr(out), out.numel(),
                                     offsets.data_ptr() + 4, ssd_hip.ptr(ws), ws.numel(), ssd_hip.stream()), "ssd_png_encode")
    off = offsets.cpu().numpy()
    assert off[0] == -7 and off[-1] == -7 and off[1] == 0
    host = store.cpu().numpy()
    end = int(off[B + 1])
    assert (host[:guard] == 0xA5).all() and (host[guard + end:] == 0xA5).all()       # past offsets[B]: as it was
    for b, c in enumerate(picked):
        assert host[guard + off[1 + b]:guard + off[2 + b]].tobytes() == host_files[c[0]], c[0]


def test_outside_the_limits_the_bare_call_refuses_and_encode_png_batch_falls_back_to_pillow(monkeypatch):
    rgb = next(c for c in CASES if c[0] == "shape_2x3")[1]
    dev_rgb = torch.as_tensor(rgb).to(ssd_hip.device())
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        data_utils.png_pack_batch(dev_rgb.reshape(-1), [(2, 3)], [6])                # a filter outside 0..5, through the bare call
    monkeypatch.setitem(ssd_hip.PNG_FILTERS, "adaptive", 6)                         # the same refusal under encode_png_batch
    got = data_utils.encode_png_batch([dev_rgb, dev_rgb])
    assert len(got) == 2
    for blob in got:
        assert np.array_equal(_decode(blob), rgb)
    buf = io.BytesIO()
    from PIL import Image
    Image.fromarray(rgb).save(buf, "PNG")
    assert got[0] == buf.getvalue()                                                 # Pillow wrote it
    with pytest.raises(ValueError):
        data_utils.encode_png_batch([torch.as_tensor(rgb)])                         # host tensors are refused, as for JPEG
    with pytest.raises(ValueError):
        data_utils.encode_png_batch([dev_rgb], filter="best")


def _drawn_batch():
    rng = np.random.default_rng(5)
    B, T, H, W = 3, 6, 96, 128
    imgs = rng.random((B, H, W, 3)).astype(np.float32)
    y1, x1 = rng.uniform(0, 0.6, (B, T)), rng.uniform(0, 0.6, (B, T))
    boxes = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.4, (B, T)), x1 + rng.uniform(0.1, 0.4, (B, T))], -1).astype(np.float32)
    labels = rng.integers(1, len(dc.LABELS), (B, T))
    probs = rng.uniform(0.3, 1.0, (B, T)).astype(np.float32)
    return imgs, boxes, labels, probs


def test_drawn_detections_with_the_switch_decode_to_the_drawn_tensor_and_without_it_are_pillows_bytes(tmp_path, monkeypatch):
    from PIL import Image
    imgs, boxes, labels, probs = _drawn_batch()
    drawn = du.draw_detections_batch(ssd_hip.to_dev(imgs), boxes, labels, probs, dc.LABELS, colors=dc.colors())
    host = drawn.cpu().numpy()
    monkeypatch.setenv("SSD_PNG_GPU", "1")
    du._present(drawn, str(tmp_path / "gpu"), 5, False, out_format="png")
    assert sorted(f.name for f in (tmp_path / "gpu").iterdir()) == ["img_%05d.png" % (5 + i) for i in range(3)]
    for i in range(3):
        with open(str(tmp_path / "gpu" / ("img_%05d.png" % (5 + i))), "rb") as f:
            blob = f.read()
        assert np.array_equal(_decode(blob), host[i]), i
        assert blob == pc.host_encode(host[i], 5)[1], i
    case = dc.cases()[0]                                                            # the public functions reach the same road
    one = du.draw_bboxes_with_labels(case["img"], case["boxes"], case["labels"], case["probs"], dc.LABELS, colors=case["colors"],
                                     out_dir=str(tmp_path / "one"), out_format="png")
    with open(str(tmp_path / "one" / "img_00000.png"), "rb") as f:
        blob = f.read()
    assert np.array_equal(_decode(blob), one.cpu().numpy()) and blob == pc.host_encode(one.cpu().numpy(), 5)[1]
    for setting in (None, "0", "yes"):                                              # unset or anything else: Pillow's loop, byte for byte
        if setting is None:
            monkeypatch.delenv("SSD_PNG_GPU")
        else:
            monkeypatch.setenv("SSD_PNG_GPU", setting)
        d = tmp_path / ("pil_%s" % setting)
        du._present(drawn, str(d), 0, False, out_format="png")
        for i, a in enumerate(host):
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, "PNG")
            with open(str(d / ("img_%05d.png" % i)), "rb") as f:
                assert f.read() == buf.getvalue(), (setting, i)


def test_more_rows_than_the_filter_kernels_grid():
    """The filter kernel launches at most 2^20 workgroups and strides over the rows beyond: 65 images of 16384 x 1 are
    1 064 960 rows (3 MB of pixels), so the last 16 384 rows are a workgroup's second row."""
    rng = np.random.default_rng(11)
    kinds = [rng.integers(0, 256, (16384, 1, 3), dtype=np.uint8), np.repeat(rng.integers(0, 256, (64, 1, 3), dtype=np.uint8), 256, 0)]
    want = [pc.host_encode(a, 5)[1] for a in kinds]
    dev = [torch.as_tensor(a).to(ssd_hip.device()) for a in kinds]
    got = data_utils.encode_png_batch([dev[b % 2] for b in range(65)])
    assert got == [want[b % 2] for b in range(65)]
    assert np.array_equal(_decode(got[64]), kinds[0]) and np.array_equal(_decode(got[63]), kinds[1])
