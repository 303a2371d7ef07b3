"""The device half of the JPEG decoder (``ssd_jpeg_decode`` through ``data_utils.decode_jpeg_batch``) against the
Pillow-written fixture and live Pillow, the decode feeding the two resize launches in place, and the GPU-decoder
road of ``voc_batches`` (``SSD_JPEG_GPU``).  Bit-exactness is the bar: no tolerance anywhere."""
import ctypes
import io

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import ssd_hip
import voc_cases as vc
from utils import data_utils

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


@pytest.fixture(scope="module")
def real():
    blob = jc.real_size_blob()
    rc, info, _ = jc.parse(blob)
    rc2, coef, _ = jc.entropy_decode(blob, info)
    assert rc == 0 and rc2 == 0
    return blob, jc.pillow_decode(blob) if jc.pillow_is_turbo() else jc.restate(info, coef)


def test_all_fixture_cases_in_one_ragged_call(fixture):
    names = [c[0] for c in jc.cases()]
    blobs = [fixture[n][0] for n in names]
    runs = []
    for _ in range(2):
        jb = data_utils.decode_jpeg_batch(blobs)
        assert jb.kinds == [ssd_hip.JPEG_COEFFICIENTS] * len(names)             # nothing took the Pillow road
        assert all((int(o) & 15) == 0 for o in jb.desc["src_offset"])
        runs.append([_np(im) for im in jb.images])
    for n, a, b in zip(names, runs[0], runs[1]):
        want = fixture[n][1]
        assert a.dtype == np.uint8 and a.shape == want.shape, n
        assert np.array_equal(a, want), (n, np.argwhere(a != want)[:4])
        assert np.array_equal(a, b), n


def test_coefficient_and_raw_pixel_images_mix_in_one_batch(fixture, real):
    from PIL import Image
    rgb = jc.content(24, 40, "444", "smooth")
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", progressive=True)                    # unsupported: Pillow decodes, raw pixels travel
    prog = buf.getvalue()
    png = io.BytesIO()
    Image.fromarray(rgb).save(png, "PNG")
    raw = jc.content(7, 5, "444", "noise")
    prepared = data_utils.jpeg_host_decode(fixture["size_40x24_420"][0])       # what a pool thread hands over
    assert isinstance(prepared, data_utils.JpegCoefficients)
    entries = [fixture["size_17x33_420"][0], prog, raw, real[0], png.getvalue(), prepared, fixture["size_1x1_L"][0]]
    want = [fixture["size_17x33_420"][1], jc.pillow_decode(prog), raw, real[1], rgb, fixture["size_40x24_420"][1],
            fixture["size_1x1_L"][1]]
    jb = data_utils.decode_jpeg_batch(entries)
    assert jb.kinds == [0, 1, 1, 0, 1, 0, 0]
    for i, (im, w) in enumerate(zip(jb.images, want)):
        assert np.array_equal(_np(im), w), i
    with pytest.raises(Exception):                                                # Pillow raises what it raised before
        data_utils.decode_jpeg_batch([fixture["size_17x33_420"][0][:40]])
    cut = real[0][:len(real[0]) // 2]                                             # whole header, half a scan: INVALID -> Pillow
    try:
        expect = jc.pillow_decode(cut)
    except Exception as exc:
        with pytest.raises(type(exc)):
            data_utils.decode_jpeg_batch([cut, fixture["size_8x8_444"][0]])
    else:
        jb = data_utils.decode_jpeg_batch([cut, fixture["size_8x8_444"][0]])
        assert jb.kinds == [1, 0] and np.array_equal(_np(jb.images[0]), expect)


def test_decode_feeds_the_bilinear_resize_in_place(real, fixture):
    blobs = [real[0], fixture["size_33x17_422"][0], fixture["size_17x33_L"][0]]
    pixels = [real[1], fixture["size_33x17_422"][1], fixture["size_17x33_L"][1]]
    want = data_utils.preprocess_ragged_batch(pixels, 300, 300)
    got = data_utils.preprocess_jpeg_batch(blobs, 300, 300)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 300, 300, 3)
    assert np.array_equal(_np(got).view(np.uint32), _np(want).view(np.uint32))


def test_decode_feeds_the_lanczos_resize_in_place(real, fixture):
    blobs = [real[0], fixture["size_33x17_422"][0], fixture["size_40x24_420"][0]]
    pixels = [real[1], fixture["size_33x17_422"][1], fixture["size_40x24_420"][1]]
    want_u8 = torch.empty((3, 300, 300, 3), dtype=torch.uint8, device=ssd_hip.device())
    got_u8 = torch.empty_like(want_u8)
    want = data_utils.resize_lanczos_batch(pixels, 300, 300, out_u8=want_u8)
    got = data_utils.resize_lanczos_jpeg_batch(blobs, 300, 300, out_u8=got_u8)
    assert np.array_equal(_np(got).view(np.uint32), _np(want).view(np.uint32))
    assert np.array_equal(_np(got_u8), _np(want_u8))


def test_decoding_into_a_view_leaves_the_rest_of_the_buffer_alone(fixture):
    names = ["size_7x9_420", "size_17x33_444", "size_1x1_422", "size_33x17_L"]
    blobs = [fixture[n][0] for n in names]
    need = sum((fixture[n][1].size + 15) & ~15 for n in names)
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=ssd_hip.device())
    at = 1024 + (-big.data_ptr()) % 16
    jb = data_utils.decode_jpeg_batch(blobs, out_u8=big[at:at + need])
    host = _np(big)
    written = np.zeros(host.size, bool)
    for n, o in zip(names, jb.desc):
        want = fixture[n][1]
        lo = at + int(o["src_offset"])
        assert np.array_equal(host[lo:lo + want.size].reshape(want.shape), want), n
        written[lo:lo + want.size] = True
    assert (host[~written] == 0xA5).all()                                         # the padding between the images too
    with pytest.raises(ValueError):
        data_utils.decode_jpeg_batch(blobs, out_u8=big[at:at + need - 16])
    with pytest.raises(ValueError):
        data_utils.decode_jpeg_batch(blobs, out_u8=big[at + 1:at + 1 + need])


def test_bad_arguments_are_refused_unlaunched(fixture):
    lib = ssd_hip.lib()
    dev = ssd_hip.device()
    blob, want = fixture["size_17x33_420"]
    item = data_utils.jpeg_host_decode(blob)
    layout = data_utils._jpeg_layout([item])
    host = np.zeros(layout["total"], np.uint8)
    data_utils._jpeg_fill(host, [item], layout, [])
    packed = torch.as_tensor(host).to(dev)
    rgb = torch.full((layout["rgb_bytes"] + 64,), 0xA5, dtype=torch.uint8, device=dev)
    ws = torch.zeros(max(layout["plane_bytes"], 16), dtype=torch.uint8, device=dev)
    base = packed.data_ptr()

    def call(desc=None, out_desc=None, B=1, nbytes=None, rgb_bytes=None, ws_bytes=None, packed_ptr=base, rgb_ptr=None):
        d = layout["desc"] if desc is None else desc
        o = layout["out_desc"] if out_desc is None else out_desc
        return lib.ssd_jpeg_decode(packed_ptr, layout["total"] if nbytes is None else nbytes, d.ctypes.data, base, B,
                                   rgb.data_ptr() if rgb_ptr is None else rgb_ptr, layout["rgb_bytes"] if rgb_bytes is None else rgb_bytes,
                                   o.ctypes.data, base + layout["out_at"], ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                   ssd_hip.stream())

    def changed(field, value, which="desc"):
        a = layout[which].copy()
        a[0][field] = value
        return {which: a}
    refused = [
        (call(B=-1), -1), (call(B=70000), -3), (call(packed_ptr=None), -1), (call(rgb_ptr=rgb.data_ptr() + 4), -1),
        (call(nbytes=layout["total"] - 16), -1), (call(rgb_bytes=layout["rgb_bytes"] - 16), -1), (call(ws_bytes=16), -1),
        (call(**changed("kind", 2)), -1), (call(**changed("coef_offset", 8)), -1), (call(**changed("quant_offset", -16)), -1),
        (call(**changed("plane_offset", 4)), -1), (call(**changed("block_start", 1)), -1), (call(**changed("item_start", 1)), -1),
        (call(**changed("H", 16385)), -3), (call(**changed("h_samp", 4)), -3), (call(**changed("components", 2)), -3),
        (call(**changed("H", 16, "out_desc")), -1), (call(**changed("src_offset", 8, "out_desc")), -1),
    ]
    for i, (rc, expect) in enumerate(refused):
        assert rc == expect, (i, rc, lib.ssd_last_error())
    assert lib.ssd_jpeg_decode(None, 0, None, None, 0, None, 0, None, None, None, 0, ssd_hip.stream()) == 0   # B == 0: a no-op
    torch.cuda.synchronize()
    assert (_np(rgb) == 0xA5).all()                                               # nothing was launched
    assert call() == 0
    assert np.array_equal(_np(rgb)[:want.size].reshape(want.shape), want)
    assert lib.ssd_jpeg_decode_workspace_bytes(layout["desc"].ctypes.data, 1) == layout["plane_bytes"]
    assert len(data_utils.decode_jpeg_batch([]).images) == 0
    assert ctypes.sizeof(ssd_hip.JpegInfo) == 504


@pytest.fixture(scope="module")
def devkit(tmp_path_factory):
    root = tmp_path_factory.mktemp("voc_jpeg")
    vc.write_devkit(root)
    return root


@pytest.mark.parametrize("workers", [1, 4])
def test_voc_batches_with_the_gpu_decoder_yield_the_same_bits(devkit, workers, monkeypatch):
    a, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    b, _ = data_utils.get_dataset("voc/2007", "test", str(devkit))
    ds = a.concatenate(b)
    monkeypatch.setenv("SSD_JPEG_GPU", "0")                                       # the Pillow pool
    ref = [(_np(x), gt, gl) for x, gt, gl in data_utils.voc_batches(ds, 4, 300, 300, workers=workers)]
    monkeypatch.setenv("SSD_JPEG_GPU", "1")
    seen = []
    real_decode = data_utils.preprocess_jpeg_batch
    monkeypatch.setattr(data_utils, "preprocess_jpeg_batch", lambda *a, **k: (seen.append(len(a[0])), real_decode(*a, **k))[1])
    got = [(_np(x), gt, gl) for x, gt, gl in data_utils.voc_batches(ds, 4, 300, 300, workers=workers)]
    assert seen == [4, 4, 2]                                                      # the new road was taken
    monkeypatch.delenv("SSD_JPEG_GPU", raising=False)                             # ... and it is the default (measured)
    list(data_utils.voc_batches(ds, 4, 300, 300, workers=workers))
    assert seen == [4, 4, 2] * 2
    assert len(got) == len(ref) == 3
    for (x, gt, gl), (rx, rgt, rgl) in zip(got, ref):
        assert np.array_equal(x.view(np.uint32), rx.view(np.uint32))
        assert np.array_equal(gt, rgt) and np.array_equal(gl, rgl)


def test_custom_images_with_the_gpu_decoder_yield_the_same_bits(tmp_path, fixture, real, monkeypatch):
    from PIL import Image
    (tmp_path / "a.jpg").write_bytes(real[0])
    (tmp_path / "b.jpg").write_bytes(fixture["size_40x24_420"][0])
    Image.fromarray(jc.content(30, 20, "444", "smooth")).save(str(tmp_path / "c.png"))
    np.save(str(tmp_path / "d.npy"), jc.content(9, 11, "444", "noise"))
    paths = data_utils.get_custom_imgs(str(tmp_path))
    monkeypatch.setenv("SSD_JPEG_GPU", "0")
    ref = [_np(x) for x, _, _ in data_utils.custom_data_batches(paths, 300, 300, 3)]
    ref1 = [_np(x) for x, _, _ in data_utils.custom_data_generator(paths[:2], 300, 300)]
    monkeypatch.setenv("SSD_JPEG_GPU", "1")
    got = [_np(x) for x, _, _ in data_utils.custom_data_batches(paths, 300, 300, 3)]
    got1 = [_np(x) for x, _, _ in data_utils.custom_data_generator(paths[:2], 300, 300)]
    assert [g.shape for g in got] == [r.shape for r in ref] == [(3, 300, 300, 3), (1, 300, 300, 3)]
    for g, r in zip(got + got1, ref + ref1):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))
