"""The device PNG decoder (``ssd_png_decode`` through ``data_utils.decode_png_batch`` / ``decode_image_batch``) against
Pillow's decode of the same bytes, bit for bit, and against the host model; then the roads around it: guard regions,
repeatability, the bare call's refusals, the Pillow fallback, mixed batches, the directory loader with the switch on and
off, and the round trip through the device encoder.  The cases are those of ``png_decode_cases``: all tiny."""
import ctypes
import io

import numpy as np
import pytest
import torch

import png_decode_cases as dc
import ssd_hip
from utils import data_utils

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")

ACCEPTED = dc.accepted_cases()
REFUSED = dc.refusal_cases()
GUARD = 4096


@pytest.fixture(scope="module")
def want():
    """name -> Pillow's pixels, decoded once for all tests."""
    out = {}
    for case in ACCEPTED:
        kind, px = dc.pillow_outcome(case["blob"])
        assert kind == "pixels", case["name"]
        out[case["name"]] = px
    return out


@pytest.fixture(scope="module")
def ragged():
    """The whole accepted list as ONE ragged batch."""
    return data_utils.decode_png_batch([c["blob"] for c in ACCEPTED])


def _pixels(batch):
    host = batch.rgb.cpu().numpy()
    return [host[int(o["src_offset"]):int(o["src_offset"]) + int(o["H"]) * int(o["W"]) * 3].reshape(int(o["H"]), int(o["W"]), 3)
            for o in batch.desc]


def test_ragged_batch_equals_pillow_bit_for_bit(ragged, want):
    got = _pixels(ragged)
    assert len(got) == len(ACCEPTED)
    for case, px in zip(ACCEPTED, got):
        assert np.array_equal(px, want[case["name"]]), case["name"]
    assert ragged.kinds == [ssd_hip.PNG_SCANLINES] * len(ACCEPTED)
    for case, im in zip(ACCEPTED, ragged.images):
        assert np.array_equal(im.cpu().numpy(), want[case["name"]]), case["name"]


def test_ragged_batch_equals_the_host_model(ragged):
    for case, px in zip(ACCEPTED, _pixels(ragged)):
        item = data_utils.png_host_inflate(case["blob"])
        i = item.info
        model = np.zeros((i.height, i.width, 3), np.uint8)
        assert ssd_hip.lib().ssd_png_decode_host(ctypes.byref(i), item.filtered.ctypes.data, item.filtered.nbytes, model.ctypes.data,
                                                 model.nbytes) == 0
        assert np.array_equal(px, model), case["name"]


def test_every_case_alone_and_the_reversed_batch_give_the_same_pixels(want):
    rev = ACCEPTED[::-1]
    for case, px in zip(rev, _pixels(data_utils.decode_png_batch([c["blob"] for c in rev]))):
        assert np.array_equal(px, want[case["name"]]), case["name"]
    for case in ACCEPTED:
        one = data_utils.decode_png_batch([case["blob"]])
        assert one.kinds == [ssd_hip.PNG_SCANLINES]
        assert np.array_equal(one.images[0].cpu().numpy(), want[case["name"]]), case["name"]


def test_two_calls_give_equal_bytes_and_an_empty_batch_is_a_no_op(ragged):
    again = data_utils.decode_png_batch([c["blob"] for c in ACCEPTED])
    for a, b in zip(_pixels(ragged), _pixels(again)):
        assert np.array_equal(a, b)
    empty = data_utils.decode_png_batch([])
    assert empty.images == [] and empty.kinds == [] and len(empty.desc) == 0
    assert ssd_hip.lib().ssd_png_decode(None, 0, None, None, 0, None, 0, None, 0, ssd_hip.stream()) == 0


def _guarded(nbytes):
    store = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=ssd_hip.device())
    assert store.data_ptr() % 16 == 0
    return store, store[GUARD:GUARD + nbytes]


def test_guard_bands_and_padding_are_untouched_and_out_u8_is_honoured(ragged, want):
    nbytes = sum((int(o["H"]) * int(o["W"]) * 3 + 15) & ~15 for o in ragged.desc)
    store, out = _guarded(nbytes)
    batch = data_utils.decode_png_batch([c["blob"] for c in ACCEPTED], out_u8=out)
    assert batch.rgb.data_ptr() == out.data_ptr()
    host = store.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + nbytes:] == 0xA5).all()
    written = np.zeros(nbytes, bool)
    for case, o in zip(ACCEPTED, batch.desc):
        at, n = int(o["src_offset"]), int(o["H"]) * int(o["W"]) * 3
        assert at % 16 == 0
        assert np.array_equal(host[GUARD + at:GUARD + at + n].reshape(want[case["name"]].shape), want[case["name"]]), case["name"]
        written[at:at + n] = True
    assert (host[GUARD:GUARD + nbytes][~written] == 0xA5).all()
    with pytest.raises(ValueError):
        data_utils.decode_png_batch([ACCEPTED[0]["blob"]], out_u8=out[1:])
    with pytest.raises(ValueError):
        data_utils.decode_png_batch([c["blob"] for c in ACCEPTED], out_u8=out[:nbytes - 16])


def _bare(items, edit=None, rgb_cut=0, ws_cut=0, shift=(0, 0, 0), null=None):
    """``ssd_png_decode`` itself on a guarded output, with one thing wrong: the return code and whether anything was
    written."""
    lib, dev = ssd_hip.lib(), ssd_hip.device()
    layout = data_utils._png_decode_layout(items)
    host = np.zeros(layout["total"], np.uint8)
    data_utils._png_decode_fill(host, items, layout)
    desc = layout["desc"].copy()
    if edit:
        edit(desc)
    packed = torch.from_numpy(host).to(dev)
    store, out = _guarded(max(layout["rgb_bytes"], 16) + 16)
    ws = torch.zeros(max(layout["raw_bytes"], 16) + 16, dtype=torch.uint8, device=dev)
    args = [packed.data_ptr() + shift[0], layout["total"], desc.ctypes.data, packed.data_ptr(), len(items), out.data_ptr() + shift[1],
            max(layout["rgb_bytes"], 16) - rgb_cut, ws.data_ptr() + shift[2], max(layout["raw_bytes"], 16) - ws_cut, ssd_hip.stream()]
    if null is not None:
        args[null] = None
    rc = lib.ssd_png_decode(*args)
    torch.cuda.synchronize()
    return rc, bool((store.cpu().numpy() == 0xA5).all())


def test_the_bare_call_refuses_with_nothing_launched():
    items = [data_utils.png_host_inflate(c["blob"]) for c in ACCEPTED[:3]]
    assert _bare(items) == (0, False)

    def field(name, value, b=1):
        def edit(desc):
            desc[b][name] = value
        return edit
    big = ssd_hip.MAX_IMAGE_SIDE + 1
    assert _bare(items, field("W", big)) == (dc.UNSUPPORTED, True)
    assert _bare(items, field("H", big)) == (dc.UNSUPPORTED, True)
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        ssd_hip.check(_bare(items, field("H", big))[0], "ssd_png_decode")
    invalid = [dict(edit=field("W", 0)), dict(edit=field("H", -1)), dict(edit=field("depth", 3)),
               dict(edit=field("color_type", 5)), dict(edit=field("color_type", 0)), dict(edit=field("src_offset", 8)), dict(edit=field("src_offset", -16)),
               dict(edit=field("src_offset", 1 << 40)), dict(edit=field("src_offset", 0, 2)), dict(edit=field("dst_offset", 8)),
               dict(edit=field("dst_offset", 0, 2)), dict(edit=field("dst_offset", 1 << 40)), dict(edit=field("chain_offset", 4)),
               dict(edit=field("chain_offset", 1 << 40)), dict(edit=field("chains", 0)), dict(edit=field("chains", 1 << 20)),
               dict(edit=field("chain_start", 7)), dict(edit=field("row_start", 3)), dict(edit=field("raw_offset", 8)),
               dict(rgb_cut=16), dict(ws_cut=16), dict(shift=(8, 0, 0)), dict(shift=(0, 8, 0)), dict(shift=(0, 0, 8)),
               dict(null=0), dict(null=2), dict(null=3), dict(null=5), dict(null=7)]
    for kw in invalid:
        assert _bare(items, **kw) == (dc.INVALID, True), kw
    palette = [data_utils.png_host_inflate(next(c for c in ACCEPTED if c["color_type"] == 3)["blob"])]
    assert _bare(palette) == (0, False)
    assert _bare(palette, field("palette_offset", 8, 0)) == (dc.INVALID, True)
    assert _bare(palette, field("palette_offset", 1 << 40, 0)) == (dc.INVALID, True)
    with pytest.raises(ValueError):
        ssd_hip.check(_bare(items, field("W", 0))[0], "ssd_png_decode")
    assert ssd_hip.lib().ssd_png_decode_workspace_bytes(None, 3) == 0


def test_the_refusal_list_gives_pillows_pixels_or_pillows_exception():
    for name, blob, _ in REFUSED:
        kind, want = dc.pillow_outcome(blob)
        if kind == "raises":
            with pytest.raises(want):
                data_utils.decode_png_batch([ACCEPTED[0]["blob"], blob])
        else:
            batch = data_utils.decode_png_batch([ACCEPTED[0]["blob"], blob])
            assert batch.kinds == [ssd_hip.PNG_SCANLINES, ssd_hip.JPEG_RAW], name
            assert np.array_equal(batch.images[1].cpu().numpy(), want), name


def _jpeg_bytes(px):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", quality=85)
    return buf.getvalue()


def _pillow(blob):
    return dc.pillow_outcome(blob)[1]


def _mixed():
    rng = np.random.default_rng(11)
    jpeg = _jpeg_bytes(rng.integers(0, 256, (21, 35, 3), dtype=np.uint8))
    array = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    png = [next(c for c in ACCEPTED if c["name"] == n)["blob"] for n in ("format_ct3_d4_13x5", "band_paeth_5x65", "pillow_smooth_RGBA")]
    grey16 = next(r for r in REFUSED if r[0] == "grey_16")[1]
    entries = [png[0], jpeg, array, grey16, png[1], jpeg, png[2]]
    expect = [_pillow(png[0]), _pillow(jpeg), array, _pillow(grey16), _pillow(png[1]), _pillow(jpeg), _pillow(png[2])]
    kinds = [ssd_hip.PNG_SCANLINES, ssd_hip.JPEG_COEFFICIENTS, ssd_hip.JPEG_RAW, ssd_hip.JPEG_RAW, ssd_hip.PNG_SCANLINES,
             ssd_hip.JPEG_COEFFICIENTS, ssd_hip.PNG_SCANLINES]
    return entries, expect, kinds


def test_a_mixed_batch_gives_every_image_in_order():
    entries, expect, kinds = _mixed()
    batch = data_utils.decode_image_batch(entries)
    assert batch.kinds == kinds
    for b, (im, px) in enumerate(zip(batch.images, expect)):
        assert np.array_equal(im.cpu().numpy(), px), b
    for got, px in zip(_pixels(batch), expect):                                     # the descriptors say the same
        assert np.array_equal(got, px)
    # the two consumers on top of it, against the same functions on Pillow's pixels
    assert torch.equal(data_utils.resize_lanczos_image_batch(entries, 30, 30), data_utils.resize_lanczos_batch(expect, 30, 30))
    assert torch.equal(data_utils.preprocess_image_batch(entries, 30, 30), data_utils.preprocess_ragged_batch(expect, 30, 30))
    only_jpeg = data_utils.decode_image_batch([entries[1], entries[2]])
    assert only_jpeg.kinds == [ssd_hip.JPEG_COEFFICIENTS, ssd_hip.JPEG_RAW]


def test_directory_runs_with_the_switch_on_and_off_are_bitwise_equal(tmp_path, monkeypatch):
    entries, expect, _ = _mixed()
    paths = []
    for b, x in enumerate(entries):
        if isinstance(x, np.ndarray):
            paths.append(str(tmp_path / ("%02d.npy" % b)))
            np.save(paths[-1], x)
        else:
            paths.append(str(tmp_path / ("%02d.%s" % (b, "png" if x[:4] == b"\x89PNG" else "jpg"))))
            with open(paths[-1], "wb") as f:
                f.write(x)
    calls = []
    lib = ssd_hip.lib()
    real = lib.ssd_png_decode

    class Counting(object):
        def __getattr__(self, name):
            return getattr(lib, name)

        def ssd_png_decode(self, *args):
            calls.append(len(args))
            return real(*args)
    monkeypatch.setattr(ssd_hip, "_lib", Counting())

    def run():
        return [imgs.clone() for imgs, _, _ in data_utils.custom_data_batches(paths, 24, 32, 4)]
    monkeypatch.delenv("SSD_PNG_DECODE_GPU", raising=False)
    off = run()
    assert calls == []
    monkeypatch.setenv("SSD_PNG_DECODE_GPU", "1")
    on = run()
    assert len(calls) == 2                                                          # two batches, each with PNG files
    monkeypatch.setenv("SSD_JPEG_GPU", "0")                                         # JPEG on Pillow, PNG still on the device
    on_jpeg_off = run()
    assert len(calls) == 4
    want = data_utils.resize_lanczos_batch(expect, 24, 32)
    for got in (off, on, on_jpeg_off):
        assert [len(g) for g in got] == [4, 3]
        assert torch.equal(torch.cat(got), want)


def test_round_trip_through_the_device_encoder(monkeypatch):
    monkeypatch.setenv("SSD_PNG_GPU", "1")
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:70, 0:90]
    drawn = np.stack([np.clip(np.stack([128 + 100 * np.sin(yy / (5.0 + b) + c) * np.cos(xx / 7.0) for c in range(3)], -1)
                              + rng.normal(0, 3, (70, 90, 3)), 0, 255) for b in range(3)]).astype(np.uint8)
    batch = torch.as_tensor(drawn).to(ssd_hip.device())
    files = data_utils.encode_png_batch(batch)
    back = data_utils.decode_png_batch(files)
    assert back.kinds == [ssd_hip.PNG_SCANLINES] * 3
    assert torch.equal(torch.stack(back.images), batch)
