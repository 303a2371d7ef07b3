"""The host half of the PNG decoder and its host model, without a GPU: ``ssd_png_parse`` fills what the files say and
refuses exactly the refusal list, ``ssd_png_decode_host`` equals Pillow on every accepted case, ``png_host_inflate``
returns scanlines for the accepted cases and the fallback's pixels otherwise, and inflate is bounded by the image."""
import ctypes
import zlib

import numpy as np
import pytest

import png_decode_cases as dc
import ssd_hip
from utils import data_utils

pytest.importorskip("PIL")

ACCEPTED = dc.accepted_cases()
REFUSED = dc.refusal_cases()


def _parse(blob):
    info = ssd_hip.PngInfo()
    return ssd_hip.lib().ssd_png_parse(blob, len(blob), ctypes.byref(info)), info


def _host_model(item):
    i = item.info
    rgb = np.full(i.height * i.width * 3 + 32, 0xA5, np.uint8)
    rc = ssd_hip.lib().ssd_png_decode_host(ctypes.byref(i), item.filtered.ctypes.data, item.filtered.nbytes, rgb[16:].ctypes.data,
                                           i.height * i.width * 3)
    assert rc == 0, ssd_hip.lib().ssd_last_error().decode()
    assert (rgb[:16] == 0xA5).all() and (rgb[-16:] == 0xA5).all()
    return rgb[16:-16].reshape(i.height, i.width, 3)


def _never(blob):
    raise AssertionError("the fallback was asked for an accepted file")


@pytest.mark.parametrize("case", ACCEPTED, ids=[c["name"] for c in ACCEPTED])
def test_parse_fills_the_fields(case):
    rc, info = _parse(case["blob"])
    assert rc == 0, ssd_hip.lib().ssd_last_error().decode()
    assert (info.width, info.height, info.color_type) == (case["W"], case["H"], case["color_type"])
    depth = info.depth
    assert case["depth"] in (None, depth) and depth in (1, 2, 4, 8, 16)
    channels = dc.CHANNELS[info.color_type]
    assert info.channels == channels
    assert info.row_bytes == (info.width * channels * depth + 7) // 8
    assert info.filter_distance == max(1, channels * depth // 8)
    assert info.stream_bytes == info.height * (1 + info.row_bytes)
    # the IDAT payloads, found by a chunk walk of this test's own
    blob, pos, spans = case["blob"], 8, []
    while pos < len(blob):
        n, kind = int.from_bytes(blob[pos:pos + 4], "big"), blob[pos + 4:pos + 8]
        if kind == b"IDAT":
            spans.append((pos, blob[pos + 8:pos + 8 + n]))
        if kind == b"PLTE":
            plte = blob[pos + 8:pos + 8 + n]
            assert info.palette_entries == n // 3
            assert bytes(info.palette) == plte + bytes(768 - n)
        pos += 12 + n
    assert info.idat_count == len(spans) and info.first_idat == spans[0][0]
    stream = b"".join(s for _, s in spans)
    assert info.idat_bytes == len(stream)
    out = np.zeros(len(stream) + 1, np.uint8)
    assert ssd_hip.lib().ssd_png_idat(blob, len(blob), ctypes.byref(info), out.ctypes.data, len(stream)) == 0
    assert out[:-1].tobytes() == stream and out[-1] == 0
    assert ssd_hip.lib().ssd_png_idat(blob, len(blob), ctypes.byref(info), out.ctypes.data, len(stream) - 1) == dc.INVALID


@pytest.mark.parametrize("name,blob,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_parse_refuses_the_refusal_list_with_the_right_code(name, blob, code):
    rc, info = _parse(blob)
    assert rc == code, (rc, ssd_hip.lib().ssd_last_error().decode())
    if rc != 0:
        assert bytes(info) == bytes(ctypes.sizeof(info))                             # nothing half-filled


def test_every_accepted_case_takes_the_device_road_and_the_host_model_equals_pillow():
    """The cap: no accepted case may take the fallback (Pillow decodes every row of the format table, so a file that
    falls back is a bug of the library, not of the input)."""
    fell_back = []
    for case in ACCEPTED:
        kind, want = dc.pillow_outcome(case["blob"])
        assert kind == "pixels", case["name"]
        try:
            item = data_utils.png_host_inflate(case["blob"], fallback=_never)
        except AssertionError:
            fell_back.append(case["name"])
            continue
        assert isinstance(item, data_utils.PngScanlines) and item.filtered.nbytes == item.info.stream_bytes, case["name"]
        assert np.array_equal(_host_model(item), want), case["name"]
    assert fell_back == []


@pytest.mark.parametrize("name,blob,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_a_refused_file_gives_the_fallbacks_pixels_or_its_exception(name, blob, code):
    kind, want = dc.pillow_outcome(blob)
    calls = []

    def fallback(b):
        calls.append(b)
        return data_utils._pillow_rgb(b)
    if kind == "raises":
        with pytest.raises(want):
            data_utils.png_host_inflate(blob, fallback=fallback)
    else:
        got = data_utils.png_host_inflate(blob, fallback=fallback)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert calls == [blob]


def test_the_host_model_refuses_what_it_must():
    item = data_utils.png_host_inflate(ACCEPTED[0]["blob"], fallback=_never)
    i, lib = item.info, ssd_hip.lib()
    n = i.height * i.width * 3
    rgb = np.full(n, 0xA5, np.uint8)
    F = item.filtered.copy()
    assert lib.ssd_png_decode_host(ctypes.byref(i), F.ctypes.data, F.nbytes - 1, rgb.ctypes.data, n) == dc.INVALID
    assert lib.ssd_png_decode_host(ctypes.byref(i), F.ctypes.data, F.nbytes, rgb.ctypes.data, n - 1) == dc.INVALID
    assert lib.ssd_png_decode_host(ctypes.byref(i), None, F.nbytes, rgb.ctypes.data, n) == dc.INVALID
    F[(1 + i.row_bytes) * 2] = 5
    assert lib.ssd_png_decode_host(ctypes.byref(i), F.ctypes.data, F.nbytes, rgb.ctypes.data, n) == dc.INVALID
    assert (rgb == 0xA5).all()


def test_inflate_is_bounded_by_the_image(monkeypatch):
    """A stream that expands far past the image is refused after at most one byte more than the image needs."""
    seen = []
    real = zlib.decompressobj

    class Bounded(object):
        def __init__(self):
            self.z = real()

        def decompress(self, data, max_length=0):
            out = self.z.decompress(data, max_length)
            seen.append((max_length, len(out)))
            return out

        def __getattr__(self, name):
            return getattr(self.z, name)
    monkeypatch.setattr(zlib, "decompressobj", Bounded)
    expected = 5 * (1 + 39)
    bomb = dc.write_png(13, 5, 2, 8, None, None, stream=zlib.compress(bytes(1 << 24), 9))
    got = data_utils.png_host_inflate(bomb, fallback=lambda b: "fallback")
    assert got == "fallback"
    assert seen == [(expected + 1, expected + 1)]
