"""The device inflater (``ssd_png_inflate``) against Python's ``zlib`` bit for bit and against its host model's status
words: the bare call on ragged batches inside guard bands, its refusals with nothing launched, and the roads on top of it
(``decode_png_batch`` / ``decode_image_batch`` / ``custom_data_batches`` with ``SSD_PNG_INFLATE_GPU=1``) against Pillow.
The cases are those of ``png_inflate_cases`` and ``png_decode_cases``: all small (the largest inflates to 72 KB)."""
import ctypes
import io
import zlib

import numpy as np
import pytest
import torch

import png_decode_cases as dc
import png_inflate_cases as ic
import ssd_hip
from utils import data_utils

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")

ACCEPTED = ic.all_accepted()
REFUSED = ic.refusal_cases()
GUARD = 4096
FILL = 0xA5


@pytest.fixture(scope="module")
def want():
    """name -> zlib's bytes, inflated once for all tests."""
    return {c[0]: zlib.decompress(c[1]) for c in ACCEPTED}


def _layout(cases):
    """One ``ssd_png_inflate`` batch: descriptors | payloads || guard | scanlines | chain lists | guard."""
    B = len(cases)
    desc = np.zeros(B, ssd_hip.PNG_INFLATE_DESC_DTYPE)
    front, total = data_utils._place([desc.nbytes] + [len(c[1]) for c in cases])
    behind, end = data_utils._place([c[2] * (1 + c[3]) for c in cases] + [4 * c[2] for c in cases], total + GUARD)
    desc["zlib_offset"], desc["zlib_bytes"] = front[1:], [len(c[1]) for c in cases]
    desc["dst_offset"], desc["chain_offset"] = behind[:B], behind[B:]
    desc["H"], desc["row_bytes"] = [c[2] for c in cases], [c[3] for c in cases]
    return desc, total, end + GUARD


def _run(cases, edit=None, shift=0, null=None, batch=None):
    """The bare call: ``(rc, scanlines, chain lists, status words, everything else untouched)``."""
    lib, dev = ssd_hip.lib(), ssd_hip.device()
    desc, total, size = _layout(cases)
    host = np.full(size, FILL, np.uint8)
    host[:desc.nbytes] = desc.view(np.uint8)
    for d, c in zip(desc, cases):
        host[int(d["zlib_offset"]):int(d["zlib_offset"]) + len(c[1])] = np.frombuffer(c[1], np.uint8)
    regions = [(int(d["dst_offset"]), int(d["H"]) * (1 + int(d["row_bytes"]))) for d in desc] + [(int(d["chain_offset"]), 4 * int(d["H"])) for d in desc]
    used = desc.copy()
    if edit:
        edit(used)
    packed = torch.from_numpy(host).to(dev)
    store = torch.full((len(cases) + 128,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    args = [packed.data_ptr() + shift, size, used.ctypes.data, packed.data_ptr(), len(cases) if batch is None else batch, store.data_ptr() + 256,
            ssd_hip.stream()]
    if null is not None:
        args[null] = None
    rc = lib.ssd_png_inflate(*args)
    torch.cuda.synchronize()
    after, words = packed.cpu().numpy(), store.cpu().numpy()
    same = after == host
    for at, n in regions:
        same[at:at + n] = True
    untouched = bool(same.all()) and bool((words[:64] == 0x5A5A5A5A).all()) and bool((words[64 + len(cases):] == 0x5A5A5A5A).all())
    rows = [after[at:at + n].tobytes() for at, n in regions[:len(cases)]]
    lists = [after[at:at + n].view(np.int32).copy() for at, n in regions[len(cases):]]
    nothing = bool((after == host).all()) and bool((words == 0x5A5A5A5A).all())
    return {"rc": rc, "rows": rows, "lists": lists, "status": words[64:64 + len(cases)].copy(), "untouched": untouched, "nothing": nothing}


def _chain_rule(data, H, rb):
    types = np.frombuffer(data, np.uint8)[::1 + rb]
    starts = sorted(set([0] + [int(y) for y in np.flatnonzero(types <= 1)]))
    return np.array(starts + [H] * (H - len(starts)), np.int32)


def _host_status(stream, H, rb):
    out = np.zeros(H * (1 + rb), np.uint8)
    status = ctypes.c_int(-1)
    assert ssd_hip.lib().ssd_png_inflate_host(stream, len(stream), out.ctypes.data, out.nbytes, rb, ctypes.byref(status)) == 0
    return status.value


@pytest.fixture(scope="module")
def ragged():
    return _run(ACCEPTED)


def test_the_ragged_batch_gives_zlibs_bytes_status_0_and_the_chain_lists(ragged, want):
    assert ragged["rc"] == 0, ssd_hip.lib().ssd_last_error().decode()
    assert ragged["status"].tolist() == [0] * len(ACCEPTED)
    assert ragged["untouched"]
    for c, rows, chain in zip(ACCEPTED, ragged["rows"], ragged["lists"]):
        assert rows == want[c[0]], c[0]
        assert np.array_equal(chain, _chain_rule(want[c[0]], c[2], c[3])), c[0]


def test_every_case_alone_and_the_reversed_batch_give_the_same_bytes(want):
    rev = _run(ACCEPTED[::-1])
    assert rev["rc"] == 0 and not rev["status"].any() and rev["untouched"]
    for c, rows in zip(ACCEPTED[::-1], rev["rows"]):
        assert rows == want[c[0]], c[0]
    for c in ACCEPTED:
        one = _run([c])
        assert one["rc"] == 0 and one["status"].tolist() == [0] and one["untouched"], c[0]
        assert one["rows"][0] == want[c[0]], c[0]
        assert np.array_equal(one["lists"][0], _chain_rule(want[c[0]], c[2], c[3])), c[0]


def test_two_calls_give_equal_bytes_and_an_empty_batch_is_a_no_op(ragged):
    again = _run(ACCEPTED)
    assert again["rows"] == ragged["rows"]
    assert all(np.array_equal(a, b) for a, b in zip(again["lists"], ragged["lists"]))
    assert ssd_hip.lib().ssd_png_inflate(None, 0, None, None, 0, None, ssd_hip.stream()) == 0
    assert _run(ACCEPTED[:2], batch=0)["nothing"]


def test_a_batch_of_accepted_and_refused_streams(want):
    mixed = []
    for k, r in enumerate(REFUSED):
        mixed += [r[:4], ACCEPTED[k % len(ACCEPTED)]]
    got = _run(mixed)
    assert got["rc"] == 0 and got["untouched"]
    for c, rows, chain, status in zip(mixed, got["rows"], got["lists"], got["status"]):
        assert int(status) == _host_status(*c[1:]), c[0]
        if c[0] in want:
            assert status == 0 and rows == want[c[0]], c[0]
            assert np.array_equal(chain, _chain_rule(want[c[0]], c[2], c[3])), c[0]
        else:
            assert status != 0, c[0]
    for r, status in zip(REFUSED, got["status"][0::2]):
        assert int(status) == ssd_hip.PNG_INFLATE_STATUS[r[4]], r[0]


def test_the_bare_call_refuses_with_nothing_launched():
    cases = ACCEPTED[:3]
    assert _run(cases)["rc"] == 0

    def field(name, value, b=1):
        def edit(desc):
            desc[b][name] = value
        return edit

    def same_as(name, b, other_name, other):
        def edit(desc):
            desc[b][name] = desc[other][other_name]
        return edit
    invalid = [dict(edit=field("H", 0)), dict(edit=field("H", -1)), dict(edit=field("row_bytes", 0)), dict(edit=field("zlib_bytes", -1)),
               dict(edit=field("reserved", 1)), dict(edit=field("zlib_offset", 8)), dict(edit=field("dst_offset", 8)),
               dict(edit=field("chain_offset", 4)), dict(edit=field("zlib_offset", -16)), dict(edit=field("dst_offset", -16)),
               dict(edit=field("zlib_offset", 1 << 40)), dict(edit=field("dst_offset", 1 << 40)), dict(edit=field("chain_offset", 1 << 40)),
               dict(edit=field("zlib_bytes", 1 << 40)), dict(edit=same_as("dst_offset", 1, "dst_offset", 0)),
               dict(edit=same_as("chain_offset", 1, "dst_offset", 2)), dict(edit=same_as("dst_offset", 2, "zlib_offset", 0)),
               dict(edit=same_as("chain_offset", 0, "chain_offset", 2)), dict(shift=8), dict(null=0), dict(null=2), dict(null=3), dict(null=5),
               dict(batch=-1)]
    for kw in invalid:
        got = _run(cases, **kw)
        assert (got["rc"], got["nothing"]) == (dc.INVALID, True), kw
    cap = ssd_hip.PNG_INFLATE_MAX_STREAM
    for kw in (dict(edit=field("row_bytes", cap)), dict(edit=field("row_bytes", cap // cases[1][2])), dict(batch=65536)):
        got = _run(cases, **kw)
        assert (got["rc"], got["nothing"]) == (dc.UNSUPPORTED, True), kw
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        ssd_hip.check(_run(cases, batch=65536)["rc"], "ssd_png_inflate")
    with pytest.raises(ValueError):
        ssd_hip.check(_run(cases, edit=field("H", 0))["rc"], "ssd_png_inflate")


# ---- the roads on top ----------------------------------------------------------------------------------------------------
def _no_host_inflate(monkeypatch):
    def refuse(*args, **kw):
        raise AssertionError("the host inflate was used")
    monkeypatch.setattr(zlib, "decompressobj", refuse)


def test_decode_png_batch_gives_pillows_pixels_without_the_host_inflate(monkeypatch):
    files = dc.accepted_cases()
    expect = [dc.pillow_outcome(c["blob"]) for c in files]
    assert all(kind == "pixels" for kind, _ in expect)
    monkeypatch.setenv("SSD_PNG_INFLATE_GPU", "1")
    assert data_utils.png_inflate_gpu_enabled()
    _no_host_inflate(monkeypatch)
    batch = data_utils.decode_png_batch([c["blob"] for c in files])
    assert batch.kinds == [ssd_hip.PNG_SCANLINES] * len(files)
    for c, im, (_, px) in zip(files, batch.images, expect):
        assert np.array_equal(im.cpu().numpy(), px), c["name"]
    one = data_utils.decode_png_batch([data_utils.png_host_parse(files[0]["blob"])])
    assert np.array_equal(one.images[0].cpu().numpy(), expect[0][1])


def test_refused_files_give_pillows_pixels_or_pillows_exception(monkeypatch):
    good = dc.accepted_cases()[0]["blob"]
    files = [(name, blob) for name, blob, _ in dc.refusal_cases()] + [(r[0], ic.as_png(*r[1:4])) for r in REFUSED]
    for switch in ("0", "1"):
        monkeypatch.setenv("SSD_PNG_INFLATE_GPU", switch)
        for name, blob in files:
            kind, expect = dc.pillow_outcome(blob)
            if kind == "raises":
                with pytest.raises(expect):
                    data_utils.decode_png_batch([good, blob])
            else:
                batch = data_utils.decode_png_batch([good, blob])
                assert batch.kinds[0] == ssd_hip.PNG_SCANLINES, name
                assert np.array_equal(batch.images[0].cpu().numpy(), dc.pillow_outcome(good)[1]), name
                assert np.array_equal(batch.images[1].cpu().numpy(), expect), name


def _jpeg_bytes(px):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", quality=85)
    return buf.getvalue()


def _mixed():
    rng = np.random.default_rng(12)
    by_name = {c["name"]: c["blob"] for c in dc.accepted_cases()}
    jpeg = _jpeg_bytes(rng.integers(0, 256, (21, 35, 3), dtype=np.uint8))
    array = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    png = [by_name[n] for n in ("format_ct3_d4_13x5", "band_paeth_5x65", "pillow_smooth_RGBA", "chains_pattern_6x11")]
    big = ic.as_png(*next(c for c in ACCEPTED if c[0] == "rgb_200x120_level6")[1:])
    entries = [png[0], jpeg, array, png[1], big, jpeg, png[2], png[3]]
    expect = [dc.pillow_outcome(x)[1] if isinstance(x, bytes) else x for x in entries]
    return entries, expect


def test_a_mixed_batch_of_streams_scanlines_jpeg_and_raw_keeps_its_order(monkeypatch):
    entries, expect = _mixed()
    items = list(entries)
    items[0] = data_utils.png_host_parse(entries[0])
    items[3] = data_utils.png_host_inflate(entries[3])
    items[4] = data_utils.png_host_parse(entries[4])
    items[6] = data_utils.png_host_inflate(entries[6])
    assert isinstance(items[0], data_utils.PngStream) and isinstance(items[3], data_utils.PngScanlines)
    monkeypatch.setenv("SSD_PNG_INFLATE_GPU", "1")                                  # entries[7]: bytes, parsed inside
    batch = data_utils.decode_image_batch(items)
    assert batch.kinds == [ssd_hip.PNG_SCANLINES, ssd_hip.JPEG_COEFFICIENTS, ssd_hip.JPEG_RAW, ssd_hip.PNG_SCANLINES, ssd_hip.PNG_SCANLINES,
                           ssd_hip.JPEG_COEFFICIENTS, ssd_hip.PNG_SCANLINES, ssd_hip.PNG_SCANLINES]
    for b, (im, px) in enumerate(zip(batch.images, expect)):
        assert np.array_equal(im.cpu().numpy(), px), b
    png_only = data_utils.decode_png_batch([items[3], items[0], entries[2], items[4], items[6]])
    for b, (im, k) in enumerate(zip(png_only.images, (3, 0, 2, 4, 6))):
        assert np.array_equal(im.cpu().numpy(), expect[k]), b
    assert png_only.kinds == [ssd_hip.PNG_SCANLINES, ssd_hip.PNG_SCANLINES, ssd_hip.JPEG_RAW, ssd_hip.PNG_SCANLINES, ssd_hip.PNG_SCANLINES]


def test_directory_runs_with_the_switch_on_and_off_are_bitwise_equal(tmp_path, monkeypatch):
    entries, expect = _mixed()
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
    real = lib.ssd_png_inflate

    class Counting(object):
        def __getattr__(self, name):
            return getattr(lib, name)

        def ssd_png_inflate(self, *args):
            calls.append(args[4])
            return real(*args)
    monkeypatch.setattr(ssd_hip, "_lib", Counting())

    def run():
        return [imgs.clone() for imgs, _, _ in data_utils.custom_data_batches(paths, 24, 32, 5)]
    monkeypatch.setenv("SSD_PNG_DECODE_GPU", "1")
    monkeypatch.delenv("SSD_PNG_INFLATE_GPU", raising=False)
    off = run()
    assert calls == []
    monkeypatch.setenv("SSD_PNG_INFLATE_GPU", "1")
    on = run()
    assert calls == [3, 2]                                                          # two batches: three PNG files, then two
    monkeypatch.delenv("SSD_PNG_DECODE_GPU")                                        # the inflate switch alone changes nothing
    alone = run()
    assert calls == [3, 2]
    expect_resized = data_utils.resize_lanczos_batch(expect, 24, 32)
    for got in (off, on, alone):
        assert [len(g) for g in got] == [5, 3]
        assert torch.equal(torch.cat(got), expect_resized)
