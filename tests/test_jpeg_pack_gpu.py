"""The device entropy coder (``ssd_jpeg_pack``; ``data_utils.jpeg_pack_batch``; ``encode_jpeg_batch`` with
``SSD_JPEG_ENTROPY_GPU=1``) against two oracles: the bytes Pillow wrote (tests/golden/jpeg_encode.npz) and, for inputs
the fixture does not hold, the host coder ``ssd_jpeg_entropy_encode`` -- itself held to Pillow by
tests/test_jpeg_encode_cpu.py -- on the downloaded coefficients of the same ``ssd_jpeg_forward`` call.  Byte equality is
the bar: no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import drawing_cases as dc
import jpeg_encode_cases as jc
import ssd_hip
from utils import data_utils
from utils import drawing_utils as du

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in jc.cases()]
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(ssd_hip.device())


def _forward_pack(arrays, subs, qualities):
    """``jpeg_forward_batch`` + ``jpeg_pack_batch`` on host arrays -> (streams, offsets, status, host coder's streams)."""
    tables = np.stack([jc.quality_tables(q) for q in qualities])
    shapes, samplings = [a.shape[:2] for a in arrays], [jc.SAMPLING[s] for s in subs]
    coef, desc = data_utils.jpeg_forward_batch(_dev(np.concatenate([a.reshape(-1) for a in arrays])), shapes, samplings, tables)
    out, offsets, status = data_utils.jpeg_pack_batch(coef, desc, shapes, samplings, tables)
    assert out.dtype == torch.uint8 and offsets.dtype == torch.int32 and status.dtype == torch.int32
    assert tuple(offsets.shape) == (len(arrays) + 1,) and tuple(status.shape) == (len(arrays),)
    out, offsets, status = out.cpu().numpy(), offsets.cpu().numpy(), status.cpu().numpy()
    streams = [out[offsets[b]:offsets[b + 1]].tobytes() for b in range(len(arrays))]
    return streams, offsets, status, _host_streams(coef.cpu().numpy(), desc, shapes, subs, tables)


def _host_streams(coef_host, desc, shapes, subs, tables):
    want = []
    for b, ((H, W), s) in enumerate(zip(shapes, subs)):
        g = jc.Geometry(H, W, *jc.SAMPLING[s])
        at = int(desc[b]["coef_offset"])
        rc, info = jc.lib_info(H, W, s, tables[b])
        rc2, blob, intact = jc.lib_entropy_encode(coef_host[at:at + g.n * 2].view(np.int16), info)
        assert rc == 0 and intact
        want.append(blob if rc2 == 0 else None)
    return want


def test_every_fixture_case_in_one_ragged_batch_equals_pillow(fixture):
    arrays = [fixture[n][0] for n in NAMES]
    streams, offsets, status, host = _forward_pack(arrays, [fixture[n][2] for n in NAMES], [fixture[n][1] for n in NAMES])
    for n, got, again in zip(NAMES, streams, host):
        assert got == fixture[n][3], (n, len(got), len(fixture[n][3]))
        assert again == fixture[n][3], n
    assert offsets.tolist() == [0] + np.cumsum([len(fixture[n][3]) for n in NAMES]).tolist()
    assert not status.any()


def test_streams_that_cross_workgroups_and_scan_chunks():
    """More than 256 blocks and far more than one 224-byte slot per image; 0xFF bytes at every chunk boundary of a stream
    past 100 KB; a flat image whose blocks take 6 bits each, so five share a 32-bit word; a 1x1 image last."""
    noise = jc.content(300, 300, "noise")
    flat = np.full((64, 64, 3), 128, np.uint8)
    arrays = [noise, jc.content(301, 299, "noise"), flat, jc.content(1, 1, "noise")]
    subs, qualities = ["4:2:0", "4:2:2", "4:4:4", "4:2:0"], [100, 95, 75, 75]
    stats = {}
    jc.restate(noise[:64, :64], 100, "4:2:0", stats)                               # on the CPU: such content has stuffed bytes
    assert stats["stuffed"] >= 1
    streams, offsets, status, host = _forward_pack(arrays, subs, qualities)
    assert not status.any() and offsets.tolist() == [0] + np.cumsum([len(s) for s in streams]).tolist()
    for b in range(4):
        assert streams[b] == host[b], (b, len(streams[b]), len(host[b]))
    g = jc.Geometry(300, 300, 2, 2)
    assert g.mcus_x * g.mcus_y * 6 == 2166 and len(streams[0]) > 100 * 1024
    assert streams[0][ssd_hip.JPEG_HEADER_BYTES:-2].count(b"\xff\x00") >= stats["stuffed"]
    assert b"\xff" not in streams[0][ssd_hip.JPEG_HEADER_BYTES:-2].replace(b"\xff\x00", b"")
    assert streams[2] == jc.restate(flat, 75, "4:4:4")
    assert len(streams[2]) < ssd_hip.JPEG_HEADER_BYTES + 3 + 192 + 2                # 6 bits a block after the first three


@pytest.mark.parametrize("setting", ["1", None])
def test_encode_jpeg_batch_equals_the_fixture_on_both_roads(fixture, monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("SSD_JPEG_ENTROPY_GPU", raising=False)
    else:
        monkeypatch.setenv("SSD_JPEG_ENTROPY_GPU", setting)

        def no_pool(workers):
            raise AssertionError("the device coder's road touched the thread pool")
        monkeypatch.setattr(data_utils, "_encode_pool", no_pool)
    monkeypatch.setenv("SSD_JPEG_ENCODE_GPU", "1")
    assert data_utils.jpeg_entropy_gpu_enabled() == (setting == "1")
    images = [_dev(fixture[n][0]) for n in NAMES]
    blobs = data_utils.encode_jpeg_batch(images, quality=[fixture[n][1] for n in NAMES], subsampling=[fixture[n][2] for n in NAMES])
    assert len(blobs) == len(NAMES)
    for n, b in zip(NAMES, blobs):
        assert isinstance(b, bytes) and b == fixture[n][3], n
    same = [n for n in NAMES if n.startswith("37x53_")]
    x = torch.stack([_dev(fixture[n][0]) for n in same])
    got = data_utils.encode_jpeg_batch(x, quality=[fixture[n][1] for n in same], subsampling=[fixture[n][2] for n in same])
    assert got == [fixture[n][3] for n in same]
    assert data_utils.encode_jpeg_batch([]) == []


def test_drawn_detections_are_the_same_files_under_both_settings(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    B, H, W, T = 3, 40, 56, 4
    imgs = np.stack([dc.image(H, W, seed=i) for i in range(B)])
    y1, x1 = rng.uniform(0, 0.6, (B, T)), rng.uniform(0, 0.6, (B, T))
    boxes = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.4, (B, T)), x1 + rng.uniform(0.1, 0.4, (B, T))], -1).astype(np.float32)
    drawn = du.draw_detections_batch(ssd_hip.to_dev(imgs), boxes, rng.integers(1, len(dc.LABELS), (B, T)),
                                     rng.uniform(0.3, 1.0, (B, T)).astype(np.float32), dc.LABELS, colors=dc.colors())
    monkeypatch.setenv("SSD_JPEG_ENCODE_GPU", "1")
    monkeypatch.setenv("SSD_JPEG_ENTROPY_GPU", "1")
    du._present(drawn, str(tmp_path / "gpu"), 5, False, out_format="jpeg", out_quality=90)
    monkeypatch.delenv("SSD_JPEG_ENTROPY_GPU")
    du._present(drawn, str(tmp_path / "host"), 5, False, out_format="jpeg", out_quality=90)
    names = ["img_%05d.jpg" % (5 + i) for i in range(B)]
    assert sorted(f.name for f in (tmp_path / "gpu").iterdir()) == names
    for n in names:
        a, b = (tmp_path / "gpu" / n).read_bytes(), (tmp_path / "host" / n).read_bytes()
        assert a == b and a[:2] == b"\xff\xd8" and a[-2:] == b"\xff\xd9", n


# ---- direct calls of the entry point, on buffers with guard bands

class _Batch(object):
    """One ``ssd_jpeg_pack`` call's arguments for hand-made int16 coefficients: the packed upload, the output and the
    workspace with GUARD bytes of FILL on both sides."""

    def __init__(self, shapes, subs, coef16, qualities=None):
        lib = ssd_hip.lib()
        self.B = len(shapes)
        self.shapes, self.subs = shapes, subs
        self.samplings = [jc.SAMPLING[s] for s in subs]
        self.tables = np.stack([jc.quality_tables(q) for q in (qualities or [75] * self.B)])
        self.enc = data_utils._jpeg_encode_layout(shapes, self.samplings)
        self.layout = data_utils._jpeg_pack_layout(self.enc["desc"], shapes, self.samplings, self.tables)
        self.desc = self.layout["desc"]
        host = np.zeros(self.layout["total"], np.uint8)
        data_utils._jpeg_pack_fill(host, self.layout)
        self.packed = _dev(host)
        self.coef_host = np.ascontiguousarray(coef16, np.int16).view(np.uint8)
        assert self.coef_host.size == self.enc["coef_bytes"]
        self.coef = _dev(self.coef_host)
        self.out_bytes = self.layout["out_bytes"]
        self.ws_bytes = int(lib.ssd_jpeg_pack_workspace_bytes(self.desc.ctypes.data, self.B))
        assert self.ws_bytes > 0
        self.meta = torch.full((2 * self.B + 1,), -7, dtype=torch.int32, device=ssd_hip.device())
        self.fresh(FILL)

    def fresh(self, out_fill):
        dev = ssd_hip.device()
        self.out = torch.full((self.out_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.out[GUARD:GUARD + self.out_bytes] = out_fill
        self.ws = torch.full((self.ws_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)

    def call(self, desc=None, B=None, out_bytes=None, out_shift=0):
        desc = self.desc if desc is None else desc
        return ssd_hip.lib().ssd_jpeg_pack(
            ssd_hip.ptr(self.coef), self.coef.numel(), ssd_hip.ptr(self.packed), self.packed.numel(), desc.ctypes.data,
            ssd_hip.ptr(self.packed), self.B if B is None else B, self.out.data_ptr() + GUARD + out_shift,
            self.out_bytes if out_bytes is None else out_bytes, self.meta.data_ptr(), self.meta.data_ptr() + 4 * (self.B + 1),
            self.ws.data_ptr() + GUARD, self.ws_bytes, ssd_hip.stream())

    def results(self):
        torch.cuda.synchronize()
        out, meta = self.out.cpu().numpy(), self.meta.cpu().numpy()
        return out[GUARD:GUARD + self.out_bytes], meta[:self.B + 1], meta[self.B + 1:]

    def guards_intact(self):
        torch.cuda.synchronize()
        out, ws = self.out.cpu().numpy(), self.ws.cpu().numpy()
        return bool((out[:GUARD] == FILL).all() and (out[GUARD + self.out_bytes:] == FILL).all()
                    and (ws[:GUARD] == FILL).all() and (ws[GUARD + self.ws_bytes:] == FILL).all())

    def host(self):
        return _host_streams(self.coef_host, self.enc["desc"], self.shapes, self.subs, self.tables)


def _small_coefficients(shapes, subs, seed):
    """Seeded int16 storage of a batch (values -3..3, a third of them nonzero) as ``_jpeg_encode_layout`` places it, and
    the per-image views."""
    rng = np.random.default_rng(seed)
    enc = data_utils._jpeg_encode_layout(shapes, [jc.SAMPLING[s] for s in subs])
    coef = np.zeros(enc["coef_bytes"] // 2, np.int16)
    views = []
    for d, (H, W), s in zip(enc["desc"], shapes, subs):
        g = jc.Geometry(H, W, *jc.SAMPLING[s])
        v = coef[int(d["coef_offset"]) // 2:int(d["coef_offset"]) // 2 + g.n]
        v[:] = rng.integers(-3, 4, g.n) * (rng.random(g.n) < 0.33)
        views.append((g, v))
    return coef, views


SHAPES3, SUBS3 = [(16, 24), (8, 16), (17, 15)], ["4:2:0", "4:4:4", "4:2:2"]


def test_out_of_range_coefficients_are_reported_and_contained(monkeypatch):
    coef, views = _small_coefficients(SHAPES3, SUBS3, 5)
    g1, v1 = views[1]
    g1.plane(v1, 0)[0, 1, 9] = 1024                                                # an AC term of category 11
    g2, v2 = views[2]
    g2.plane(v2, 1)[1, 0, 0] = g2.plane(v2, 1)[0, 0, 0] + 4096                     # a DC step of category 13
    batch = _Batch(SHAPES3, SUBS3, coef)
    want = batch.host()
    assert want[0] is not None and want[1] is None and want[2] is None            # the host coder refuses exactly these
    assert batch.call() == 0
    out, offsets, status = batch.results()
    assert batch.guards_intact()
    assert status[0] == 0 and status[1] != 0 and status[2] != 0
    assert offsets[0] == 0 and out[:offsets[1]].tobytes() == want[0]
    assert all(0 < offsets[b + 1] - offsets[b] <= ssd_hip.lib().ssd_jpeg_encode_bound(ctypes.byref(batch.layout["infos"][b]))
               for b in range(3))
    # the whole road raises what the host road raises for these coefficients
    monkeypatch.setattr(data_utils, "jpeg_forward_batch", lambda rgb, shapes, samplings, tables: (batch.coef, batch.enc["desc"]))
    monkeypatch.setenv("SSD_JPEG_ENCODE_GPU", "1")
    images = [torch.zeros((h, w, 3), dtype=torch.uint8, device=ssd_hip.device()) for h, w in SHAPES3]
    errors = []
    for setting in ("0", "1"):
        monkeypatch.setenv("SSD_JPEG_ENTROPY_GPU", setting)
        with pytest.raises(ValueError) as e:
            data_utils.encode_jpeg_batch(images, subsampling=SUBS3, workers=1)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "an AC coefficient of 1024" in errors[1]


def test_nothing_outside_the_buffers_is_written_and_two_calls_agree():
    shapes, subs = [(40, 56), (1, 1), (33, 100)], ["4:2:0", "4:2:2", "4:4:4"]
    coef, _ = _small_coefficients(shapes, subs, 6)
    batch = _Batch(shapes, subs, coef, qualities=[30, 75, 95])
    want = batch.host()
    assert batch.call() == 0
    first, offsets, status = batch.results()
    assert batch.guards_intact() and not status.any()
    n = int(offsets[3])
    assert [first[offsets[b]:offsets[b + 1]].tobytes() for b in range(3)] == want
    batch.fresh(0xFF)                                                              # another output, pre-filled with 0xFF
    assert batch.call() == 0
    second, offsets2, status2 = batch.results()
    assert batch.guards_intact() and not status2.any()
    assert offsets2.tolist() == offsets.tolist() and second[:n].tobytes() == first[:n].tobytes()


def test_refusals_launch_nothing_and_an_empty_batch_is_a_no_op():
    lib = ssd_hip.lib()
    assert lib.ssd_jpeg_pack(None, 0, None, 0, None, None, 0, None, 0, None, None, None, 0, ssd_hip.stream()) == 0
    coef, _ = _small_coefficients(SHAPES3, SUBS3, 7)
    batch = _Batch(SHAPES3, SUBS3, coef)

    def edited(b, **fields):
        d = batch.desc.copy()
        for k, v in fields.items():
            d[b][k] = v
        return d

    assert batch.call(B=0) == 0
    assert batch.call(out_bytes=batch.out_bytes - 1) == -1
    assert lib.ssd_last_error().decode().startswith("ssd_jpeg_pack")
    assert batch.call(out_shift=8, out_bytes=batch.out_bytes) == -1                # a misaligned pointer
    assert batch.call(desc=edited(1, block_start=int(batch.desc[1]["block_start"]) + 1)) == -1
    assert batch.call(desc=edited(2, coef_offset=int(batch.desc[1]["coef_offset"]))) == -1
    assert batch.call(desc=edited(0, header_offset=batch.layout["total"])) == -1
    assert batch.call(desc=edited(0, h_samp=4, v_samp=1)) == -3                    # sampling 4x1
    assert batch.call(desc=edited(1, W=16385)) == -3
    assert batch.call(B=70000) == -3
    out, offsets, status = batch.results()
    assert bool((out == FILL).all()) and bool((offsets == -7).all()) and bool((status == -7).all())
    assert bool((batch.ws.cpu().numpy() == FILL).all())
    assert batch.call() == 0                                                       # and the same arguments, unedited, run
    out, offsets, status = batch.results()
    assert [out[offsets[b]:offsets[b + 1]].tobytes() for b in range(3)] == batch.host() and not status.any()
