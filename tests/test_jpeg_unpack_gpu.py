"""The device entropy decoder (``ssd_jpeg_unpack``; ``data_utils.jpeg_unpack_batch``; the JPEG road with
``SSD_JPEG_ENTROPY_DECODE_GPU=1``) against the host decoder ``ssd_jpeg_entropy_decode`` -- itself held to Pillow by
tests/test_jpeg_cpu.py -- bit for bit, and the whole road against the default road's pixels.  The malformed inputs are
those of tests/test_jpeg_unpack_cpu.py, which the host model has decoded under sanitizers
(tests/micro/jpeg_unpack_host_check.sh): here they test the status contract."""
import io

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_unpack_cases as uc
import ssd_hip
import voc_cases as vc
from utils import data_utils

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in jc.cases()]
GUARD, FILL = 64, 0xA5


def _host(blob, info=None):
    """``(info, host return code, host coefficients)``; ``info``: the sound stream's, for a damaged one."""
    if info is None:
        rc, info, err = jc.parse(blob)
        assert rc == 0, err
    rc, coef, intact = jc.entropy_decode(blob, info)
    assert intact
    return info, rc, coef


@pytest.fixture(scope="module")
def fixture():
    """{name: (blob, info, host coefficients)}, decoded once."""
    out = {}
    for name, (blob, _) in jc.load_fixture()[0].items():
        info, rc, coef = _host(blob)
        assert rc == 0
        out[name] = (blob, info, coef)
    return out


@pytest.fixture(scope="module")
def real():
    out = {}
    for name, blob in uc.real_streams().items():
        info, rc, coef = _host(blob)
        assert rc == 0
        out[name] = (blob, info, coef)
    return out


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(ssd_hip.device())


class _Batch(object):
    """One ``ssd_jpeg_unpack`` call's arguments: the packed upload, and a coefficient destination pre-filled with FILL in
    which GUARD bytes lie before, between and after the images' regions; the workspace between guards too."""

    def __init__(self, streams, bits):
        self.scans = []
        for blob, info in streams:
            scan = data_utils._jpeg_plan(blob, info)
            assert scan is not None
            self.scans.append(scan)
        self.B, self.bits = len(self.scans), bits
        self.layout = data_utils._jpeg_unpack_layout(self.scans, bits)
        self.desc = self.layout["desc"]
        at = GUARD
        self.regions = []
        for d, s in zip(self.desc, self.scans):
            d["coef_offset"] = at
            self.regions.append((at, int(s.info.coef_bytes)))
            at += (int(s.info.coef_bytes) + 15) // 16 * 16 + GUARD
        self.coef_bytes = at
        host = np.zeros(self.layout["total"], np.uint8)
        data_utils._jpeg_unpack_fill(host, self.scans, self.layout)
        self.packed = _dev(host)
        self.ws_bytes = int(ssd_hip.lib().ssd_jpeg_unpack_workspace_bytes(self.desc.ctypes.data, self.B, bits))
        assert self.ws_bytes > 0
        dev = ssd_hip.device()
        self.coef = torch.full((self.coef_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.ws = torch.full((self.ws_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.status = torch.full((self.B,), -7, dtype=torch.int32, device=dev)

    def call(self, desc=None, B=None, bits=None, coef_shift=0, coef_bytes=None, ws_bytes=None, coef_ptr=None):
        desc = self.desc if desc is None else desc
        base = self.packed.data_ptr()
        return ssd_hip.lib().ssd_jpeg_unpack(
            base, self.packed.numel(), desc.ctypes.data, base + self.layout["desc_at"], self.B if B is None else B,
            self.bits if bits is None else bits, self.coef.data_ptr() + GUARD + coef_shift if coef_ptr is None else coef_ptr,
            self.coef_bytes if coef_bytes is None else coef_bytes, self.status.data_ptr(), self.ws.data_ptr() + GUARD,
            self.ws_bytes if ws_bytes is None else ws_bytes, ssd_hip.stream())

    def results(self):
        """(per image int16 coefficients, status, sweeps, every guard intact)"""
        torch.cuda.synchronize()
        coef, ws = self.coef.cpu().numpy(), self.ws.cpu().numpy()
        inner = coef[GUARD:GUARD + self.coef_bytes]
        images, mask = [], np.ones(inner.size, bool)
        for at, n in self.regions:
            images.append(inner[at:at + n].view(np.int16))
            mask[at:at + n] = False
        intact = bool((inner[mask] == FILL).all() and (coef[:GUARD] == FILL).all() and (coef[GUARD + self.coef_bytes:] == FILL).all()
                      and (ws[:GUARD] == FILL).all() and (ws[GUARD + self.ws_bytes:] == FILL).all())
        sweeps = ws[GUARD:GUARD + 4 * self.B].view(np.int32)
        return images, self.status.cpu().numpy(), sweeps, intact


@pytest.mark.parametrize("bits", [128, 0])
def test_every_fixture_case_in_one_ragged_call_equals_the_host_decoder(fixture, bits):
    batch = _Batch([fixture[n][:2] for n in NAMES], bits)
    assert batch.B == 66 and batch.call() == 0
    images, status, sweeps, intact = batch.results()
    assert intact and not status.any(), status
    for n, got in zip(NAMES, images):
        assert np.array_equal(got, fixture[n][2]), (n, int((got != fixture[n][2]).sum()))
    assert (sweeps >= 1).all() and (sweeps <= 256).all()
    if bits == 128:
        assert sweeps.max() >= 3                                                  # several subsequences inside the small streams


@pytest.mark.parametrize("bits", [128, 0])
def test_real_size_streams_equal_the_host_decoder(real, bits):
    names = list(real)
    batch = _Batch([real[n][:2] for n in names], bits)
    assert batch.call() == 0
    images, status, sweeps, intact = batch.results()
    assert intact and not status.any(), status
    for n, got in zip(names, images):
        assert np.array_equal(got, real[n][2]), (n, bits, int((got != real[n][2]).sum()))
    print("sweeps at %d bits: %s" % (bits or ssd_hip.JPEG_UNPACK_SUBSEQ_BITS, dict(zip(names, sweeps.tolist()))))
    assert (sweeps >= 2).all() and (sweeps <= 256).all()


def test_sound_and_malformed_streams_in_one_batch_keep_the_status_contract(fixture, real):
    picked = []
    for base, info in (fixture["size_17x33_420"][:2], real["real_size"][:2]):
        accepted, refused = [], []
        for name, blob in uc.malformed(base):
            if jc.parse(blob)[0] != 0 or data_utils._jpeg_plan(blob, info) is None:
                continue                                                          # never reaches the device: the plan refuses it
            _, rc, coef = _host(blob, info)
            (accepted if rc == 0 else refused).append((blob, info, rc, coef))
        assert len(refused) >= 2
        picked += accepted[:2] + refused[:4 - min(len(accepted), 2)]
    assert len(picked) == 8 and sum(p[2] == 0 for p in picked) >= 1 and sum(p[2] != 0 for p in picked) >= 4
    sound = [(b, i, 0, c) for b, i, c in (fixture["q92_noise_444"], fixture["restart3_444"], real["optimize"])]
    streams = [sound[0]] + picked[:4] + [sound[1]] + picked[4:] + [sound[2]]
    batch = _Batch([s[:2] for s in streams], 128)
    assert batch.call() == 0
    images, status, _, intact = batch.results()
    assert intact
    flagged = 0
    for b, (blob, info, rc, want) in enumerate(streams):
        if status[b] == 0:                                                        # unflagged: the host decoder takes it, to the same bits
            assert rc == 0 and np.array_equal(images[b], want), b
        if rc != 0:                                                               # the host decoder refuses: flagged
            assert status[b] != 0, b
        flagged += status[b] != 0
    assert flagged >= 4 and all(status[b] == 0 for b in (0, 5, 10))               # the sound neighbours are exact (checked above)


def _pixels(jb):
    torch.cuda.synchronize()
    return [im.cpu().numpy() for im in jb.images]


def test_decode_jpeg_batch_with_the_switch_on_gives_the_default_roads_pixels(fixture, real, monkeypatch):
    from PIL import Image
    rgb = jc.content(24, 40, "444", "smooth")
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "PNG")
    raw = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"), dtype=np.uint8)
    blobs = [fixture[n][0] for n in NAMES] + [real["real_size"][0], raw]
    monkeypatch.delenv("SSD_JPEG_ENTROPY_DECODE_GPU", raising=False)
    assert not data_utils.jpeg_entropy_decode_gpu_enabled()
    want = _pixels(data_utils.decode_jpeg_batch(blobs))
    calls = []
    real_launch = data_utils._jpeg_unpack_launch
    monkeypatch.setattr(data_utils, "_jpeg_unpack_launch", lambda *a, **k: calls.append(len(a[1]["desc"])) or real_launch(*a, **k))
    monkeypatch.setenv("SSD_JPEG_ENTROPY_DECODE_GPU", "0")
    assert not data_utils.jpeg_entropy_decode_gpu_enabled()
    monkeypatch.setenv("SSD_JPEG_ENTROPY_DECODE_GPU", "1")
    assert data_utils.jpeg_entropy_decode_gpu_enabled()
    monkeypatch.setattr(data_utils, "_jpeg_entropy_into", lambda *a: pytest.fail("the host entropy decoder ran"))
    jb = data_utils.decode_jpeg_batch(blobs)
    got = _pixels(jb)
    assert calls == [67] and jb.kinds == [ssd_hip.JPEG_COEFFICIENTS] * 67 + [ssd_hip.JPEG_RAW]
    assert len(got) == len(want) == 68
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), b
    assert np.array_equal(got[-1], raw)


def test_a_damaged_file_in_the_batch_yields_what_the_default_road_yields(fixture, real, monkeypatch):
    base = real["real_size"][0]
    damaged = None
    for name, blob in uc.malformed(base):                                         # a flip the plan takes and the host decoder refuses
        if name.startswith("flip") and data_utils._jpeg_plan(blob, real["real_size"][1]) is not None \
                and _host(blob, real["real_size"][1])[1] != 0:
            damaged = blob
            break
    assert damaged is not None
    blobs = [fixture["size_17x33_420"][0], damaged, fixture["restart1_420"][0]]
    seen = []

    def fallback(blob):
        seen.append(len(blob))
        return np.full((5, 7, 3), 9, np.uint8)
    monkeypatch.delenv("SSD_JPEG_ENTROPY_DECODE_GPU", raising=False)
    want = _pixels(data_utils.decode_jpeg_batch(blobs, fallback=fallback))
    monkeypatch.setenv("SSD_JPEG_ENTROPY_DECODE_GPU", "1")
    got = _pixels(data_utils.decode_jpeg_batch(blobs, fallback=fallback))
    assert seen == [len(damaged)] * 2                                             # Pillow's business on both roads, once each
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert got[1].shape == (5, 7, 3)


@pytest.fixture(scope="module")
def devkit(tmp_path_factory):
    root = tmp_path_factory.mktemp("voc_jpeg_unpack")
    vc.write_devkit(root)
    return root


@pytest.mark.parametrize("workers", [1, 4])
def test_voc_batches_with_the_switch_on_yield_the_same_bits(devkit, workers, monkeypatch):
    a, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    b, _ = data_utils.get_dataset("voc/2007", "test", str(devkit))
    ds = a.concatenate(b)

    def run():
        out = [(x.cpu().numpy(), gt, gl) for x, gt, gl in data_utils.voc_batches(ds, 4, 300, 300, workers=workers)]
        torch.cuda.synchronize()
        return out
    monkeypatch.delenv("SSD_JPEG_ENTROPY_DECODE_GPU", raising=False)
    ref = run()
    calls = []
    real_launch = data_utils._jpeg_unpack_launch
    monkeypatch.setattr(data_utils, "_jpeg_unpack_launch", lambda *a, **k: calls.append(len(a[1]["desc"])) or real_launch(*a, **k))
    monkeypatch.setenv("SSD_JPEG_ENTROPY_DECODE_GPU", "1")
    got = run()
    assert calls == [4, 4, 2]                                                     # the new road was taken
    assert len(got) == len(ref) == 3
    for (x, gt, gl), (rx, rgt, rgl) in zip(got, ref):
        assert np.array_equal(x, rx) and np.array_equal(gt, rgt) and np.array_equal(gl, rgl)


def test_jpeg_unpack_batch_is_the_bare_call(fixture):
    names = ["size_33x17_422", "restart3_L", "q100_noise_420"]
    coef, desc, status, sweeps = data_utils.jpeg_unpack_batch([fixture[n][0] for n in names], subseq_bits=256)
    assert coef.dtype == torch.uint8 and status.dtype == torch.int32 and sweeps.dtype == torch.int32
    assert tuple(status.shape) == (3,) and not status.cpu().numpy().any() and (sweeps.cpu().numpy() >= 1).all()
    host = coef.cpu().numpy()
    for d, n in zip(desc, names):
        at = int(d["coef_offset"])
        assert np.array_equal(host[at:at + fixture[n][2].nbytes].view(np.int16), fixture[n][2]), n
    with pytest.raises(ValueError):
        data_utils.jpeg_unpack_batch([b"not a jpeg"])
    assert data_utils.jpeg_unpack_batch([])[0].numel() == 0


def test_refusals_launch_nothing_and_an_empty_batch_is_a_no_op(fixture):
    lib = ssd_hip.lib()
    assert lib.ssd_jpeg_unpack(None, 0, None, None, 0, 0, None, 0, None, None, 0, ssd_hip.stream()) == 0
    names = ["size_17x33_420", "restart1_420", "size_40x24_L"]
    batch = _Batch([fixture[n][:2] for n in names], 128)

    def edited(b, **fields):
        d = batch.desc.copy()
        for k, v in fields.items():
            d[b][k] = v
        return d

    assert batch.call(B=0) == 0
    assert batch.call(ws_bytes=batch.ws_bytes - 16) == -1
    assert lib.ssd_last_error().decode().startswith("ssd_jpeg_unpack")
    assert batch.call(coef_shift=8) == -1                                          # a misaligned pointer
    assert batch.call(coef_bytes=batch.coef_bytes - GUARD - 16) == -1              # the last region ends outside
    assert batch.call(coef_ptr=batch.packed.data_ptr() + 16, coef_bytes=batch.packed.numel() - 16) == -1   # overlaps packed_dev
    assert batch.call(desc=edited(1, block_start=int(batch.desc[1]["block_start"]) + 1)) == -1
    assert batch.call(desc=edited(2, sub_start=int(batch.desc[2]["sub_start"]) + 256)) == -1
    assert batch.call(desc=edited(2, seg_start=int(batch.desc[2]["seg_start"]) + 1)) == -1
    assert batch.call(desc=edited(2, coef_offset=int(batch.desc[1]["coef_offset"]))) == -1     # overlapping regions
    assert batch.call(desc=edited(0, coef_offset=int(batch.desc[0]["coef_offset"]) + 8)) == -1
    assert batch.call(desc=edited(0, scan_offset=batch.layout["total"])) == -1
    assert batch.call(desc=edited(0, huff_offset=batch.layout["total"] - 16)) == -1
    assert batch.call(desc=edited(1, segments=9)) == -1                            # the frame has ten
    assert batch.call(desc=edited(1, scan_bytes=-1)) == -1
    for bits in (64, 96, 130, 1 << 20):
        assert batch.call(bits=bits) == -3, bits
    assert batch.call(desc=edited(0, h_samp=4, v_samp=1)) == -3                    # sampling 4x1
    assert batch.call(desc=edited(2, components=2)) == -3
    assert batch.call(desc=edited(1, W=16385)) == -3
    assert batch.call(desc=edited(1, scan_bytes=1 << 28)) == -3
    assert batch.call(B=70000) == -3
    torch.cuda.synchronize()
    assert bool((batch.coef.cpu().numpy() == FILL).all()) and bool((batch.ws.cpu().numpy() == FILL).all())
    assert bool((batch.status.cpu().numpy() == -7).all())
    assert batch.call() == 0                                                       # and the same arguments, unedited, run
    images, status, _, intact = batch.results()
    assert intact and not status.any()
    assert all(np.array_equal(got, fixture[n][2]) for n, got in zip(names, images))
