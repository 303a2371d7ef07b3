"""Shared by the device entropy decoder's tests (tests/test_jpeg_unpack_cpu.py, tests/test_jpeg_unpack_gpu.py), its
sanitizer check (tests/micro/jpeg_unpack_host_check.sh) and tests/bench_jpeg_unpack.py: the real-size streams, the
malformed set, an independent walk over a scan's markers, and the ctypes calls of ``ssd_jpeg_scan_plan`` and
``ssd_jpeg_entropy_decode_subseq``.  Content, ``encode`` and the fixture come from tests/jpeg_cases.py."""
import ctypes

import numpy as np

import jpeg_cases as jc

OK, INVALID, UNSUPPORTED = 0, -1, -3
RESTART_CASES = {"restart1_420": 10, "restart3_444": 10, "restart3_L": 5}         # segments; the last is ceil(15 / 3)


def real_streams():
    """{name: JPEG bytes}: the four streams large enough for many 256-subsequence chunks at 128 bits."""
    h, w = jc.REAL_SIZE
    real = jc.content(h, w, "420", "smooth", 5)
    return {
        "real_size": jc.real_size_blob(),
        "noise_444_q100": jc.encode(jc.content(200, 200, "444", "noise"), "444", {"quality": 100}),      # heavy stuffing, long codes
        "restart_rows": jc.encode(real, "420", {"quality": 92, "restart_marker_rows": 1}),
        "optimize": jc.encode(real, "420", {"quality": 92, "optimize": True}),
    }


def scan_data_at(blob):
    """Index of the first entropy-coded byte (after the first SOS header)."""
    scan = blob.index(b"\xff\xda")
    return scan + 2 + ((blob[scan + 2] << 8) | blob[scan + 3])


def _mid(blob, marker):
    at = blob.index(marker)
    return at + 4 + (((blob[at + 2] << 8) | blob[at + 3]) - 2) // 2


def malformed(blob):
    """[(name, bytes)] from one sound stream: the 64 single-byte ``^= 0xFF`` flips of
    test_jpeg_cpu.py::test_truncated_and_damaged_files_never_crash_or_write_outside (same seed), six truncations, and the
    scan data replaced by seeded random bytes (as they are, and with every 0xFF stuffed so that decoding goes deep)."""
    n, scan_data = len(blob), scan_data_at(blob)
    out = []
    rng = np.random.default_rng(7)
    for pos in rng.choice(np.arange(scan_data, n - 2), 64, replace=False):
        b = bytearray(blob)
        b[int(pos)] ^= 0xFF
        out.append(("flip_%d" % pos, bytes(b)))
    for cut in (0, 2, 20, _mid(blob, b"\xff\xc4"), (scan_data + n) // 2, n - 2):
        out.append(("cut_%d" % cut, blob[:cut]))
    noise = np.random.default_rng(11).integers(0, 256, n - 2 - scan_data, dtype=np.uint8).tobytes()
    out.append(("random", blob[:scan_data] + noise + b"\xff\xd9"))
    out.append(("random_stuffed", blob[:scan_data] + noise.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"))
    return out


def walk_segments(blob, info):
    """The scan's segments by an independent walk over the bytes: ``(data_begin, data_end, [(first_byte, bytes, first_mcu)])``
    or None where a restart marker is wrong or missing.  A segment ends at the first 0xFF not followed by 0x00."""
    at = begin = scan_data_at(blob)
    mcus = info.mcus_x * info.mcus_y
    ri = info.restart_interval
    count = -(-mcus // ri) if ri else 1
    segs = []
    for k in range(count):
        end = at
        while end < len(blob) and not (blob[end] == 0xFF and blob[end + 1:end + 2] != b"\x00"):
            end += 2 if blob[end] == 0xFF else 1
        end = min(end, len(blob))
        segs.append((at - begin, end - at, k * ri))
        at = end
        if k + 1 < count:
            fills = 0
            while at + fills < len(blob) and blob[at + fills] == 0xFF:
                fills += 1
            if fills == 0 or at + fills >= len(blob) or blob[at + fills] != 0xD0 + (k & 7):
                return None
            at += fills + 1
    return begin, at, segs


def segment_count(info):
    mcus = info.mcus_x * info.mcus_y
    return -(-mcus // info.restart_interval) if info.restart_interval else 1


def _buffer(blob):
    return (ctypes.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob.ljust(1, b"\0"))


def scan_plan(blob, info, capacity=None):
    """``(return code, JpegScanPlan, segments as a JPEG_SEGMENT_DTYPE array)`` of ``ssd_jpeg_scan_plan``."""
    import ssd_hip
    plan = ssd_hip.JpegScanPlan()
    segs = np.zeros(segment_count(info) if capacity is None else capacity, ssd_hip.JPEG_SEGMENT_DTYPE)
    buf = _buffer(blob)
    rc = ssd_hip.lib().ssd_jpeg_scan_plan(ctypes.addressof(buf), len(blob), ctypes.byref(info), ctypes.byref(plan),
                                          segs.ctypes.data, len(segs))
    return rc, plan, segs


def subseq_decode(blob, info, subseq_bits, guard=64, fill=0x5A5A):
    """``jpeg_cases.entropy_decode`` for ``ssd_jpeg_entropy_decode_subseq``: ``(return code, coefficients, guards intact)``."""
    import ssd_hip
    n = int(info.coef_bytes) // 2
    store = np.full(n + 2 * guard, fill, np.int16)
    buf = _buffer(blob)
    rc = ssd_hip.lib().ssd_jpeg_entropy_decode_subseq(ctypes.addressof(buf), len(blob), ctypes.byref(info),
                                                     store.ctypes.data + 2 * guard, n * 2, subseq_bits)
    intact = bool((store[:guard] == fill).all() and (store[n + guard:] == fill).all())
    return rc, store[guard:n + guard].copy(), intact
