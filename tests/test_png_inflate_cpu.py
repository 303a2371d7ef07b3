"""The host model of the device inflater, without a GPU: ``ssd_png_inflate_host`` gives zlib's bytes and status 0 on every
accepted case of ``png_inflate_cases`` and the documented status bit on every refusal case, writes nothing outside its
output, and is callable from several threads.  The case set itself is checked first: it covers what its docstring names,
and the host road's rule (``data_utils._png_inflate``) accepts and refuses the same streams."""
import ctypes
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import png_inflate_cases as ic
import ssd_hip
from utils import data_utils

ACCEPTED = ic.all_accepted()
REFUSED = ic.refusal_cases()
GUARD = 64


def host_inflate(stream, H, rb):
    """``(bytes, status)`` of ``ssd_png_inflate_host``; asserts the guard bytes around the output."""
    n = H * (1 + rb)
    store = np.full(n + 2 * GUARD, 0xA5, np.uint8)
    status = ctypes.c_int(-1)
    rc = ssd_hip.lib().ssd_png_inflate_host(stream, len(stream), store.ctypes.data + GUARD, n, rb, ctypes.byref(status))
    assert rc == 0, ssd_hip.lib().ssd_last_error().decode()
    assert (store[:GUARD] == 0xA5).all() and (store[GUARD + n:] == 0xA5).all()
    return store[GUARD:GUARD + n].tobytes(), status.value


def _host_road(stream, H, rb):
    blob = ic.as_png(stream, H, rb)
    info = data_utils._png_parse(blob)
    assert info is not None and (info.height, info.row_bytes) == (H, rb)
    return data_utils._png_inflate(blob, info)


def test_the_case_set_covers_what_it_names():
    ic.coverage()
    assert len({bit for _, _, _, _, bit in REFUSED}) == len(ssd_hip.PNG_INFLATE_STATUS)    # every cause has a case


def test_the_host_road_accepts_and_refuses_the_same_streams():
    for name, stream, H, rb in ACCEPTED:
        assert ic.zlib_accepts(stream, H, rb), name
        got = _host_road(stream, H, rb)
        assert got is not None and got.tobytes() == zlib.decompress(stream), name
    for name, stream, H, rb, _ in REFUSED:
        assert not ic.zlib_accepts(stream, H, rb), name
        assert _host_road(stream, H, rb) is None, name


@pytest.mark.parametrize("case", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_accepted_streams_give_zlibs_bytes_and_status_0(case):
    name, stream, H, rb = case
    data, status = host_inflate(stream, H, rb)
    assert status == 0
    assert data == zlib.decompress(stream)


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_streams_give_the_documented_bit(case):
    name, stream, H, rb, bit = case
    _, status = host_inflate(stream, H, rb)
    assert status == ssd_hip.PNG_INFLATE_STATUS[bit]


def test_truncations_and_corruptions_are_never_accepted_wrongly():
    """Status 0 implies zlib's verdict and zlib's bytes, whatever the input: every truncation and a sweep of single-byte
    corruptions of four small streams (guard bytes checked on every call)."""
    picked = [c for c in ACCEPTED if c[0] in ("one_pixel", "no_distance_code", "length_3_and_258_at_distance_1", "smooth_level1")]
    assert len(picked) == 4
    for name, stream, H, rb in picked:
        variants = [stream[:k] for k in range(len(stream))]
        for k in range(len(stream)):
            for flip in (0x01, 0x80, 0xFF):
                variants.append(stream[:k] + bytes([stream[k] ^ flip]) + stream[k + 1:])
        for v in variants:
            data, status = host_inflate(v, H, rb)
            if status == 0:                                                         # an Adler-32 can collide: zlib's verdict and bytes, not the original's
                assert ic.zlib_accepts(v, H, rb) and data == zlib.decompressobj().decompress(v, H * (1 + rb) + 1), (name, v.hex())


def test_bad_arguments_are_refused():
    lib = ssd_hip.lib()
    name, stream, H, rb = ACCEPTED[0]
    out = np.zeros(H * (1 + rb), np.uint8)
    status = ctypes.c_int(0)
    assert lib.ssd_png_inflate_host(None, len(stream), out.ctypes.data, out.nbytes, rb, ctypes.byref(status)) == -1
    assert lib.ssd_png_inflate_host(stream, len(stream), None, out.nbytes, rb, ctypes.byref(status)) == -1
    assert lib.ssd_png_inflate_host(stream, len(stream), out.ctypes.data, out.nbytes, rb, None) == -1
    assert lib.ssd_png_inflate_host(stream, len(stream), out.ctypes.data, out.nbytes - 1, rb, ctypes.byref(status)) == -1
    assert lib.ssd_png_inflate_host(stream, len(stream), out.ctypes.data, 0, rb, ctypes.byref(status)) == -1
    assert lib.ssd_png_inflate_host(stream, len(stream), out.ctypes.data, out.nbytes, 0, ctypes.byref(status)) == -1


def test_callable_from_several_threads():
    work = [c[:4] for c in ACCEPTED] + [c[:4] for c in REFUSED]
    want = [host_inflate(*c[1:]) for c in work]
    with ThreadPoolExecutor(8) as pool:
        for _ in range(3):
            assert list(pool.map(lambda c: host_inflate(*c[1:]), work)) == want


def test_the_binding_matches_the_header():
    assert ssd_hip.PNG_INFLATE_DESC_DTYPE.itemsize == 48
    assert ssd_hip.PNG_INFLATE_DESC_DTYPE.names == ("zlib_offset", "zlib_bytes", "dst_offset", "chain_offset", "row_bytes", "H", "reserved")
    bits = sorted(ssd_hip.PNG_INFLATE_STATUS.values())
    assert bits == [1 << k for k in range(15)]
