"""The host half of the JPEG encoder (``ssd_jpeg_quality_tables`` / ``ssd_jpeg_encode_info`` / ``ssd_jpeg_encode_bound`` /
``ssd_jpeg_entropy_encode``: no GPU needed) and the arithmetic the device half must reproduce: the NumPy restatement of
tests/jpeg_encode_cases.py equals the bytes Pillow wrote for every fixture case.  No tolerance anywhere: every comparison
is equality."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_cases as jd
import jpeg_encode_cases as jc

OK, INVALID, UNSUPPORTED = 0, -1, -3
NAMES = [c[0] for c in jc.cases()]


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


@pytest.fixture(scope="module")
def restated(fixture):
    """{name: (Geometry, coefficient storage, tables)} of the restatement, computed once."""
    out = {}
    for name, (rgb, q, s, _) in fixture.items():
        tables = jc.quality_tables(q)
        out[name] = jc.forward(rgb, s, tables) + (tables,)
    return out


def _encode(rgb, q, s, coef):
    tables = jc.lib_quality_tables(q)
    rc, info = jc.lib_info(rgb.shape[0], rgb.shape[1], s, tables)
    assert rc == OK
    rc, blob, intact = jc.lib_entropy_encode(coef, info)
    assert rc == OK and intact
    return info, blob


def test_fixture_was_written_by_libjpeg_turbo():
    _, versions = jc.load_fixture()
    assert versions.startswith("Pillow ") and "libjpeg-turbo" in versions
    assert len(NAMES) == len(set(NAMES)) >= 60
    kept = set((q, s) for _, _, q, s in jc.cases())
    assert kept == set((q, s) for q in jc.QUALITIES for s in jc.SUBSAMPLINGS)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow(fixture, restated, name):
    rgb, q, s, blob = fixture[name]
    g, coef, tables = restated[name]
    assert jc.entropy_encode(g, coef, tables) == blob
    if jc.pillow_is_turbo():                            # a Pillow on another libjpeg may round differently: fixture only
        assert jc.pillow_encode(rgb, q, s) == blob


def test_the_fixture_reaches_every_mechanism(fixture, restated):
    """ZRL symbols, stuffed 0xFF bytes, dummy blocks to the right, below and in the corner, a category-11 DC difference."""
    total = {}
    for name in NAMES:
        g, coef, tables = restated[name]
        stats = {}
        jc.entropy_encode(g, coef, tables, stats)
        for k, v in stats.items():
            total[k] = max(total.get(k, 0), v)
    assert all(total[k] >= 1 for k in ("zrl", "stuffed", "dummy_right", "dummy_bottom", "dummy_corner")), total
    assert total["max_dc_category"] == 11
    stats = {}
    g, coef, tables = restated[jc.DC11]
    jc.entropy_encode(g, coef, tables, stats)
    assert stats["max_dc_category"] == 11


def test_vertical_edge_replicates_the_downsampled_row(fixture):
    """The first trap: padding the input rows to the MCU height before downsampling gives other chroma when H is not a
    multiple of 8 * v_samp, and Pillow's bytes follow the other reading."""
    name = next(n for n in NAMES if n.startswith("64x48_") and n.endswith("_420"))          # 64 rows: 4 MCU rows, no padding
    rgb, q, s, _ = fixture[name]
    part = rgb[:18]                                     # 18 rows: one whole row group below row 16, 14 rows of padding
    tables = jc.quality_tables(q)
    g, coef = jc.forward(part, s, tables)
    _, wrong = jc.forward(part, s, tables, pad_input_rows_first=True)
    assert not np.array_equal(g.real(coef), g.real(wrong))
    if jc.pillow_is_turbo():
        assert jc.entropy_encode(g, coef, tables) == jc.pillow_encode(part, q, s)


@pytest.mark.parametrize("quality", jc.QUALITIES + [0, 49, 50, 101])
def test_quality_tables(fixture, quality):
    got = jc.lib_quality_tables(quality)
    assert got.dtype == np.uint16 and np.array_equal(got, jc.quality_tables(quality))
    for name in NAMES:                                  # the DQT segments Pillow wrote at this quality
        _, q, _, blob = fixture[name]
        if q == quality:
            at = blob.index(b"\xff\xdb")
            for t in range(2):
                seg = blob[at + 69 * t:at + 69 * (t + 1)]
                assert seg[:5] == b"\xff\xdb\x00\x43" + bytes([t])
                assert np.array_equal(np.frombuffer(seg[5:], np.uint8), got[t][jc.ZIGZAG])


@pytest.mark.parametrize("name", NAMES)
def test_entropy_encode_equals_pillow_and_round_trips(fixture, restated, name):
    rgb, q, s, blob = fixture[name]
    g, coef, _ = restated[name]
    info, got = _encode(rgb, q, s, coef)
    assert got == blob
    # the decoder's host half reads the stream back: the same info, the same real blocks
    rc, parsed, err = jd.parse(got)
    assert rc == OK, err
    assert bytes(parsed) == bytes(info)
    rc, back, intact = jd.entropy_decode(got, parsed)
    assert rc == OK and intact
    assert np.array_equal(g.real(back), g.real(coef))


def test_padding_blocks_are_never_read(fixture, restated):
    """The second trap: the dummy blocks of the last MCU column and row are synthesised, not read from storage."""
    for name in NAMES:
        rgb, q, s, blob = fixture[name]
        g, coef, _ = restated[name]
        if all(g.rw[c] == g.bw[c] and g.rh[c] == g.bh[c] for c in range(3)):
            continue
        junk = np.full_like(coef, 12345)
        for c in range(3):
            g.plane(junk, c)[:g.rh[c], :g.rw[c]] = g.plane(coef, c)[:g.rh[c], :g.rw[c]]
        assert _encode(rgb, q, s, junk)[1] == blob, name


def test_bound_buffer_size_and_info_are_checked(fixture, restated):
    import ssd_hip
    lib = ssd_hip.lib()
    name = next(n for n in NAMES if n.startswith("37x53_noise"))
    rgb, q, s, blob = fixture[name]
    g, coef, tables = restated[name]
    rc, info = jc.lib_info(rgb.shape[0], rgb.shape[1], s, tables)
    assert rc == OK and info.coef_bytes == coef.nbytes
    assert lib.ssd_jpeg_encode_bound(ctypes.byref(info)) >= len(blob)
    rc, got, intact = jc.lib_entropy_encode(coef, info, out_bytes=len(blob))       # exactly enough
    assert rc == OK and intact and got == blob
    for n in (len(blob) - 1, len(blob) // 2, 700, 10, 0):                          # too small: mid-scan, mid-header, empty
        rc, _, intact = jc.lib_entropy_encode(coef, info, out_bytes=n)
        assert rc == INVALID and intact, n
        assert lib.ssd_last_error().decode().startswith("ssd_jpeg_entropy_encode")
    for field, value in (("mcus_x", info.mcus_x + 1), ("coef_bytes", info.coef_bytes - 128), ("components", 1),
                         ("restart_interval", 4), ("width", 0), ("height", 20000)):
        bad = ssd_hip.JpegInfo.from_buffer_copy(info)
        setattr(bad, field, value)
        rc, _, intact = jc.lib_entropy_encode(coef, bad, out_bytes=1 << 16)
        assert rc == INVALID and intact, field
        assert lib.ssd_jpeg_encode_bound(ctypes.byref(bad)) == 0
    bad = ssd_hip.JpegInfo.from_buffer_copy(info)
    bad.h_samp[0] = 4
    assert jc.lib_entropy_encode(coef, bad, out_bytes=1 << 16)[0] == INVALID
    bad = ssd_hip.JpegInfo.from_buffer_copy(info)
    bad.quant[2][5] += 1                                                             # Cb and Cr share one table
    assert jc.lib_entropy_encode(coef, bad, out_bytes=1 << 16)[0] == INVALID
    assert jc.lib_info(8, 8, "4:2:0", np.zeros((2, 64), np.uint16))[0] == INVALID   # a table entry of 0
    assert jc.lib_info(8, 16385, "4:2:0", tables)[0] == UNSUPPORTED
    info2 = ssd_hip.JpegInfo()
    assert lib.ssd_jpeg_encode_info(8, 8, 1, 2, tables.ctypes.data, ctypes.byref(info2)) == UNSUPPORTED    # 4:4:0


def test_coefficients_outside_baseline_range_are_an_error(fixture, restated):
    rgb, q, s, _ = fixture[jc.DC11]
    g, coef, tables = restated[jc.DC11]
    _, info = jc.lib_info(rgb.shape[0], rgb.shape[1], s, tables)
    for index, value in ((0, 2048), (0, -2048), (1, 1024), (63, -1024), (5, -32768)):
        bad = coef.copy()
        bad[index] = value
        rc, _, intact = jc.lib_entropy_encode(bad, info)
        assert rc == INVALID and intact, (index, value)
    for index, value in ((0, 1023), (0, -1024), (1, 1023), (63, -1023)):            # the largest that are in range
        ok = coef.copy()
        ok[64:] = 0
        ok[index] = value
        rc, blob, intact = jc.lib_entropy_encode(ok, info)
        assert rc == OK and intact and blob == jc.entropy_encode(g, ok, tables), (index, value)


def test_two_threads_encode_different_images_at_once(fixture, restated):
    names = [n for n in NAMES if n.startswith(("33x100_", "64x48_"))][:8]
    assert len(names) == 8

    def job(name):
        rgb, q, s, _ = fixture[name]
        return _encode(rgb, q, s, restated[name][1])[1]

    with ThreadPoolExecutor(max_workers=2) as pool:
        for _ in range(4):
            for name, got in zip(names, pool.map(job, names)):
                assert got == fixture[name][3], name
