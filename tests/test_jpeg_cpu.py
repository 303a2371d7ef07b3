"""The host half of the JPEG decoder (``ssd_jpeg_parse`` / ``ssd_jpeg_entropy_decode``: no GPU needed) and the arithmetic
the device half must reproduce: the NumPy restatement of tests/jpeg_cases.py, applied to the library's coefficients,
equals Pillow's bytes for every fixture case.  No tolerance anywhere: every comparison is equality."""
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_cases as jc

OK, INVALID, UNSUPPORTED = 0, -1, -3


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


def _decode(blob):
    rc, info, err = jc.parse(blob)
    assert rc == OK, err
    rc, coef, intact = jc.entropy_decode(blob, info)
    assert rc == OK and intact
    return info, coef


def test_fixture_was_written_by_libjpeg_turbo():
    _, versions = jc.load_fixture()
    assert versions.startswith("Pillow ") and "libjpeg-turbo" in versions
    assert len(jc.cases()) == len(set(c[0] for c in jc.cases())) >= 60


@pytest.mark.parametrize("name", [c[0] for c in jc.cases()])
def test_parse_and_restatement_equal_pillow(fixture, name):
    from PIL import Image
    blob, rgb = fixture[name]
    info, coef = _decode(blob)
    im = Image.open(io.BytesIO(blob))
    assert (info.width, info.height) == im.size and info.components == im.layers
    got = jc.restate(info, coef)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb)
    if jc.pillow_is_turbo():                            # a Pillow on another libjpeg may round differently: fixture only
        assert np.array_equal(got, jc.pillow_decode(blob))


def test_bottom_edge_replicates_the_last_real_chroma_row(fixture):
    """The open point of the design: below the last REAL chroma row (24 rows of 4:2:0 -> 12 real rows in 16 padded ones)
    h2v2 upsampling sees that row again, not row 12 of the padded block.  The two readings differ on this case, and
    Pillow agrees with the first."""
    blob, rgb = fixture["size_40x24_420"]
    blob2, rgb2 = fixture["size_17x33_420"]
    differs = False
    for b, want in ((blob, rgb), (blob2, rgb2)):
        info, coef = _decode(b)
        assert np.array_equal(jc.restate(info, coef, "real"), want)
        differs = differs or not np.array_equal(jc.restate(info, coef, "padded"), want)
    assert differs


def test_real_size_image():
    blob = jc.real_size_blob()
    info, coef = _decode(blob)
    assert (info.height, info.width) == jc.REAL_SIZE and (info.h_samp[0], info.v_samp[0]) == (2, 2)
    assert info.coef_bytes == (24 * 32 * 4 + 2 * 24 * 32) * 128
    if not jc.pillow_is_turbo():
        pytest.skip("live comparison needs a Pillow built on libjpeg-turbo")
    assert np.array_equal(jc.restate(info, coef), jc.pillow_decode(blob))


def _save(arr, **options):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **options)
    return buf.getvalue()


def _patch_sof_sampling(blob, value):
    """The same file with the first component's sampling byte of the SOF0 header replaced."""
    at = blob.index(b"\xff\xc0")
    b = bytearray(blob)
    b[at + 11] = value
    return bytes(b)


def test_unsupported_inputs_are_refused_with_a_text():
    from PIL import Image
    rgb = jc.content(24, 24, "444", "smooth")
    cmyk = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[..., :1]]), mode="CMYK").save(cmyk, "JPEG")
    cases = {
        "progressive": _save(rgb, progressive=True),
        "4:4:0": _patch_sof_sampling(_save(rgb, subsampling="4:4:4"), 0x12),
        "4:1:1": _patch_sof_sampling(_save(rgb, subsampling="4:4:4"), 0x41),
        "keep_rgb": _save(rgb, keep_rgb=True),
        "cmyk": cmyk.getvalue(),
    }
    for what, blob in cases.items():
        rc, _, err = jc.parse(blob)
        assert rc == UNSUPPORTED and err.startswith("ssd_jpeg"), (what, rc, err)
    try:
        blob = _save(rgb, subsampling=(1, 2))           # a Pillow that writes 4:4:0 itself
    except Exception:
        blob = None
    if blob is not None:
        rc, info, err = jc.parse(blob)
        assert rc == UNSUPPORTED or (info.h_samp[0], info.v_samp[0]) in ((1, 1), (2, 1), (2, 2)), err


def _mid(blob, marker):
    at = blob.index(marker)
    return at + 4 + (((blob[at + 2] << 8) | blob[at + 3]) - 2) // 2


def test_truncated_and_damaged_files_never_crash_or_write_outside():
    blob = jc.load_fixture()[0]["size_17x33_420"][0]
    rc, info, _ = jc.parse(blob)
    assert rc == OK
    n = len(blob)
    scan = blob.index(b"\xff\xda")
    scan_data = scan + 2 + ((blob[scan + 2] << 8) | blob[scan + 3])
    for cut in (0, 2, 20, _mid(blob, b"\xff\xc4"), (scan_data + n) // 2, n - 2):
        part = blob[:cut]
        rc, _, err = jc.parse(part)
        if rc == OK:                                    # the header is whole: the scan is not
            rc, _, intact = jc.entropy_decode(part, info)
            assert intact
            if cut == n - 2 and rc == OK:
                continue                                # only the EOI marker is missing: every MCU is there
        assert rc == INVALID, (cut, rc, err)
    rng = np.random.default_rng(7)
    for pos in rng.choice(np.arange(scan_data, n - 2), 64, replace=False):
        b = bytearray(blob)
        b[int(pos)] ^= 0xFF
        rc, coef, intact = jc.entropy_decode(bytes(b), info)
        assert rc in (OK, INVALID) and intact, (pos, rc)


def test_missing_tables_and_bad_restart_markers_are_invalid():
    fx = jc.load_fixture()[0]
    blob = fx["size_16x16_444"][0]
    at = blob.index(b"\xff\xc4")
    length = (blob[at + 2] << 8) | blob[at + 3]
    assert jc.parse(blob[:at] + blob[at + 2 + length:])[0] == INVALID           # the first DHT segment removed
    at = blob.index(b"\xff\xdb")
    length = (blob[at + 2] << 8) | blob[at + 3]
    without = blob[:at] + blob[at + 2 + length:]
    if b"\xff\xdb" not in without:
        assert jc.parse(without)[0] == INVALID                                     # no DQT at all
    blob = fx["restart1_420"][0]
    rc, info, _ = jc.parse(blob)
    assert rc == OK and info.restart_interval == 1 and blob.count(b"\xff\xd7") >= 1   # the counter wrapped past 7
    at = blob.index(b"\xff\xd3")
    bad = blob[:at + 1] + b"\xd5" + blob[at + 2:]
    rc, _, intact = jc.entropy_decode(bad, info)
    assert rc == INVALID and intact


def test_info_and_buffer_size_are_checked():
    import ctypes
    import ssd_hip
    fx = jc.load_fixture()[0]
    blob, other = fx["size_17x33_420"][0], fx["size_33x17_420"][0]
    _, info, _ = jc.parse(blob)
    _, info2, _ = jc.parse(other)
    assert jc.entropy_decode(blob, info2)[0] == INVALID                           # another stream's info
    store = np.full(int(info.coef_bytes) // 2, 0x5A5A, np.int16)
    rc = ssd_hip.lib().ssd_jpeg_entropy_decode(blob, len(blob), ctypes.byref(info), store.ctypes.data, store.nbytes - 128)
    assert rc == INVALID and (store == 0x5A5A).all()


def test_sixteen_threads_decode_what_one_thread_decodes(fixture):
    names = [c[0] for c in jc.cases() if c[1] != (1, 1)][::4][:16]
    assert len(names) == 16
    single = [_decode(fixture[n][0])[1] for n in names]
    with ThreadPoolExecutor(max_workers=16) as pool:
        for _ in range(4):
            many = list(pool.map(lambda n: _decode(fixture[n][0])[1], names))
            for a, b in zip(single, many):
                assert np.array_equal(a, b)
