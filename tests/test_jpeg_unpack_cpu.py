"""The host side of the device entropy decoder, without a GPU: ``ssd_jpeg_scan_plan`` against an independent walk over
the markers, and ``ssd_jpeg_entropy_decode_subseq`` -- the kernels' decode core and phases as loops over "threads" --
against ``ssd_jpeg_entropy_decode``, bit for bit, on the fixture, on real-size streams and on malformed ones."""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_unpack_cases as uc

OK, INVALID, UNSUPPORTED = uc.OK, uc.INVALID, uc.UNSUPPORTED
NAMES = [c[0] for c in jc.cases()]


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


@pytest.fixture(scope="module")
def real():
    """{name: (blob, info, the host decoder's coefficients)}, decoded once."""
    out = {}
    for name, blob in uc.real_streams().items():
        rc, info, err = jc.parse(blob)
        assert rc == OK, (name, err)
        rc, coef, intact = jc.entropy_decode(blob, info)
        assert rc == OK and intact, name
        out[name] = (blob, info, coef)
    return out


def test_scan_plan_equals_an_independent_marker_walk_on_every_fixture_case(fixture):
    assert len(NAMES) == 66
    for name in NAMES:
        blob = fixture[name][0]
        rc, info, _ = jc.parse(blob)
        assert rc == OK
        rc, plan, segs = uc.scan_plan(blob, info)
        assert rc == OK, name
        begin, end, want = uc.walk_segments(blob, info)
        assert (plan.data_begin, plan.data_end, plan.segments) == (begin, end, len(want)), name
        assert [(int(s["first_byte"]), int(s["bytes"]), int(s["first_mcu"])) for s in segs] == want, name
        assert plan.segments == uc.RESTART_CASES.get(name, 1), name
        assert blob[end:end + 2] == b"\xff\xd9", name                               # the fixture's scans end at EOI
        assert uc.scan_plan(blob, info, capacity=max(plan.segments - 1, 0))[0] == INVALID   # room for one segment less


def test_scan_plan_tables_are_the_files_code_lengths(fixture):
    """The device-ready tables decode every code the DHT segments define: walking look / maxcode / valoff / vals over all
    16-bit prefixes gives each symbol exactly 2^(16 - length) times."""
    blob = fixture["optimize_420"][0]
    rc, info, _ = jc.parse(blob)
    rc, plan, _ = uc.scan_plan(blob, info)
    assert rc == OK
    tables = {}
    at = 0
    while True:
        at = blob.find(b"\xff\xc4", at)
        if at < 0:
            break
        end, q = at + 2 + ((blob[at + 2] << 8) | blob[at + 3]), at + 4
        while q < end:
            counts = list(blob[q + 1:q + 17])
            tables[blob[q]] = (counts, list(blob[q + 17:q + 17 + sum(counts)]))
            q += 17 + sum(counts)
        at = end
    sos = blob.index(b"\xff\xda")
    for c in range(3):
        sel = blob[sos + 6 + 2 * c]
        for a, key in ((0, sel >> 4), (1, 0x10 | (sel & 15))):
            counts, symbols = tables[key]
            t = plan.huff[2 * c + a]
            code, k = 0, 0
            for length in range(1, 17):
                for _ in range(counts[length - 1]):
                    if length <= 8:
                        assert t.look[code << (8 - length)] == (length << 8) | symbols[k]
                    else:
                        assert t.look[code >> (length - 8)] == 0 and code <= t.maxcode[length]
                        assert t.vals[t.valoff[length] + code] == symbols[k]
                    code, k = code + 1, k + 1
                code <<= 1


def test_a_damaged_restart_marker_is_invalid(fixture):
    blob = fixture["restart1_420"][0]
    rc, info, _ = jc.parse(blob)
    at = blob.index(b"\xff\xd3")
    bad = blob[:at + 1] + b"\xd5" + blob[at + 2:]
    assert uc.walk_segments(bad, info) is None
    assert uc.scan_plan(bad, info)[0] == INVALID
    rc, _, intact = uc.subseq_decode(bad, info, 128)
    assert rc == INVALID and intact
    assert uc.scan_plan(blob[:at], info)[0] == INVALID                              # fewer segments than the frame needs


@pytest.mark.parametrize("bits", [128, 160, 1024])
def test_subsequence_decode_equals_the_host_decoder_on_every_fixture_case(fixture, bits):
    several = 0
    for name in NAMES:
        blob = fixture[name][0]
        rc, info, _ = jc.parse(blob)
        rc, want, _ = jc.entropy_decode(blob, info)
        assert rc == OK
        rc, got, intact = uc.subseq_decode(blob, info, bits)
        assert rc == OK and intact, (name, rc)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        if name.startswith("q") and not name.endswith("_L"):
            several += (uc.scan_plan(blob, info)[1].data_end - uc.scan_data_at(blob)) * 8 > 2 * bits
    assert bits != 128 or several >= 12                                           # 128 bits: several subsequences inside 17x17 streams


def test_subseq_bits_and_arguments_are_checked(fixture):
    blob, other = fixture["size_17x33_420"][0], fixture["size_33x17_420"][0]
    _, info, _ = jc.parse(blob)
    _, info2, _ = jc.parse(other)
    rc, want, _ = jc.entropy_decode(blob, info)
    rc0, got, intact = uc.subseq_decode(blob, info, 0)                             # 0: the built-in default
    assert rc0 == OK and intact and np.array_equal(got, want)
    for bits in (64, 96, 130, 1000, -128, 1 << 20):
        rc, got, intact = uc.subseq_decode(blob, info, bits)
        assert rc == UNSUPPORTED and intact and (got == 0x5A5A).all(), bits
    assert uc.subseq_decode(blob, info2, 128)[0] == INVALID                        # another stream's info
    assert uc.scan_plan(blob, info2)[0] == INVALID
    import ctypes
    import ssd_hip
    store = np.full(int(info.coef_bytes) // 2, 0x5A5A, np.int16)
    rc = ssd_hip.lib().ssd_jpeg_entropy_decode_subseq(blob, len(blob), ctypes.byref(info), store.ctypes.data, store.nbytes - 128, 128)
    assert rc == INVALID and (store == 0x5A5A).all()


@pytest.mark.parametrize("bits", [128, 1024])
def test_real_size_streams_cross_many_chunks(real, bits):
    for name, (blob, info, want) in real.items():
        rc, plan, segs = uc.scan_plan(blob, info)
        assert rc == OK
        rc, got, intact = uc.subseq_decode(blob, info, bits)
        assert rc == OK and intact, (name, rc)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        if bits == 128:                                                           # the carry between 256-subsequence chunks is exercised
            longest = max(int(s["bytes"]) for s in segs) * 8 // bits
            assert longest > (256 if name != "restart_rows" else 100), (name, longest)
    assert real["restart_rows"][1].restart_interval == 32 and real["noise_444_q100"][0].count(b"\xff\x00") > 300
    assert len(real["noise_444_q100"][0]) > 150000


def _check_malformed(base, info, bits_list):
    accepted = refused = 0
    for name, blob in uc.malformed(base):
        rc_host, want, intact = jc.entropy_decode(blob, info)
        assert intact and rc_host in (OK, INVALID), name
        for bits in bits_list:
            rc, got, intact = uc.subseq_decode(blob, info, bits)
            assert intact and rc in (OK, INVALID), (name, bits, rc)
            if rc == OK:                                                          # the model is at least as strict as the host decoder
                assert rc_host == OK and np.array_equal(got, want), (name, bits)
            if rc_host != OK:
                assert rc != OK, (name, bits)
        accepted += rc_host == OK
        refused += rc_host != OK
    return accepted, refused


def test_malformed_small_streams(fixture):
    base = fixture["size_17x33_420"][0]
    _, info, _ = jc.parse(base)
    accepted, refused = _check_malformed(base, info, (128, 160, 1024))
    assert accepted + refused == 72 and refused >= 8


def test_malformed_real_size_streams(real):
    base, info, _ = real["real_size"]
    accepted, refused = _check_malformed(base, info, (128, 1024))
    assert accepted + refused == 72 and accepted >= 1 and refused >= 8
