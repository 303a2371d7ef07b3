"""What the device entropy coder (``ssd_jpeg_pack``) needs from the host, no GPU: ``ssd_jpeg_encode_header`` writes the
header ``ssd_jpeg_entropy_encode`` wrote before it was factored out (the Pillow fixture pins both), and the packer of
``data_utils.jpeg_pack_batch`` lays descriptors and headers out as ONE upload.  Every comparison is equality."""
import ctypes

import numpy as np
import pytest

import jpeg_encode_cases as jc
import ssd_hip
from utils import data_utils

OK, INVALID = 0, -1
NAMES = [c[0] for c in jc.cases()]


@pytest.fixture(scope="module")
def fixture():
    return jc.load_fixture()[0]


def _header(info, out_bytes=ssd_hip.JPEG_HEADER_BYTES, guard=64, fill=0xA5):
    store = np.full(out_bytes + 2 * guard, fill, np.uint8)
    written = ctypes.c_size_t(77)
    rc = ssd_hip.lib().ssd_jpeg_encode_header(ctypes.byref(info), store.ctypes.data + guard, out_bytes, ctypes.byref(written))
    intact = bool((store[:guard] == fill).all() and (store[guard + out_bytes:] == fill).all())
    return rc, store[guard:guard + out_bytes], int(written.value), intact


def test_header_equals_the_front_of_every_fixture_stream_and_the_restatement(fixture):
    for name in NAMES:
        rgb, q, s, blob = fixture[name]
        tables = jc.lib_quality_tables(q)
        rc, info = jc.lib_info(rgb.shape[0], rgb.shape[1], s, tables)
        assert rc == OK, name
        rc, got, written, intact = _header(info)
        want = jc.header(jc.Geometry(rgb.shape[0], rgb.shape[1], *jc.SAMPLING[s]), jc.quality_tables(q))
        assert rc == OK and intact and written == ssd_hip.JPEG_HEADER_BYTES == len(want), name
        assert got.tobytes() == want == blob[:len(want)], name


def test_header_refuses_a_short_buffer_a_bad_info_and_null(fixture):
    lib = ssd_hip.lib()
    rc, info = jc.lib_info(17, 15, "4:2:0", jc.lib_quality_tables(75))
    assert rc == OK
    rc, got, written, intact = _header(info, out_bytes=ssd_hip.JPEG_HEADER_BYTES - 1)
    assert rc == INVALID and written == 0 and intact and bool((got == 0xA5).all())   # nothing written
    assert lib.ssd_last_error().decode().startswith("ssd_jpeg_encode_header")
    info.mcus_x += 1                                                               # no longer what ssd_jpeg_encode_info fills in
    assert _header(info)[0] == INVALID
    written = ctypes.c_size_t(0)
    assert lib.ssd_jpeg_encode_header(None, np.zeros(700, np.uint8).ctypes.data, 700, ctypes.byref(written)) == INVALID
    info.mcus_x -= 1
    assert lib.ssd_jpeg_encode_header(ctypes.byref(info), None, 700, ctypes.byref(written)) == INVALID


def test_entropy_encode_still_writes_the_fixture(fixture):
    """The refactor changed no byte: the host coder on the restated coefficients is the fixture, case by case."""
    for name in NAMES:
        rgb, q, s, blob = fixture[name]
        tables = jc.lib_quality_tables(q)
        g, coef = jc.forward(rgb, s, tables)
        rc, info = jc.lib_info(rgb.shape[0], rgb.shape[1], s, tables)
        rc2, got, intact = jc.lib_entropy_encode(coef, info)
        assert rc == OK and rc2 == OK and intact and got == blob, name


def test_packer_layout_is_one_upload_in_order():
    shapes, samplings = [(17, 15), (1, 1), (37, 53)], [(2, 2), (1, 1), (2, 1)]
    tables = np.stack([jc.lib_quality_tables(q) for q in (75, 30, 100)])
    enc = data_utils._jpeg_encode_layout(shapes, samplings)["desc"]
    layout = data_utils._jpeg_pack_layout(enc, shapes, samplings, tables)
    desc = layout["desc"]
    assert desc.dtype == ssd_hip.JPEG_PACK_DESC_DTYPE and desc.dtype.itemsize == 40 and len(desc) == 3
    # descriptors first, then the headers: multiples of 16, in order, none overlapping, all inside the one buffer
    ends = [desc.nbytes]
    for b in range(3):
        at = int(desc[b]["header_offset"])
        assert at % 16 == 0 and at >= ends[-1] and at == layout["headers_at"][b]
        ends.append(at + ssd_hip.JPEG_HEADER_BYTES)
    assert layout["total"] % 16 == 0 and ends[-1] <= layout["total"] < ends[-1] + 16
    # what the forward call's descriptors say, carried over
    blocks = [12, 3, 4 * 5 * 4]
    assert [int(v) for v in desc["block_start"]] == [0, 12, 15] == [int(v) for v in enc["block_start"]]
    assert [int(v) for v in desc["coef_offset"]] == [int(v) for v in enc["coef_offset"]]
    assert all(int(v) % 16 == 0 for v in desc["coef_offset"]) and int(desc["reserved"].max()) == 0
    assert [(int(d["H"]), int(d["W"])) for d in desc] == shapes and [(int(d["h_samp"]), int(d["v_samp"])) for d in desc] == samplings
    bounds = [int(ssd_hip.lib().ssd_jpeg_encode_bound(ctypes.byref(i))) for i in layout["infos"]]
    assert bounds == [ssd_hip.JPEG_HEADER_BYTES + n * 416 + 4 for n in blocks]
    assert layout["out_bytes"] == sum((n + 15) // 16 * 16 for n in bounds)
    # ONE buffer is filled: the descriptors at 0, each header where its descriptor says
    host = np.full(layout["total"], 0xEE, np.uint8)
    data_utils._jpeg_pack_fill(host, layout)
    assert host[:desc.nbytes].tobytes() == desc.tobytes()
    for b, ((H, W), (hs, vs)) in enumerate(zip(shapes, samplings)):
        at = int(desc[b]["header_offset"])
        want = jc.header(jc.Geometry(H, W, hs, vs), tables[b])
        assert host[at:at + len(want)].tobytes() == want
    # the workspace the library asks for holds the unstuffed streams at their worst case (224 bytes a block) and more
    n = sum(blocks)
    ws = int(ssd_hip.lib().ssd_jpeg_pack_workspace_bytes(desc.ctypes.data, 3))
    assert ws % 16 == 0 and n * (224 + 8) <= ws <= n * (224 + 8) + 1024
    assert ssd_hip.lib().ssd_jpeg_pack_workspace_bytes(None, 0) == 0
