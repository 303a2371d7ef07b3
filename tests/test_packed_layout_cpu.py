"""The four host packers of ``utils/data_utils.py`` (ragged preprocessing, Lanczos resize, JPEG decode, JPEG encode)
without a device: for the small cases of tests/packed_layout_cases.py each packer's layout scalars, descriptor bytes and
the sha256 of the filled staging buffer equal what tests/golden/packed_layouts.json records from the commit BEFORE the
packers were folded onto one layout helper.  Every comparison is equality; the fixture is never regenerated from the code
under test."""
import pytest

import packed_layout_cases as pc
from utils import data_utils


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def test_fixture_records_the_commit_it_was_made_at(golden):
    assert len(golden["commit"]) == 40 and set(golden["packers"]) == {"ragged", "lanczos", "jpeg_decode", "jpeg_encode"}
    assert golden["packers"]["lanczos"]["scalars"]["size"] == list(pc.OUT_SIZE)


@pytest.mark.parametrize("packer", ["ragged", "lanczos", "jpeg_decode"])
def test_packer_lays_out_and_fills_what_it_did_before(golden, packer):
    got = getattr(pc, packer)(data_utils)
    want = golden["packers"][packer]
    assert got["scalars"] == want["scalars"]
    assert got["desc"] == want["desc"] and got.get("out_desc") == want.get("out_desc")
    assert got["sha256"] == want["sha256"]


def test_encode_packer_lays_out_and_fills_what_it_did_before(golden):
    got = pc.jpeg_encode(data_utils, data_utils._jpeg_encode_fill)
    assert got == golden["packers"]["jpeg_encode"]


def test_device_resident_lanczos_layout_ends_after_the_tables():
    """``resize_lanczos_jpeg_batch``'s form: sizes only, the offsets of another buffer, no pixels in this one."""
    shapes = pc.SHAPES
    offsets = [0, 16, 224, 1920]
    full = data_utils._lanczos_layout(pc.pixels(shapes, 12), *pc.OUT_SIZE)
    lay = data_utils._lanczos_layout(shapes, *pc.OUT_SIZE, src_offsets=offsets)
    assert lay["total"] == lay["src_at"] == full["src_at"] and lay["tables_at"] == full["tables_at"]
    assert list(lay["desc"]["src_offset"]) == offsets
    for field in ("tmp_offset", "H", "W", "h_bounds", "h_k", "h_ksize", "v_bounds", "v_k", "v_ksize"):
        assert list(lay["desc"][field]) == list(full["desc"][field])
