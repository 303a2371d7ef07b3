"""Shared by tests/test_packed_layout_cpu.py and the fixture script (tests/golden/make_packed_layouts_golden.py): the four
host packers of ``utils/data_utils.py`` (ragged preprocessing, Lanczos resize, JPEG decode, JPEG encode) run on small
seeded inputs without a device, each reduced to what a byte-exact refactor must keep: the layout's scalar keys, the
descriptor records as bytes, and the sha256 of the filled staging buffer."""
import hashlib
import json
import os

import numpy as np

import jpeg_cases as jc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_layouts.json")

SHAPES = [(1, 1), (7, 9), (33, 17), (300, 300)]                                    # (H, W)
OUT_SIZE = (300, 300)                               # the last image skips both Lanczos passes
JPEG_STREAMS = ["size_7x9_420", "size_17x33_444", "size_1x1_422", "size_33x17_L"]
RAW_SHAPE = (5, 4)
ENC_SHAPES, ENC_SAMPLINGS = [(17, 15), (8, 8)], [(2, 2), (1, 1)]
SCALAR_KEYS = ("out_at", "total", "rgb_bytes", "plane_bytes", "tables_at", "coef_bytes", "src_at", "n_ints", "tmp_bytes", "size")


def pixels(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def _record(layout, host):
    out = {"scalars": {k: (list(layout[k]) if isinstance(layout[k], tuple) else int(layout[k])) for k in SCALAR_KEYS if k in layout},
           "desc": layout["desc"].tobytes().hex(), "sha256": hashlib.sha256(host.tobytes()).hexdigest()}
    if "out_desc" in layout:
        out["out_desc"] = layout["out_desc"].tobytes().hex()
    return out


def _filled(layout, fill):
    host = np.zeros(layout["total"], np.uint8)
    fill(host)
    return _record(layout, host)


def ragged(du):
    arrays = pixels(SHAPES, 11)
    layout = du._ragged_layout(arrays)
    return _filled(layout, lambda host: du._ragged_fill(host, arrays, layout))


def lanczos(du):
    arrays = pixels(SHAPES, 12)
    layout = du._lanczos_layout(arrays, *OUT_SIZE)
    return _filled(layout, lambda host: du._lanczos_fill(host, arrays, layout))


def jpeg_decode(du):
    fixture = jc.load_fixture()[0]

    def no_fallback(blob):
        raise AssertionError("a fixture stream the library does not decode")
    items = du._jpeg_items([fixture[n][0] for n in JPEG_STREAMS] + pixels([RAW_SHAPE], 13), no_fallback)
    layout = du._jpeg_layout(items)
    failed = []
    out = _filled(layout, lambda host: du._jpeg_fill(host, items, layout, failed))   # entropy-decodes in place
    assert failed == []
    return out


def encode_tables():
    """uint16 [B,2,64]: the quality-75 and quality-30 tables, one pair per image."""
    import ssd_hip
    tables = np.empty((len(ENC_SHAPES), 2, 64), np.uint16)
    for b, q in enumerate((75, 30)):
        assert ssd_hip.lib().ssd_jpeg_quality_tables(q, tables[b].ctypes.data) == 0
    return tables


def jpeg_encode(du, fill):
    """``fill(host, layout, tables)``: how ``jpeg_forward_batch`` writes its upload."""
    layout = du._jpeg_encode_layout(ENC_SHAPES, ENC_SAMPLINGS)
    tables = encode_tables()
    return _filled(layout, lambda host: fill(host, layout, tables))


def compute(du, encode_fill):
    return {"ragged": ragged(du), "lanczos": lanczos(du), "jpeg_decode": jpeg_decode(du), "jpeg_encode": jpeg_encode(du, encode_fill)}


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
