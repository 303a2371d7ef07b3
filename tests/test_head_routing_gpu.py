"""The fused head conv's TWO-DESTINATION store (csrc/ssd_conv.h ``ConvParams::n_split``: channels below A L go to the
concatenated label buffer, the rest to the box buffer; a 4-wide store that straddles the split -- A = 6 puts it at channel
126 -- falls back to scalars) has four implementations: the shared MFMA epilogue, ``splitk_reduce_kernel``,
``conv_skinny_kernel`` and ``conv_wino_kernel``.  A whole-net test runs whichever one the table of its batch size names.

Here ONE MobileNetV2-SSD300 at B = 3 is re-pinned (``set_tuning``) with all six ``N_conv_heads`` lines forced onto the first
and the last tile of ``mfma_*``, ``mfma3_*``, ``dma3_*``, ``dmah_*``, ``skinny_*`` and the Winograd tiles with split-K 1, and onto
the first tile of the four implicit-GEMM families with split-K 3 (the reduce kernel; Winograd's split goes through the same
reduce kernel and is held at op level): 16 tables.  After each forward

* ``layers(B)`` names the forced config on every head -- with the documented fallback as an expected value, not a skip: a
  ``dmah_*`` line on a head whose input is not a ReLU6 output (levels 3-6: the extras end in ReLU) runs the ``dma3_*`` twin of
  the same tile and split (no head at B = 3 has M > 8192, the other documented fallback, of the skinny tiles);
* deltas and probabilities are held to the float64 head oracle (oracle/conv_oracle.py ``head_f64``) fed with the six
  feature maps fetched from the same forward: 1e-4 absolute on the probabilities, ``_assert_deltas`` on the deltas;
* all forced runs agree with each other within the same bars."""
import hashlib

import numpy as np
import pytest

import helpers
from oracle import conv_oracle as cv
from test_conv_gpu import _np
from test_fullsize_gpu import _assert_deltas
from test_plane_only_gpu import forced_table

pytestmark = pytest.mark.gpu

B = 3
HEADS = ["%d_conv_heads" % i for i in range(1, 7)]
FEATS = [("block_13_expand_relu", 19), ("out_relu", 10), ("extra1_2", 5), ("extra2_2", 3), ("extra3_2", 2), ("extra4_2", 1)]
RELU6_INPUT = (True, True, False, False, False, False)      # block 13's expanded map, Conv_1's output; the extras end in ReLU
FAMILY_PREFIX = ["mfma_", "mfma3_", "dma3_", "dmah_", "skinny_", "wino_"]
# (family prefix, which tile of the family, split-K): 12 + 4 = 16 forced tables
FORCED = [(f, which, 1) for f in FAMILY_PREFIX for which in ("first", "last")] + \
         [(f, "first", 3) for f in ("mfma_", "mfma3_", "dma3_", "dmah_")]
assert len(FORCED) <= 16


def forced_table_split(backbone, hp, batch, force):
    """``forced_table`` of tests/test_plane_only_gpu.py with the split-K factor forced too: ``force`` = {layer: (config, split)}."""
    lines = []
    for l in forced_table(backbone, hp, batch, {n: cfg for n, (cfg, _) in force.items()}).splitlines():
        parts = l.split(" ")
        if parts[0] in force:
            assert parts[1] == force[parts[0]][0]
            parts[2] = str(force[parts[0]][1])
        lines.append(" ".join(parts))
    return "\n".join(lines) + "\n"


def tile_of(prefix, which):
    import ssd_hip as h
    lib = h.lib()
    names = [lib.ssd_conv_config_name(c).decode() for c in range(lib.ssd_conv_num_configs())]
    fam = [n for n in names if n.startswith(prefix)]
    assert len(fam) >= 2, (prefix, fam)
    return fam[0] if which == "first" else fam[-1]


def expected_config(tile, split, relu6_input):
    """What ``layers(B)`` must report for a head forced onto (tile, split)."""
    if tile.startswith("dmah_") and not relu6_input:        # the two-plane fp16 form is for ReLU6-bounded inputs: the dma3 twin runs
        tile = "dma3_" + tile[len("dmah_"):].replace("_ks2", "")
    return tile if split == 1 else "%s/s%d" % (tile, split)


@pytest.fixture(scope="module")
def net():
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    heads = [tuple(np.asarray(w["%d_conv_%s_output/%s" % (i, kind, var)], np.float32)
                   for kind, var in (("label", "kernel"), ("label", "bias"), ("boxes", "kernel"), ("boxes", "bias")))
             for i in range(1, 7)]
    return m, hp, heads, helpers.images(B, 300, seed=33)


_ORACLE = {}        # digest of the six feature maps -> (deltas, probs) in float64: computed once per distinct input
RUNS = {}           # forced table -> (deltas, probs) of its forward


def head_oracle(feats, heads, L):
    key = hashlib.sha256(b"".join(f.tobytes() for f in feats)).hexdigest()
    if key not in _ORACLE:
        d, p = cv.head_f64(feats, heads, L)
        d.setflags(write=False)
        p.setflags(write=False)
        _ORACLE[key] = (d, p)
    return _ORACLE[key]


@pytest.mark.parametrize("prefix,which,split", FORCED, ids=["%s%s_split%d" % f for f in FORCED])
def test_heads_forced_onto_one_tile(net, prefix, which, split):
    m, hp, heads, x = net
    tile = tile_of(prefix, which)
    m.set_tuning(forced_table_split("mobilenet_v2", hp, B, {n: (tile, split) for n in HEADS}))
    d, p = [_np(t) for t in m(x)]
    assert m.tuning_info["source"] == "explicit" and m.tuning_info["choices_timed_on_device"] == 0, m.tuning_info
    ran = {r["name"]: r["config"] for r in m.layers(B) if r["flops"] > 0}
    want = {n: expected_config(tile, split, r6) for n, r6 in zip(HEADS, RELU6_INPUT)}
    assert {n: ran.get(n) for n in HEADS} == want
    feats = [m.fetch_activation(name).reshape(B, s, s, hd[0].shape[2]) for (name, s), hd in zip(FEATS, heads)]
    assert all(np.isfinite(f).all() for f in feats)
    rd, rp = head_oracle(feats, heads, hp["total_labels"])
    assert d.shape == rd.shape == (B, 2268, 4) and p.shape == rp.shape == (B, 2268, 21)
    perr, derr = float(np.abs(p - rp).max()), float(np.abs(d - rd).max())
    print("heads on %s split %d: probs max abs err %.2e, deltas %.2e (max |delta| %.2f)" % (tile, split, perr, derr, np.abs(rd).max()))
    assert perr <= 1e-4
    _assert_deltas(d, rd, hp["variances"])
    RUNS[(tile, split)] = (d, p)


def test_forced_runs_agree_with_each_other():
    assert len(RUNS) == len(FORCED), sorted(RUNS)
    hp = helpers.hyper_params("mobilenet_v2")
    keys = sorted(RUNS)
    worst = 0.0
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            worst = max(worst, float(np.abs(RUNS[a][1] - RUNS[b][1]).max()))
            assert np.abs(RUNS[a][1] - RUNS[b][1]).max() <= 1e-4, (a, b)
            _assert_deltas(RUNS[a][0], RUNS[b][0], hp["variances"])
    print("%d forced tables: probabilities agree within %.2e" % (len(keys), worst))
