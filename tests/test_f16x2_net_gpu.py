"""The two-plane fp16 conv tiles ``dmah_*`` inside MobileNetV2-SSD300 (csrc/ssd_net.hip): block 13's expanded map and
Conv_1's output are ReLU6 outputs, so their plane readers -- head 1, head 2, extra1_1 -- may take the fp16 pair.

One fresh process with a NaN-poisoned arena (``SSD_HIP_DEBUG_POISON=1``) runs, on forced tables (the shipped table with the
three lines replaced): the ``dmah_2x2_2x2`` table twice, the ``dma3_2x2_2x2`` table, the ``dmah`` table under option
``conv_f16x2`` 0, the ``dmah`` table with ``extra1_2`` (a ReLU input) forced onto ``dmah`` too, and the ``dmah`` table at
B = 5 (tiles crossing image boundaries)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from test_fullsize_gpu import _assert_deltas

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READERS = ("1_conv_heads", "2_conv_heads", "extra1_1")
E13, CONV1 = "block_13_expand_relu", "out_relu"

CHILD = r'''
import os, sys
sys.path[:0] = [%(repo)r, os.path.join(%(repo)r, "tf-ssd_amd"), os.path.join(%(repo)r, "tests")]
import numpy as np
import helpers
from test_plane_only_gpu import forced_table
from models.ssd_mobilenet_v2 import get_model
assert os.environ.get("SSD_HIP_DEBUG_POISON") == "1"
hp = helpers.hyper_params("mobilenet_v2")
w = helpers.synthetic_weights("mobilenet_v2", hp)
READERS = ("1_conv_heads", "2_conv_heads", "extra1_1")

def run(tag, B, tile, extra=(), f16x2=1):
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    m.set_tuning(forced_table("mobilenet_v2", hp, B, {n: tile for n in READERS + tuple(extra)}))
    m.set_option("conv_f16x2", f16x2)
    d, p = [t.detach().cpu().numpy() for t in m(helpers.images(B, 300, seed=21))]
    cfg = {r["name"]: r["config"] for r in m.layers(B)}
    out = {"deltas": d, "probs": p}
    for name in ("1_conv_heads", "2_conv_heads", "extra1_1", "extra1_2"):
        out["cfg_" + name] = np.array(cfg[name])
    for name in ("block_13_expand_relu", "out_relu"):
        pl, npl = m.fetch_planes(name)
        out["np_" + name] = np.array(npl)
        out["act_" + name] = m.fetch_activation(name)           # a plane-only tensor: the joined planes
        out["same_" + name] = np.array(pl is not None and np.array_equal(pl.view(np.uint32), out["act_" + name].view(np.uint32)))
    out["mem_planes"] = np.array(m.memory_summary()["planes"])
    return {tag + "/" + k: v for k, v in out.items()}

save = {}
save.update(run("h", 2, "dmah_2x2_2x2"))
save.update(run("h2", 2, "dmah_2x2_2x2"))
save.update(run("b", 2, "dma3_2x2_2x2"))
save.update(run("off", 2, "dmah_2x2_2x2", f16x2=0))
save.update(run("x", 2, "dmah_2x2_2x2", extra=("extra1_2",)))
save.update(run("h5", 5, "dmah_2x2_2x2"))
save.update(run("b5", 5, "dma3_2x2_2x2"))
np.savez(sys.argv[1], **save)
print("f16x2-child-ok")
'''


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("f16x2") / "runs.npz")
    env = dict(os.environ, SSD_HIP_DEBUG_POISON="1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO}, path], env=env, text=True, capture_output=True, timeout=600)
    assert out.returncode == 0 and "f16x2-child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    z = dict(np.load(path))
    return lambda tag: {k[len(tag) + 1:]: v for k, v in z.items() if k.startswith(tag + "/")}


def _agree(a, b):
    """The bound of the fp32 net-parity test (tests/test_fullsize_gpu.py: 1e-4 absolute on the probabilities, _assert_deltas)."""
    hp = helpers.hyper_params("mobilenet_v2")
    assert np.isfinite(a["probs"]).all() and np.isfinite(a["deltas"]).all()
    print("dmah vs dma3: probs max |d| %.3e, deltas %.3e" % (np.abs(a["probs"] - b["probs"]).max(), np.abs(a["deltas"] - b["deltas"]).max()))
    assert np.abs(a["probs"] - b["probs"]).max() <= 1e-4
    _assert_deltas(a["deltas"], b["deltas"], hp["variances"])


def test_dmah_table_runs_on_two_plane_tensors_and_agrees_with_dma3(runs):
    a, b = runs("h"), runs("b")
    for n in READERS:
        assert str(a["cfg_" + n]).startswith("dmah_2x2_2x2"), (n, a["cfg_" + n])
        assert str(b["cfg_" + n]).startswith("dma3_2x2_2x2"), (n, b["cfg_" + n])
    for name in (E13, CONV1):
        assert int(a["np_" + name]) == 2 and int(b["np_" + name]) == 3, name
        assert bool(a["same_" + name]), name                  # plane-only: the fetch IS the joined planes
        assert np.isfinite(a["act_" + name]).all(), name
        # the joined value against the exact three-plane tensor: the representation bound (values in [0, 6])
        err = np.abs(a["act_" + name].astype(np.float64) - b["act_" + name].astype(np.float64))
        assert (err <= 2.0 ** -22 * np.abs(b["act_" + name].astype(np.float64)) + 2.0 ** -33).all(), (name, err.max())
    # ssd_net_memory_bytes counts the fp16 weight planes of the three layers with the planes: 4 bytes per padded weight,
    # (5184 x 112 + 11520 x 160 + 1280 x 256) x 4 = 11.0 MB on top of the activation planes
    extra = int(a["mem_planes"]) - int(b["mem_planes"])
    assert extra == (5184 * 112 + 11520 * 160 + 1280 * 256) * 4, extra
    _agree(a, b)


def test_dmah_table_is_deterministic(runs):
    a, a2 = runs("h"), runs("h2")
    for k in ("deltas", "probs"):
        np.testing.assert_array_equal(a[k].view(np.uint32), a2[k].view(np.uint32))


def test_option_off_reproduces_the_dma3_table_bitwise(runs):
    off, b = runs("off"), runs("b")
    for n in READERS:
        assert str(off["cfg_" + n]) == str(b["cfg_" + n]), n
    for name in (E13, CONV1):
        assert int(off["np_" + name]) == 3
    for k in ("deltas", "probs"):
        np.testing.assert_array_equal(off[k].view(np.uint32), b[k].view(np.uint32))


def test_relu_input_falls_back_to_the_dma3_twin(runs):
    x, a = runs("x"), runs("h")
    assert str(x["cfg_extra1_2"]).startswith("dma3_2x2_2x2"), x["cfg_extra1_2"]
    for n in READERS:
        assert str(x["cfg_" + n]).startswith("dmah_2x2_2x2"), n
    assert np.isfinite(x["probs"]).all() and np.abs(x["probs"] - a["probs"]).max() <= 1e-4


def test_batch_of_five_crosses_image_boundaries(runs):
    a, b = runs("h5"), runs("b5")
    assert a["probs"].shape[0] == 5 and int(a["np_" + E13]) == 2 and int(a["np_" + CONV1]) == 2
    _agree(a, b)
