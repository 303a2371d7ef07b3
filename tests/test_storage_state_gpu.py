"""Activation storage as a function of the net's state (csrc/ssd_storage.hip): which tensors exist as planes, in which
form, whether the fp32 copy exists and which launch writes the planes must follow the options, the routes and the chosen
tiles alone -- never the order in which a net got there.

* option walk: ONE MobileNetV2-300 net at B = 2 on the forced table of ``test_plane_only_gpu.py`` (heads 1-2, ``Conv_1``,
  ``extra1_1`` on ``dma3_2x2_2x2``) walks ``plane_only`` 1, 0, 1, ``image_ticket`` 0, 1, 0, ``fuse_image`` 1, 0, 1,
  ``fuse_blocks`` 1, 0, 1 and ``set_timing`` on, off, a forward after each.  After every step the raw head outputs, the
  detections, every layer's config string and ``fetch_planes``' count and plane number for block 13's expanded map and
  ``Conv_1``'s output are bitwise those of a fresh net brought directly into that state (one per distinct state, cached);
  live planes joined back are bitwise ``fetch_activation`` (three planes: the join is exact; for a tensor with both
  copies this compares the planes with the fp32 store);
* the timing toggle leaves nothing of the above changed;
* the same walk in a fresh process with a NaN-poisoned arena (``SSD_HIP_DEBUG_POISON=1``): everything finite at every
  step -- a split pass over an fp32 slot nobody wrote, or a reader of a copy nobody wrote, shows here;
* VGG16-300 at B = 2 on its shipped table walks ``plane_only`` 1, 0, 1 with the same assertions on the outputs;
* the fp16 pair: with ``extra1_1`` on a ``dmah_*`` tile ``Conv_1``'s output has 2 planes exactly when every reader of
  its planes is on ``dmah_*``, 3 when head 2 is forced back to ``dma3_*``; the two agree at the bar of
  ``test_f16x2_net_gpu.py``."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from test_f16x2_net_gpu import _agree
from test_plane_only_gpu import CONV1, DMA_TILE, E13, FORCED, _np, forced_table

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2
OUTPUTS = ("deltas", "probs", "boxes", "labels", "scores", "valid")
DEFAULT = {"plane_only": 1, "image_ticket": 0, "fuse_image": 1, "fuse_blocks": 1, "timing": 0}
WALK = [("plane_only", 1), ("plane_only", 0), ("plane_only", 1),
        ("image_ticket", 0), ("image_ticket", 1), ("image_ticket", 0),
        ("fuse_image", 1), ("fuse_image", 0), ("fuse_image", 1),
        ("fuse_blocks", 1), ("fuse_blocks", 0), ("fuse_blocks", 1),
        ("timing", 1), ("timing", 0)]
VGG_WALK = [("plane_only", 1), ("plane_only", 0), ("plane_only", 1)]


def new_net(backbone, table):
    get_model = __import__("models.ssd_%s" % backbone, fromlist=["get_model"]).get_model
    hp = helpers.hyper_params(backbone)
    m = get_model(hp, max_batch=B)
    m.set_weights(helpers.synthetic_weights(backbone, hp))
    if table is not None:
        m.set_tuning(table)
    return m


def apply(m, name, value):
    if name == "timing":
        m.set_timing(value)
    else:
        m.set_option(name, value)


def observe(m, backbone, tensors):
    """One forward and one predict in the net's current state, and what the public surface shows of its storage."""
    from utils import bbox_utils
    hp = helpers.hyper_params(backbone)
    x = helpers.images(B, 300, seed=21)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    out = {}
    out["deltas"], out["probs"] = [_np(t) for t in m(x)]
    out["boxes"], out["labels"], out["scores"], out["valid"] = [_np(t) for t in m.predict_on_device(x, priors, hp["variances"])]
    out["configs"] = [(r["name"], r["config"]) for r in m.layers(B)]
    out["mem_planes"] = m.memory_summary()["planes"]
    for name in tensors:
        planes, npl = m.fetch_planes(name)
        act = m.fetch_activation(name)
        out["planes/" + name] = (0 if planes is None else planes.size, npl)
        out["finite/" + name] = bool(np.isfinite(act).all() and (planes is None or np.isfinite(planes).all()))
        # live planes joined back against the activation (three planes: exact)
        out["joined/" + name] = planes is None or npl != 3 or np.array_equal(planes.view(np.uint32), act.view(np.uint32))
    return out


def assert_same_state(got, want, what):
    for k in OUTPUTS:
        assert np.isfinite(got[k]).all(), (what, k)
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg="%s: %s" % (what, k))
    assert (got["scores"] > 0).sum() > 0, what
    assert got["configs"] == want["configs"], (what, [(a, b) for a, b in zip(got["configs"], want["configs"]) if a != b])
    for k in got:
        if k.startswith("planes/"):
            assert got[k] == want[k], (what, k, got[k], want[k])
        if k.startswith("joined/") or k.startswith("finite/"):
            assert got[k] and want[k], (what, k)


def walk(backbone, table, steps, tensors):
    """One net through `steps`; yields (step, state, observation) after each."""
    m = new_net(backbone, table)
    state = dict(DEFAULT)
    for name, value in steps:
        apply(m, name, value)
        state[name] = value
        yield (name, value), dict(state), observe(m, backbone, tensors)


_FRESH = {}


def fresh(backbone, table, state, tensors):
    """A fresh net brought directly into `state` (every option set before its first forward): one per distinct state,
    computed once, shared, never changed."""
    key = (backbone, table, tuple(sorted(state.items())))
    if key not in _FRESH:
        m = new_net(backbone, table)
        for name, value in sorted(state.items()):
            apply(m, name, value)
        _FRESH[key] = observe(m, backbone, tensors)
    return _FRESH[key]


def mbv2_table():
    return forced_table("mobilenet_v2", helpers.hyper_params("mobilenet_v2"), B, {n: DMA_TILE for n in FORCED})


def test_option_walk_matches_fresh_nets_in_every_state():
    table = mbv2_table()
    seen = {}
    before_toggle = None
    for step, state, got in walk("mobilenet_v2", table, WALK, (E13, CONV1)):
        want = fresh("mobilenet_v2", table, state, (E13, CONV1))
        assert_same_state(got, want, "after %s %d" % step)
        seen[tuple(sorted(state.items()))] = got
        if step == ("fuse_blocks", 1):
            before_toggle = got
        if step == ("timing", 0):           # the toggle on, off: nothing differs from before it
            assert_same_state(got, before_toggle, "after the timing toggle")
            assert got["mem_planes"] == before_toggle["mem_planes"]
    assert len(seen) == 6
    # the forced tiles run in every state, and both tensors have three live planes wherever their readers run
    base = seen[tuple(sorted(DEFAULT.items()))]
    cfg = dict(base["configs"])
    for n in FORCED:
        assert cfg[n].startswith(DMA_TILE), (n, cfg[n])
    for name in (E13, CONV1):
        assert base["planes/" + name][0] > 0 and base["planes/" + name][1] == 3, (name, base["planes/" + name])


CHILD = r'''
import os, sys
sys.path[:0] = [%(repo)r, os.path.join(%(repo)r, "tf-ssd_amd"), os.path.join(%(repo)r, "tests")]
import numpy as np
import test_storage_state_gpu as t
assert os.environ.get("SSD_HIP_DEBUG_POISON") == "1"
bad = []
for step, state, got in t.walk("mobilenet_v2", t.mbv2_table(), t.WALK, (t.E13, t.CONV1)):
    for k in t.OUTPUTS:
        if not np.isfinite(got[k]).all():
            bad.append((step, k))
    for k, v in got.items():
        if (k.startswith("finite/") or k.startswith("joined/")) and not v:
            bad.append((step, k))
    if not (got["scores"] > 0).sum() > 0:
        bad.append((step, "no detections"))
print("not finite: %%r" %% (bad,))
if not bad:
    print("storage-child-ok")
'''


def test_option_walk_on_a_poisoned_arena_stays_finite():
    env = dict(os.environ, SSD_HIP_DEBUG_POISON="1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO}], env=env, text=True, capture_output=True, timeout=600)
    assert out.returncode == 0 and "storage-child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_vgg16_plane_only_walk_matches_fresh_nets():
    states = set()
    for step, state, got in walk("vgg16", None, VGG_WALK, ()):
        assert_same_state(got, fresh("vgg16", None, state, ()), "vgg16 after %s %d" % step)
        states.add(state["plane_only"])
    assert states == {0, 1}
    cfg = dict(fresh("vgg16", None, DEFAULT, ())["configs"])
    assert sum(c.startswith("dma3_") for c in cfg.values()) >= 3, cfg


def test_fp16_pair_follows_every_reader_of_the_planes():
    hp = helpers.hyper_params("mobilenet_v2")
    readers = ("2_conv_heads", "extra1_1")            # the conv layers that read Conv_1's output

    def run(force):
        return observe(new_net("mobilenet_v2", forced_table("mobilenet_v2", hp, B, force)), "mobilenet_v2", (E13, CONV1))

    pair = run({n: "dmah_2x2_2x2" for n in readers})
    cfg = dict(pair["configs"])
    assert all(cfg[n].startswith("dmah_") for n in readers), cfg
    assert pair["planes/" + CONV1][0] > 0 and pair["planes/" + CONV1][1] == 2, pair["planes/" + CONV1]
    # one reader back on the bf16 planes: the tensor keeps the exact split and the other reader runs its twin
    mixed = run({"2_conv_heads": "dma3_2x2_2x2", "extra1_1": "dmah_2x2_2x2"})
    cfg = dict(mixed["configs"])
    assert cfg["2_conv_heads"].startswith("dma3_2x2_2x2") and cfg["extra1_1"].startswith("dma3_2x2_2x2"), cfg
    assert mixed["planes/" + CONV1][0] > 0 and mixed["planes/" + CONV1][1] == 3, mixed["planes/" + CONV1]
    for r in (pair, mixed):
        assert r["finite/" + CONV1] and r["finite/" + E13] and r["joined/" + CONV1] and r["joined/" + E13]
    _agree(pair, mixed)
