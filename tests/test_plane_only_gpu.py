"""Plane-only activations (csrc/ssd_net.hip ``Tensor::plane_only``, option ``plane_only``): an activation whose running
readers are all dense convs on LDS-DMA tiles lives as its bf16 planes alone -- the producer (conv epilogue, split-K reduce,
whole-image block kernel and its combine launch, max-pool, L2 normalisation) skips the fp32 store.

* op level: ``ssd_conv2d_planes`` with planes requested and NO fp32 output: the joined planes are bitwise the fp32 output
  of the same call with both outputs, with and without split-K, on a shape with a row tail (M = 75) and a channel tail
  (Cout = 20);
* net level: MobileNetV2-300 with heads 1-2, ``Conv_1`` and ``extra1_1`` on ``dma3_*`` tiles, ``plane_only`` 1 against 0:
  raw head outputs and detections bitwise equal, at B = 2 and B = 5 (another group count of the whole-image kernel);
* ``SSD_HIP_DEBUG_POISON=1`` (NaN arena; a fresh process, the variable is read at start): outputs finite and equal, and
  a fetch of a plane-only tensor returns the joined planes = the fp32 values of the ``plane_only`` 0 run;
* a tensor with one LDS-DMA and one register-staged reader keeps its fp32 copy;
* VGG16-300 at B = 2 (its table runs conv2_2 ... conv6 on ``dma3_*``): outputs bitwise equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
from test_conv_gpu import same, _np, guarded
from test_convdma_gpu import make_planes, join_planes, dma_configs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMA_TILE = "dma3_2x2_2x2"
FORCED = ("1_conv_heads", "2_conv_heads", "Conv_1", "extra1_1")
E13, CONV1 = "block_13_expand_relu", "out_relu"


def conv_planes(x, w, cfg, split_k, want_fp32):
    """``ssd_conv2d_planes`` (3x3 SAME, BN scale / shift, ReLU6) with the plane output requested; fp32 output optional.
    Returns (rc, fp32 output or None, joined planes)."""
    import ssd_hip as h
    lib = h.lib()
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    pt, pb = same(H, kh, 1, 1)
    d = h.ConvDesc(B, H, W, Cin, Cout, kh, kw, 1, 1, pt, pt, pb, pb, 2, 0)
    wd = h.to_dev(w)
    npk = lib.ssd_conv_packed_weight_floats(kh, kw, Cin, Cout)
    packed = torch.full((npk + 4096,), float("nan"), dtype=torch.float32, device=wd.device)[:npk]
    h.check(lib.ssd_conv_pack_weights(h.ptr(wd), kh, kw, Cin, Cout, h.ptr(packed), h.stream()), "pack")
    keep, p0, pstride = make_planes(x, 3)
    rng = np.random.default_rng(5)
    sd = guarded(rng.uniform(0.5, 1.5, Cout).astype(np.float32))
    hd = guarded(rng.uniform(-0.5, 0.5, Cout).astype(np.float32))
    M = B * H * W
    n_out = M * Cout
    ostride = (M * ((Cout + 31) // 32 * 32) + 63) // 64 * 64          # whole 32-channel slices of every pixel
    op = torch.full((3 * ostride + 64,), 0x7fc0, dtype=torch.int16, device=wd.device)
    out = torch.full((B, H, W, Cout), float("nan"), dtype=torch.float32, device=wd.device) if want_fp32 else None
    ws = torch.empty(split_k * n_out, dtype=torch.float32, device=wd.device) if split_k > 1 else None
    rc = lib.ssd_conv2d_planes(ctypes.byref(d), h.vp(p0), 3, pstride, h.ptr(packed), h.ptr(sd), h.ptr(hd), None,
                               h.ptr(out), 0, 0, h.ptr(op), ostride, cfg, split_k, h.ptr(ws), h.stream())
    if rc:
        return rc, None, None
    joined = join_planes(op.data_ptr(), n_out, Cout, 3, ostride).reshape(B, H, W, Cout)
    return rc, (_np(out) if want_fp32 else None), joined


@pytest.mark.parametrize("split_k", [1, 2])
def test_conv_writes_planes_without_an_fp32_output(split_k):
    import ssd_hip as h
    rng = np.random.default_rng(17)
    x = rng.standard_normal((3, 5, 5, 32)).astype(np.float32)            # M = 75: row tail; Cout = 20: channel tail
    w = (rng.standard_normal((3, 3, 32, 20)) / np.sqrt(288)).astype(np.float32)
    cfg = {n: c for c, n in dma_configs(b"dma3_")}[DMA_TILE]
    rc, both_out, both_planes = conv_planes(x, w, cfg, split_k, want_fp32=True)
    assert rc == 0, h.lib().ssd_last_error()
    assert np.isfinite(both_out).all() and np.abs(both_out).max() > 0.1
    np.testing.assert_array_equal(both_planes.view(np.uint32), both_out.view(np.uint32))
    rc, _, only_planes = conv_planes(x, w, cfg, split_k, want_fp32=False)
    assert rc == 0, h.lib().ssd_last_error()
    np.testing.assert_array_equal(only_planes.view(np.uint32), both_out.view(np.uint32))


def forced_table(backbone, hp, B, force):
    """The shipped table of (backbone, B) with the lines of ``force`` {layer: config} replaced (the split-K factor stays)."""
    import tuning
    text = tuning.load_shipped(tuning.table_key(backbone, 300, hp["total_labels"], hp["aspect_ratios"], B))
    assert text is not None
    lines = []
    for l in tuning.body(text).splitlines():
        parts = l.split(" ")
        if parts[0] in force:
            parts[1] = force[parts[0]]
        lines.append(" ".join(parts))
    return "\n".join(lines) + "\n"


def run_net(backbone, B, table, plane_only, fetch=()):
    from utils import bbox_utils
    get_model = __import__("models.ssd_%s" % backbone, fromlist=["get_model"]).get_model
    hp = helpers.hyper_params(backbone)
    m = get_model(hp, max_batch=B)
    m.set_weights(helpers.synthetic_weights(backbone, hp))
    if table is not None:
        m.set_tuning(table)
    m.set_option("plane_only", plane_only)
    x = helpers.images(B, 300, seed=21)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    out = {}
    out["deltas"], out["probs"] = [_np(t) for t in m(x)]
    for name in fetch:
        out[name] = m.fetch_activation(name)
    out["boxes"], out["labels"], out["scores"], out["valid"] = [_np(t) for t in m.predict_on_device(x, priors, hp["variances"])]
    out["configs"] = {r["name"]: r["config"] for r in m.layers(B)}
    return out


def assert_same_outputs(a, b):
    for k in ("deltas", "probs", "boxes", "labels", "scores", "valid"):
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    assert (a["scores"] > 0).sum() > 0


_REF = {}


def mbv2_reference(B):
    """``plane_only`` 0 run of MobileNetV2-300 on the forced table: computed once per batch size, shared, never changed."""
    if B not in _REF:
        hp = helpers.hyper_params("mobilenet_v2")
        table = forced_table("mobilenet_v2", hp, B, {n: DMA_TILE for n in FORCED})
        _REF[B] = (table, run_net("mobilenet_v2", B, table, 0, fetch=(E13, CONV1)))
    return _REF[B]


@pytest.mark.parametrize("B", [2, 5])
def test_mobilenet_plane_only_matches_the_double_store(B):
    table, ref = mbv2_reference(B)
    for n in FORCED:
        assert ref["configs"][n].startswith(DMA_TILE), (n, ref["configs"][n])
    got = run_net("mobilenet_v2", B, table, 1, fetch=(E13, CONV1))
    assert_same_outputs(got, ref)
    for name in (E13, CONV1):           # the fetch of a plane-only tensor joins its planes: the same fp32 values
        np.testing.assert_array_equal(got[name].view(np.uint32), ref[name].view(np.uint32), err_msg=name)


CHILD = r'''
import os, sys
sys.path[:0] = [%(repo)r, os.path.join(%(repo)r, "tf-ssd_amd"), os.path.join(%(repo)r, "tests")]
import numpy as np
import helpers
import test_plane_only_gpu as t
assert os.environ.get("SSD_HIP_DEBUG_POISON") == "1"
hp = helpers.hyper_params("mobilenet_v2")
table = t.forced_table("mobilenet_v2", hp, 2, {n: t.DMA_TILE for n in t.FORCED})
a = t.run_net("mobilenet_v2", 2, table, 1, fetch=(t.E13, t.CONV1))
mixed = t.forced_table("mobilenet_v2", hp, 2, {"1_conv_heads": t.DMA_TILE, "2_conv_heads": "mfma3_2x2_2x2", "Conv_1": t.DMA_TILE,
                                               "extra1_1": t.DMA_TILE})
b = t.run_net("mobilenet_v2", 2, mixed, 1, fetch=(t.E13, t.CONV1))
save = {}
for tag, r in (("a", a), ("b", b)):
    for k, v in r.items():
        if k != "configs":
            save[tag + "_" + k] = v
    save[tag + "_head2"] = np.array(r["configs"]["2_conv_heads"])
    save[tag + "_extra1_1"] = np.array(r["configs"]["extra1_1"])
np.savez(sys.argv[1], **save)
print("poison-child-ok")
'''


@pytest.fixture(scope="module")
def poisoned(tmp_path_factory):
    """One fresh process with a NaN-poisoned arena: run ``a`` = every reader of E and of Conv_1's output on LDS-DMA tiles
    (both plane-only), run ``b`` = head 2 on a register-staged tile (Conv_1's output keeps its fp32 copy)."""
    path = str(tmp_path_factory.mktemp("plane_only") / "poison.npz")
    env = dict(os.environ, SSD_HIP_DEBUG_POISON="1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO}, path], env=env, text=True, capture_output=True, timeout=600)
    assert out.returncode == 0 and "poison-child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return dict(np.load(path))


def unpack(z, tag):
    return {k[len(tag) + 1:]: v for k, v in z.items() if k.startswith(tag + "_")}


def test_poisoned_arena_outputs_and_fetches(poisoned):
    _, ref = mbv2_reference(2)
    got = unpack(poisoned, "a")
    assert_same_outputs(got, ref)
    for name in (E13, CONV1):
        assert np.isfinite(got[name]).all(), name
        np.testing.assert_array_equal(got[name].view(np.uint32), ref[name].view(np.uint32), err_msg=name)


def test_tensor_with_a_register_staged_reader_keeps_its_fp32_copy(poisoned):
    _, ref = mbv2_reference(2)
    got = unpack(poisoned, "b")
    assert str(got["head2"]).startswith("mfma3_2x2_2x2") and str(got["extra1_1"]).startswith(DMA_TILE)
    # head 2 read Conv_1's fp32 output out of a NaN-poisoned arena: it was written, and the fetch returns it
    assert np.isfinite(got[CONV1]).all()
    np.testing.assert_array_equal(got[CONV1].view(np.uint32), ref[CONV1].view(np.uint32))
    assert_same_outputs(got, ref)


def test_vgg16_plane_only_matches_the_double_store():
    ref = run_net("vgg16", 2, None, 0)
    assert sum(c.startswith("dma3_") for c in ref["configs"].values()) >= 3, ref["configs"]
    got = run_net("vgg16", 2, None, 1)
    assert_same_outputs(got, ref)
