"""Fine-tuning with frozen layers on the device (csrc/ssd_train.hip, ssd_net_set_trainable): every test is one or two
training steps of the 300 x 300 net, B = 2 for MobileNetV2 (the smallest batch with non-degenerate statistics), B = 1
for VGG16 -- the shapes of tests/test_layer_grad_gpu.py.

What is held to what:
  * pruning: freezing a prefix of the net must not change one bit of what is still trained (the tile of every conv and
    weight gradient is memoised per shape for the process, so two steps of one instance run the same kernels), frozen
    ranges of the flat gradient are exactly 0.0f, Adam leaves frozen parameters bitwise alone;
  * frozen BatchNorm: the training forward equals the INFERENCE forward of oracle/net_oracle.py within the bars
    tests/test_train.py holds the training forward to (1e-4 absolute on the probabilities, 1e-4 of the largest delta),
    the moving statistics stay bitwise, and the backward through it -- dpre = gamma * istd_moving * dout * act'(z),
    bn_bwd_apply_kernel's formula without the two batch-mean terms -- is recomputed teacher-forced in float64 from the
    device's own tensors for one layer of each kind and compared in the layer oracle's metric E at its bar E <= 16
    (oracle/layer_grad_oracle.py derives the bar; the kernels are of the classes it was derived for);
  * the matrix-core FLOP counters (ssd_net_train_matrix_flops): the weight-gradient family equals the extras' and heads'
    own 2 M K N, computed here from the layer shapes.  The two conv families (fp32-MFMA / split-bf16 tiles) are compared
    as their SUM: which family a conv shape lands in is decided by timing its tiles on the device, and a conv with a
    folded BatchNorm epilogue is timed as a shape of its own, so one family alone can rise when work moves to it while
    forward + backward-data FLOPs as a whole can only fall.

Measured on an MI355X: frozen-BatchNorm forward against the inference oracle 2.7e-5 on the probabilities, 9.6e-5 on the
deltas (largest |delta| 4.09); worst E of the backward through a frozen BatchNorm (bar 16): dW 4.9 (Conv_1), dx 6.2
(expanded_conv_depthwise), gradient handed to the residual tensor 4.9 (block_2_project); bf16 step with the backbone
frozen: loss within 5.3e-5 of the fp32 step's (bar 2e-2)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import helpers
from oracle import layer_grad_oracle as lg

pytestmark = pytest.mark.gpu

TEACHER_LAYERS = ["Conv1", "block_1_expand", "expanded_conv_depthwise", "block_1_depthwise", "block_2_project", "Conv_1"]


def _targets(hp, B, seed=3):
    from oracle import bbox_oracle as bo
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=hp["total_labels"], seed=seed)
    return bo.calculate_actual_outputs(priors, gt, gl, hp)


def _ranges(m, names):
    """Flat-vector index ranges of the parameters of the given Keras layers."""
    names = set(names)
    return [(name, off, off + int(np.prod(shape))) for name, (off, shape) in m.trainable_offsets().items()
            if name.rsplit("/", 1)[0] in names]


def _flops(m):
    mf = (ctypes.c_double * 3)()
    import ssd_hip as h
    h.check(h.lib().ssd_net_train_matrix_flops(m._net, mf), "matrix_flops")
    return [float(v) for v in mf]


def _step(m, x, yd, yl):
    loc, conf, g = m.forward_backward(x, yd, yl)
    return float((loc + conf).mean().item()), g.cpu().numpy().copy()


@pytest.fixture(scope="module")
def mbv2():
    """ONE MobileNetV2 instance, three steps on the same batch with no optimizer step in between: (all) everything
    trainable, (bn) every BatchNorm frozen, (bb) the backbone frozen as well.  Everything the tests compare is captured
    here, so they do not depend on the order they run in."""
    from models._net import SSDModel
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = helpers.hyper_params("mobilenet_v2")
    B = 2
    x = helpers.images(B, 300, seed=41)
    yd, yl = _targets(hp, B)
    m = SSDModel("mobilenet_v2", hp)
    m.set_weights({k: v.copy() for k, v in helpers.synthetic_weights("mobilenet_v2", hp).items()})
    m.compile()
    r = {"m": m, "hp": hp, "B": B, "x": x, "yd": yd, "yl": yl}
    r["loss_all"], r["g_all"] = _step(m, x, yd, yl)
    r["flops_all"] = _flops(m)
    r["w"] = m.get_weights()                     # (the all-trainable step has moved the moving statistics)
    bn = m.batch_norm_layer_names()
    assert m.set_trainable(bn, False) == bn and len(bn) == 52
    r["loss_bn"], r["g_bn"] = _step(m, x, yd, yl)
    r["w_bn"] = m.get_weights()
    r["probs"] = m.train_fetch("probs", B).reshape(B, -1, hp["total_labels"])
    r["deltas"] = m.train_fetch("deltas", B).reshape(B, -1, 4)
    specs = lg.layers("mobilenet_v2", hp)
    shapes = lg.tensor_shapes(specs, r["w"])
    r["specs"], r["shapes"] = {s["name"]: s for s in specs}, shapes
    fetched = {}
    for name in TEACHER_LAYERS + ["block_2_expand"]:
        s = r["specs"][name]
        for t in (s["tin"], s["tout"], "grad:" + s["tin"], "grad:" + s["tout"]) + (("grad:" + s["res"],) if s["res"] else ()):
            if t not in fetched and t not in ("input", "grad:input"):
                fetched[t] = m.train_fetch(t, B).reshape((B,) + shapes[t[5:] if t.startswith("grad:") else t])
    fetched["input"] = x
    r["fetched"] = fetched
    r["frozen_bb"] = m.freeze_backbone()
    r["loss_bb"], r["g_bb"] = _step(m, x, yd, yl)
    r["flops_bb"] = _flops(m)
    r["w_bb"] = m.get_weights()
    return r


# ---------------------------------------------------------------------------------------------- 1. VGG16, prefix frozen
def test_vgg16_frozen_prefix_leaves_the_rest_bitwise():
    from models._net import SSDModel
    hp = helpers.hyper_params("vgg16")
    B = 1
    x = helpers.images(B, 300, seed=43)
    yd, yl = _targets(hp, B)
    m = SSDModel("vgg16", hp)
    w0 = {k: v.copy() for k, v in helpers.synthetic_weights("vgg16", hp).items()}
    m.set_weights(w0)
    m.compile()
    _, g_all = _step(m, x, yd, yl)
    prefix = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3"]
    assert m.set_trainable(prefix, False) == prefix
    m._grads.fill_(float("nan"))                    # stale values must not pass for zeros
    _, g = _step(m, x, yd, yl)
    frozen = _ranges(m, prefix)
    assert len(frozen) == 14
    keep = np.ones(g.size, bool)
    for name, lo, hi in frozen:
        assert not g[lo:hi].any() and not np.signbit(g[lo:hi]).any(), name          # exactly +0.0f
        assert np.abs(g_all[lo:hi]).max() > 0, name                                 # ... where the full step has a gradient
        keep[lo:hi] = False
    assert keep.sum() > 0.9 * g.size
    np.testing.assert_array_equal(g[keep].view(np.uint32), g_all[keep].view(np.uint32))
    # two optimisation steps: frozen parameters bitwise unchanged, every other parameter moved
    for _ in range(2):
        m.train_on_batch(x, (yd, yl), learning_rate=1e-4)
    w2 = m.get_weights()
    offs = m.trainable_offsets()
    moved = still = 0
    for name in w0:
        if name.rsplit("/", 1)[0] in prefix:
            np.testing.assert_array_equal(w2[name].view(np.uint32), w0[name].view(np.uint32), err_msg=name)
        else:
            # (on this one image with He-normal weights parts of the tail are dead behind their ReLUs -- measured: 18 of
            # the 57 trainable parameters, biases and head kernels, have a gradient of exactly zero in the ALL-TRAINABLE
            # step as well -- and Adam does not move what has no gradient: a parameter must move where the all-trainable
            # step gives it a gradient)
            off, shape = offs[name]
            if g_all[off:off + int(np.prod(shape))].any():
                assert (w2[name] != w0[name]).any(), name
                moved += 1
            else:
                still += 1
    print("VGG16 prefix frozen: %d trainable parameters moved, %d have no gradient on this batch" % (moved, still))
    assert moved + still == 71 - 14 and moved > still


# ---------------------------------------------------------------------------------------------- 2. every BatchNorm frozen
def test_frozen_batchnorm_forward_is_the_inference_forward(mbv2):
    from oracle import net_oracle as no
    r = mbv2
    ref_deltas, ref_probs = no.forward("mobilenet_v2", r["hp"], r["w"], r["x"])
    e_p = float(np.abs(r["probs"] - ref_probs).max())
    e_d = float(np.abs(r["deltas"] - ref_deltas).max())
    print("frozen BatchNorm forward vs the inference oracle: probs %.2e, deltas %.2e of max %.3g" % (
        e_p, e_d, float(np.abs(ref_deltas).max())))
    assert e_p <= 1e-4
    assert e_d <= 1e-4 * max(1.0, float(np.abs(ref_deltas).max()))
    # ... and it differs from the batch-statistics forward the all-trainable step ran (the flag has an effect)
    assert abs(r["loss_bn"] - r["loss_all"]) > 1e-6 * abs(r["loss_all"])
    m = r["m"]
    n = 0
    for name, v in r["w"].items():
        if name.endswith(("/moving_mean", "/moving_variance")):
            np.testing.assert_array_equal(r["w_bn"][name].view(np.uint32), v.view(np.uint32), err_msg=name)
            n += 1
    assert n == 104
    for name, lo, hi in _ranges(m, m.batch_norm_layer_names()):
        assert not r["g_bn"][lo:hi].any(), name
    assert np.isfinite(r["g_bn"]).all()


def _frozen_backward(r, name):
    """Teacher-forced float64 backward of layer `name` under a frozen BatchNorm, from the device's own input, output and
    output gradient: dpre = gamma * rsqrt(moving_var + eps) * dout * act'(out), then the linear part through the layer
    oracle.  Returns (dx, dw, A_dx, A_dw): the references and the absolute-value sums of their terms."""
    s, f, w = r["specs"][name], r["fetched"], r["w"]
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    x, out, dout = t64(f[s["tin"]]), t64(f[s["tout"]]), t64(f["grad:" + s["tout"]])
    assert not (s["res"] and s["act"])
    mask = ((out > 0) & (out < 6)) if s["act"] == "relu6" else torch.ones_like(out, dtype=torch.bool)
    scale = t64(w[s["bn"] + "/gamma"]) * torch.rsqrt(t64(w[s["bn"] + "/moving_variance"]) + lg.BN_EPS)
    dpre = dout * mask * scale
    pads = lg._pads(s, x.shape[1], x.shape[2])
    res = []
    for xx, dd in ((x, dpre), (x.abs(), dpre.abs())):
        if s["kind"] == "dw":
            kernel = t64(w[name + "/depthwise_kernel"])
            res.append(lg.depthwise_backward(xx, kernel if xx is x else kernel.abs(), dd, s["stride"], pads))
        else:
            kernel = t64(w[name + "/kernel"])
            res.append(lg.conv_backward(xx, kernel if xx is x else kernel.abs(), dd, s["stride"], s["dil"], pads,
                                        need_dx=s["tin"] != "input"))
    return res[0][0], res[0][1], res[1][0], res[1][1]


@pytest.mark.parametrize("name", TEACHER_LAYERS)
def test_backward_through_a_frozen_batchnorm(mbv2, name):
    """Conv1: the im2col stem; block_1_expand: 1x1 + ReLU6; expanded_conv_depthwise / block_1_depthwise: depthwise stride 1
    / 2; block_2_project: linear + residual (the gradient handed to the residual tensor block_1_out is checked too: it is
    the output gradient plus block_2_expand's data gradient); Conv_1: the 1280-wide last conv."""
    r = mbv2
    s, f, m = r["specs"][name], r["fetched"], r["m"]
    dx, dw, A_dx, A_dw = _frozen_backward(r, name)
    kname = name + ("/depthwise_kernel" if s["kind"] == "dw" else "/kernel")
    off, shape = m.trainable_offsets()[kname]
    got_dw = r["g_bn"][off:off + int(np.prod(shape))].reshape(shape)
    E_dw, i = lg.e_metric(got_dw, dw, A_dw)
    E_dx = E_res = 0.0
    if s["tin"] != "input":
        # (each of these inputs has this layer as its only consumer)
        E_dx, j = lg.e_metric(f["grad:" + s["tin"]], dx, A_dx)
    if s["res"]:
        ex, _, A_ex, _ = _frozen_backward(r, "block_2_expand")
        assert r["specs"]["block_2_expand"]["tin"] == s["res"]
        dout = torch.from_numpy(f["grad:" + s["tout"]]).to(torch.float64)
        E_res, _ = lg.e_metric(f["grad:" + s["res"]], dout + ex, dout.abs() + A_ex)
    print("frozen BatchNorm backward %-24s E: dW %.2f, dx %.2f, residual %.2f" % (name, E_dw, E_dx, E_res))
    assert E_dw <= lg.E_BAR, "dW: E = %.3g at flat index %d" % (E_dw, i)
    assert E_dx <= lg.E_BAR and E_res <= lg.E_BAR, (E_dx, E_res)


# ---------------------------------------------------------------------------------------------- 3. backbone frozen as well
def test_frozen_backbone_prunes_the_backward(mbv2):
    r = mbv2
    m, B = r["m"], r["B"]
    names = m.layer_names()
    tail = [n for n in names if n.startswith("extra") or n[0].isdigit()]
    assert sorted(tail + r["frozen_bb"]) == sorted(names)
    n_tail = 0
    for name, lo, hi in _ranges(m, tail):
        np.testing.assert_array_equal(r["g_bb"][lo:hi].view(np.uint32), r["g_bn"][lo:hi].view(np.uint32), err_msg=name)
        # (under inference-mode BatchNorm on these synthetic moving statistics the deeper extras are dead behind their
        # ReLUs, their kernels have a zero gradient in both configurations: the layers next to the backbone must have one)
        if name.startswith(("extra1_1/", "1_conv_", "2_conv_")):
            assert np.abs(r["g_bb"][lo:hi]).max() > 0, name
        n_tail += hi - lo
    n_back = 0
    for name, lo, hi in _ranges(m, r["frozen_bb"]):
        assert not r["g_bb"][lo:hi].any(), name
        n_back += hi - lo
    assert n_tail + n_back == r["g_bb"].size
    assert r["loss_bb"] == r["loss_bn"]                         # the forward is the same: the extras have no BatchNorm
    for name, v in r["w_bn"].items():
        np.testing.assert_array_equal(r["w_bb"][name].view(np.uint32), v.view(np.uint32), err_msg=name)
    # weight-gradient FLOPs = the extras' and heads' own 2 M K N (M output pixels, K x N the kernel)
    want = 0.0
    for s in r["specs"].values():
        if s["kind"] == "head":
            H, W, _ = r["shapes"][s["tin"]]
            kn = sum(r["w"]["%d_conv_%s_output/kernel" % (s["level"] + 1, part)].size for part in ("label", "boxes"))
            want += 2.0 * B * H * W * kn
        elif s["name"].startswith("extra"):
            H, W, _ = r["shapes"][s["tout"]]
            want += 2.0 * B * H * W * r["w"][s["name"] + "/kernel"].size
    print("matrix FLOPs all-trainable %s, backbone frozen %s, expected weight-gradient %.6g" % (r["flops_all"], r["flops_bb"], want))
    assert r["flops_bb"][2] == want
    assert r["flops_bb"][2] < r["flops_all"][2]
    assert r["flops_bb"][0] + r["flops_bb"][1] < r["flops_all"][0] + r["flops_all"][1]


# ---------------------------------------------------------------------------------------------- 4. optimizer
def test_adam_leaves_frozen_parameters_alone():
    import ssd_hip as h
    from models._net import SSDModel
    from oracle import train_oracle as to
    hp = helpers.hyper_params("mobilenet_v2")
    m = SSDModel("mobilenet_v2", hp)
    w0 = {k: v.copy() for k, v in helpers.synthetic_weights("mobilenet_v2", hp).items()}
    m.set_weights(w0)
    LR = 2e-5           # tests/test_train.py's rate: its tolerance below is stated for steps of that size
    m.compile(learning_rate=LR)
    h.check(h.lib().ssd_net_train_begin(m._net, 1), "ssd_net_train_begin")
    m._train_batch = 1
    frozen = set(m.freeze_backbone())
    offs = m.trainable_offsets()
    ones = torch.ones((h.lib().ssd_net_trainable_floats(m._net),), dtype=torch.float32, device=h.device())
    m.apply_gradients(ones)
    w1 = m.get_weights()
    state = {}
    for name, (off, shape) in offs.items():
        if name.rsplit("/", 1)[0] in frozen:
            np.testing.assert_array_equal(w1[name].view(np.uint32), w0[name].view(np.uint32), err_msg=name)
            continue
        var, mm, vv = to.adam_step(w0[name], np.zeros(shape, np.float32), np.zeros(shape, np.float32), np.ones(shape, np.float32), 1,
                                    lr=LR)
        state[name] = (mm, vv)
        np.testing.assert_allclose(w1[name], var, rtol=1e-6, atol=2e-9, err_msg=name)
    assert 0 < len(state) < len(offs)
    for name in w0:                                  # the moving statistics are no business of the optimizer
        if name not in offs:
            np.testing.assert_array_equal(w1[name], w0[name], err_msg=name)
    # unfrozen, the second call moves everything: the step counter is global (t = 2), the moments of what was frozen
    # start from where they were (zero)
    m.set_trainable("*", True)
    m.apply_gradients(ones)
    w2 = m.get_weights()
    for name, (off, shape) in offs.items():
        mm, vv = state.get(name, (np.zeros(shape, np.float32), np.zeros(shape, np.float32)))
        var, _, _ = to.adam_step(w1[name], mm, vv, np.ones(shape, np.float32), 2, lr=LR)
        np.testing.assert_allclose(w2[name], var, rtol=1e-6, atol=2e-9, err_msg=name)
        assert (w2[name] != w1[name]).all(), name


# ---------------------------------------------------------------------------------------------- 5. buckets
def test_gradient_buckets_with_a_frozen_backbone():
    import ssd_hip as h
    from models._net import SSDModel
    hp = helpers.hyper_params("mobilenet_v2")
    B = 2
    x = helpers.images(B, 300, seed=31)
    yd, yl = _targets(hp, B, seed=6)
    m = SSDModel("mobilenet_v2", hp)
    m.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    m.compile()
    frozen = m.freeze_backbone()
    _, g0 = _step(m, x, yd, yl)
    for name, lo, hi in _ranges(m, frozen):
        assert not g0[lo:hi].any(), name
    starts = m._plan_gradient_buckets(B, 4)
    assert starts[0] == 0 and len(starts) == 4
    side = h.new_stream()
    m._grads.fill_(float("nan"))
    snap = torch.full_like(m._grads, float("nan"))
    torch.cuda.synchronize()
    _, _, g = m.forward_backward(x, yd, yl)
    bounds = list(starts) + [g.numel()]
    for k in reversed(range(len(starts))):
        h.check(h.lib().ssd_net_train_wait_bucket(m._net, k, h.vp(side.cuda_stream)), "wait_bucket")
        with torch.cuda.stream(side):
            snap[bounds[k]:bounds[k + 1]].copy_(g[bounds[k]:bounds[k + 1]], non_blocking=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), g0.view(np.uint32))
    np.testing.assert_array_equal(snap.cpu().numpy().view(np.uint32), g0.view(np.uint32))
    h.free_stream(side)


# ---------------------------------------------------------------------------------------------- 6. bf16 mode
def test_bf16_step_with_a_frozen_backbone(mbv2):
    """The loss bound is the one tests/test_bf16_gpu.py::test_bf16_training_step_c4_shape holds the bf16 step to against
    the fp32 step: 2 % of the fp32 loss.  The fp32 side is the shared instance's step in the same configuration."""
    from models._net import SSDModel
    r = mbv2
    m = SSDModel("mobilenet_v2", r["hp"], precision="bf16")
    m.set_weights(r["w"])
    m.compile()
    frozen = m.freeze_backbone()
    assert frozen == r["frozen_bb"]
    loss, g = _step(m, r["x"], r["yd"], r["yl"])
    print("bf16 step, backbone frozen: loss %.6f vs fp32 %.6f (rel %.2e)" % (loss, r["loss_bb"], abs(loss - r["loss_bb"]) / abs(r["loss_bb"])))
    assert np.isfinite(g).all()
    for name, lo, hi in _ranges(m, frozen):
        assert not g[lo:hi].any(), name
    tail = [n for n in m.layer_names() if n not in set(frozen)]
    for name, lo, hi in _ranges(m, tail):
        if name.startswith(("extra1_1/", "1_conv_", "2_conv_")):          # (the deeper extras are dead on these weights, see above)
            assert np.abs(g[lo:hi]).max() > 0, name
    assert abs(loss - r["loss_bb"]) <= 2e-2 * abs(r["loss_bb"])
    assert _flops(m)[1] > 0


# ---------------------------------------------------------------------------------------------- 7. trainer.main
def test_trainer_freeze_backbone(tmp_path, monkeypatch, capsys):
    from models._net import keras_default_init
    from utils import h5_reader
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_TRAINER_FREEZE", "backbone")
    monkeypatch.setenv("SSD_TRAINER_EPOCHS", "1")
    monkeypatch.setenv("SSD_TRAINER_STEPS", "2")
    monkeypatch.setenv("SSD_TRAINER_BATCH", "2")
    monkeypatch.setenv("SSD_TRAINER_AUGMENT", "0")
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "frozen: 104 layers (backbone)" in out and np.isfinite(hist["loss"]).all()
    path = os.path.join("trained", "ssd_mobilenet_v2_model_weights.h5")
    assert os.path.exists(path)
    w = h5_reader.load_keras_weights(path)
    from models._net import SSDModel
    # (the initial weights are drawn in parameter-table order: the specs come from a net, which needs no device)
    w0 = keras_default_init(SSDModel("mobilenet_v2", helpers.hyper_params("mobilenet_v2")).param_specs, "mobilenet_v2")
    assert set(w) == set(w0)
    n_back = n_tail = 0
    changed = set()
    for name, v in w.items():
        if name.startswith("extra") or name[0].isdigit():
            if (np.asarray(v) != w0[name]).any():
                changed.add(name.rsplit("/", 1)[0])
            n_tail += 1
        else:
            np.testing.assert_array_equal(np.asarray(v, np.float32).view(np.uint32), w0[name].view(np.uint32), err_msg=name)
            n_back += 1
    assert n_back == 52 * 5 and n_tail == 8 * 2 + 12 * 2
    # the heads have moved.  (Not necessarily all twelve convs in two steps: the loss reaches a level only through its
    # positive priors and mined hard negatives, and the four priors of the 1 x 1 level had neither here -- its two convs
    # kept a gradient of exactly zero.  The two large levels always have both.)
    heads = {"%d_conv_%s_output" % (i, part) for i in range(1, 7) for part in ("label", "boxes")}
    first = {"%d_conv_%s_output" % (i, part) for i in (1, 2) for part in ("label", "boxes")}
    assert first <= changed and len(heads & changed) >= 8 and "extra1_1" in changed, sorted(heads - changed)
