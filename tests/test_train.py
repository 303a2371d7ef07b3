"""N1 backward + Adam + data-parallel step: the native training step
(csrc/ssd_train.hip through the C ABI) against torch-CPU autograd of the same graph
(oracle/train_oracle.py).  Bars: network outputs 1e-4 abs; per-image losses 1e-4 rel; every
parameter gradient within 1e-3 of the tensor's max |gradient| (fp32, ~50 layers, batch statistics);
BatchNorm moving averages 1e-5; Adam update vs the NumPy ApplyAdam on the same gradients 1e-6."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 1e-3
LR = 2e-5      # Adam's first steps move EVERY weight by ~lr: small enough for a first-order decrease on random weights


def test_gradient_buckets_and_adam_oracle():
    sys.path.insert(0, os.path.join(REPO, "tf-ssd_amd"))
    import parallel
    from oracle import train_oracle as to
    assert parallel.gradient_buckets(10, None) == [(0, 10)]
    assert parallel.gradient_buckets(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert parallel.gradient_buckets(0, 4) == []
    import torch
    assert parallel.allreduce_gradients(torch.ones(5)) == 1          # no process group: no-op
    # Adam first step moves every weight by ~lr against the gradient sign
    g = np.array([0.5, -2.0, 1e-3], np.float32)
    var, m, v = to.adam_step(np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), g, 1)
    np.testing.assert_allclose(var, -1e-3 * np.sign(g), rtol=5e-3)
    np.testing.assert_allclose(m, 0.1 * g, rtol=1e-6)
    np.testing.assert_allclose(v, 0.001 * g * g, rtol=2e-5)


_DP_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tf-ssd_amd")]
import parallel
rank, _, world = parallel.init_distributed("gloo")
rng = np.random.default_rng(100 + rank)
g = torch.from_numpy(rng.standard_normal(1000).astype(np.float32))
ref = sum(np.random.default_rng(100 + r).standard_normal(1000).astype(np.float32) for r in range(world))
w = parallel.allreduce_gradients(g, bucket_floats=int(sys.argv[2]) or None)
assert w == world
np.testing.assert_allclose(g.numpy(), ref, rtol=1e-6, atol=1e-6)
# averaged update is identical on every rank (replicas stay in sync)
upd = g / w
gathered = [torch.empty_like(upd) for _ in range(world)]
dist.all_gather(gathered, upd)
for t in gathered:
    assert torch.equal(t, gathered[0])
dist.destroy_process_group()
print("DP_OK", rank)
'''


_DP_READY_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tf-ssd_amd")]
import parallel
rank, _, world = parallel.init_distributed("gloo")
n = 1003
g = torch.from_numpy(np.random.default_rng(100 + rank).standard_normal(n).astype(np.float32))
ref = sum(np.random.default_rng(100 + r).standard_normal(n).astype(np.float32) for r in range(world))
starts = parallel.bucket_starts(n, 4)
assert starts[0] == 0 and all(s % 4 == 0 for s in starts) and len(starts) == 4 and starts == sorted(set(starts))
order = []
w = parallel.allreduce_gradients_as_ready(g, starts, wait_bucket=lambda k, st: order.append(k), comm_stream=None)
assert w == world and order == [3, 2, 1, 0], order          # issued in the order the backward finishes them: from the END
np.testing.assert_allclose(g.numpy(), ref, rtol=1e-6, atol=1e-6)
dist.destroy_process_group()
print("DP_OK", rank)
'''


def test_two_process_gloo_gradient_buckets_as_ready(tmp_path):
    """World-size-2 gloo run of the bucket-as-ready exchange: buckets go out last-to-first (the order the native
    backward completes them), every bucket behind its completion hook, the sum is exact."""
    script = tmp_path / "w.py"
    script.write_text(_DP_READY_WORKER)
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), REPO], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "DP_OK %d" % r in o, o[-2000:]


@pytest.mark.parametrize("bucket", [0, 300])
def test_two_process_gloo_gradient_allreduce(tmp_path, bucket):
    """World-size-2 gloo run of the gradient exchange (single flat all-reduce and bucketed)."""
    script = tmp_path / "w.py"
    script.write_text(_DP_WORKER)
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), REPO, str(bucket)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "DP_OK %d" % r in o, o[-2000:]


def _hwc(m, name):
    n = m.train_fetch(name, 1).size
    # per-image H*W*C of a named activation: recover H, W, C from the graph's tensor table
    shapes = getattr(m, "_act_shapes", None)
    if shapes is None:
        from oracle import net_oracle as no
        acts = {}
        no.forward(m.backbone, m.hyper_params, {k: np.zeros(s, np.float32) + (1.0 if k.endswith("variance") else 0.0)
                                                for k, s in m.param_specs},
                   np.zeros((1, m.img_size, m.img_size, 3), np.float32), acts)
        shapes = m._act_shapes = {k: v.shape[1:] for k, v in acts.items() if getattr(v, "ndim", 0) == 4}
    assert int(np.prod(shapes[name])) == n
    return shapes[name]


def _targets(hp, B, seed=3):
    from oracle import bbox_oracle as bo
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=hp["total_labels"], seed=seed)
    yd, yl = bo.calculate_actual_outputs(priors, gt, gl, hp)
    return yd, yl


@pytest.mark.gpu
def test_train_step_matches_autograd_oracle():
    import torch
    from models.ssd_mobilenet_v2 import get_model
    from oracle import train_oracle as to
    from ssd_loss import CustomLoss
    hp = helpers.hyper_params("mobilenet_v2")
    w = {k: v.copy() for k, v in helpers.synthetic_weights("mobilenet_v2", hp).items()}
    B = 4
    x = helpers.images(B, 300, seed=21)
    yd, yl = _targets(hp, B)
    assert (yl[..., 1:].sum(-1) > 0).sum(1).min() > 0
    m = get_model(hp)
    m.set_weights(w)
    cl = CustomLoss(hp["neg_pos_ratio"], hp["loc_loss_alpha"])
    m.compile(loss=[cl.loc_loss_fn, cl.conf_loss_fn])
    loc, conf, g = m.forward_backward(x, yd, yl)
    loc, conf, g = loc.cpu().numpy(), conf.cpu().numpy(), g.cpu().numpy().copy()
    probs = m.train_fetch("probs", B).reshape(B, -1, hp["total_labels"])
    deltas = m.train_fetch("deltas", B).reshape(B, -1, 4)
    # the hard-negative selection the device made on ITS probabilities (bit-exactness of the
    # selection rule itself is tests/test_loss.py); the oracle differentiates with the same mask
    cl.conf_loss_fn(yl, probs)
    fm = cl.last_final_mask.cpu().numpy()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    # ... and with the device's ReLU / ReLU6 pass-masks (a handful of the ~10^7 activations sit
    # within fp32 noise of 0 or 6; one flipped mask element moves upstream gradients by percents)
    masks = []
    for name in to.mobilenet_v2_act_names():
        a = m.train_fetch(name, B)
        masks.append(((a > 0) & ((a < 6) | name.startswith("extra"))).reshape(B, *_hwc(m, name)))
    ref = to.train_step("mobilenet_v2", hp, w, x, yd, yl, 3.0, 1.0, final_mask=fm, act_masks=masks)
    free = to.train_step("mobilenet_v2", hp, w, x, yd, yl, 3.0, 1.0)          # un-synchronised oracle
    assert np.abs(probs - ref["probs"]).max() <= 1e-4
    assert np.abs(deltas - ref["deltas"]).max() <= 1e-4 * max(1.0, float(np.abs(ref["deltas"]).max()))
    np.testing.assert_allclose(loc, ref["loc"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(conf, ref["conf"], rtol=1e-4, atol=1e-6)
    # selection agrees with the oracle's own (near-ties aside)
    own = to.lo.conf_loss_fn(yl, ref["probs"], 3.0, return_parts=True)[2]
    assert (own != fm).mean() < 1e-3
    offs = m.trainable_offsets()
    assert set(offs) == set(ref["grads"])
    flips = 0
    for name in to.mobilenet_v2_act_names():
        ra = free["acts"][name]
        a = m.train_fetch(name, B).reshape(ra.shape)
        assert np.abs(a - ra).max() <= 1e-3, name
        flips += int((((a > 0) != (ra > 0)) | ((a < 6) != (ra < 6))).sum())
    print("activation pass-mask flips vs the free-running oracle: %d" % flips)
    for name in ("block_13_expand_relu", "out_relu", "extra1_1", "block_1_out"):
        rg = ref["act_grads"][name]
        got = m.train_fetch("grad:" + name, B).reshape(rg.shape)
        assert np.abs(got - rg).max() <= GRAD_TOL * np.abs(rg).max(), name
    errs = []
    for name, (off, shape) in offs.items():
        got = g[off:off + int(np.prod(shape))].reshape(shape)
        rg = ref["grads"][name]
        # (a *_project_BN/beta feeds a BatchNorm'ed conv: its exact gradient is 0 and both sides hold
        # ~1e-6 of rounding noise -- hence the absolute floor)
        scale = max(float(np.abs(rg).max()), 1e-2)
        errs.append((float(np.abs(got - rg).max()) / scale, name, scale))
    for e in sorted(errs)[-12:]:
        print("grad %-42s err %.2e of max(|g|max, 1e-2) = %.3e" % (e[1], e[0], e[2]))
    worst = max(errs)
    print("worst relative gradient error %.2e (%s)" % worst[:2])
    assert worst[0] <= GRAD_TOL, "%s: gradient off by %.3e of its max (%.3e)" % (worst[1], worst[0], worst[2])
    # free-running oracle (its own masks): same gradients up to the effect of the few flipped masks
    for name, (off, shape) in offs.items():
        got = g[off:off + int(np.prod(shape))].reshape(shape)
        rg = free["grads"][name]
        # (max-norm is chaotic here -- a flipped mask element moves single entries by tens of percent --
        # so the un-synchronised comparison is in the L2 norm)
        assert np.linalg.norm(got - rg) <= 0.25 * np.linalg.norm(rg) + 1e-5, name
    # BatchNorm moving averages after one training forward
    after = m.get_weights()
    for name, val in ref["moving"].items():
        np.testing.assert_allclose(after[name], val, rtol=1e-5, atol=1e-6, err_msg=name)
    # Adam: two steps vs the NumPy ApplyAdam on the device's own gradients
    before = {k: v.copy() for k, v in after.items()}
    m.apply_gradients(m._grads, learning_rate=LR)
    step1 = m.get_weights()
    st = {}
    for name, (off, shape) in offs.items():
        gg = g[off:off + int(np.prod(shape))].reshape(shape)
        var, mm, vv = to.adam_step(before[name], np.zeros(shape, np.float32), np.zeros(shape, np.float32), gg, 1, lr=LR)
        st[name] = (mm, vv)
        np.testing.assert_allclose(step1[name], var, rtol=1e-6, atol=2e-9, err_msg=name)
    loc2, conf2, g2 = m.forward_backward(x, yd, yl)
    g2 = g2.cpu().numpy().copy()
    m.apply_gradients(m._grads, learning_rate=LR, grad_scale=0.5)
    step2 = m.get_weights()
    for name in ("Conv1/kernel", "block_5_depthwise/depthwise_kernel", "bn_Conv1/gamma", "extra2_2/bias",
                 "1_conv_label_output/kernel", "6_conv_boxes_output/bias"):
        off, shape = offs[name]
        gg = g2[off:off + int(np.prod(shape))].reshape(shape) * np.float32(0.5)
        var, _, _ = to.adam_step(step1[name], st[name][0], st[name][1], gg, 2, lr=LR)
        np.testing.assert_allclose(step2[name], var, rtol=1e-6, atol=2e-9, err_msg=name)
    # the step reduces the loss on the same batch (sanity of sign / scale)
    assert float((loc2 + conf2).mean()) < float((loc + conf).mean())
    # inference after training re-finalises from the updated parameters
    d, p = m(x[:1])
    assert np.isfinite(p.cpu().numpy()).all()


@pytest.mark.gpu
def test_train_step_c4_per_gpu_shape():
    """BASELINE configs[3] (C4) at its per-GPU shape: SSD300-MobileNetV2 training step, B = 32, targets
    from the GPU matcher.  The autograd oracle covers B = 4 above; here the full-size step is checked
    through the loss oracle on the device's own training-mode head outputs, the whole-batch BatchNorm
    statistics of the first layer, bitwise repeatability, the data-parallel identity (gradient scaled
    by 1/world == gradient of the 1/world-scaled loss) and three Adam steps on the same batch."""
    from models.ssd_mobilenet_v2 import get_model
    from oracle import loss_oracle as lo
    from ssd_loss import CustomLoss
    hp = helpers.hyper_params("mobilenet_v2")
    w = {k: v.copy() for k, v in helpers.synthetic_weights("mobilenet_v2", hp).items()}
    B = 32
    x = helpers.images(8, 300, seed=5)
    x = np.concatenate([x * s for s in (1.0, 0.8, 0.6, 0.9)]).astype(np.float32)
    yd, yl = _targets(hp, B)
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    cl = CustomLoss(hp["neg_pos_ratio"], hp["loc_loss_alpha"])
    m.compile(loss=[cl.loc_loss_fn, cl.conf_loss_fn])
    loc, conf, g = m.forward_backward(x, yd, yl)
    loc, conf, g = loc.cpu().numpy().copy(), conf.cpu().numpy().copy(), g.cpu().numpy().copy()
    assert np.isfinite(g).all() and np.isfinite(loc).all() and np.isfinite(conf).all()
    probs = m.train_fetch("probs", B).reshape(B, -1, hp["total_labels"])
    deltas = m.train_fetch("deltas", B).reshape(B, -1, 4)
    assert probs.shape[1] == 2268
    np.testing.assert_allclose(probs.sum(-1), 1.0, atol=1e-5)
    np.testing.assert_allclose(loc, lo.loc_loss_fn(yd, deltas), rtol=1e-5, atol=1e-7)
    rconf = lo.conf_loss_fn(yl, probs, hp["neg_pos_ratio"])
    np.testing.assert_allclose(conf, rconf, rtol=2e-5, atol=1e-6)
    # training-mode BatchNorm uses the statistics of the WHOLE batch: Conv1's output (before BN) has
    # per-channel batch mean / biased variance that the moving averages must have moved towards
    after = m.get_weights()
    mom = 0.999
    c1 = m.train_fetch("Conv1_relu", B)            # post BN + ReLU6: only sanity of the shape here
    assert c1.size == B * 150 * 150 * 32
    mm = (after["bn_Conv1/moving_mean"] - mom * w["bn_Conv1/moving_mean"]) / (1 - mom)      # = batch mean
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    k = torch.from_numpy(w["Conv1/kernel"]).permute(3, 2, 0, 1)
    y = F.conv2d(F.pad(xt, (0, 1, 0, 1)), k, stride=2)             # TF SAME for 300 -> 150, k 3, s 2: pad (0, 1)
    np.testing.assert_allclose(mm, y.mean((0, 2, 3)).numpy(), rtol=2e-3, atol=2e-5)
    # bitwise repeatable
    m.set_weights(w)
    loc_b, conf_b, g_b = m.forward_backward(x, yd, yl)
    np.testing.assert_array_equal(g_b.cpu().numpy(), g)
    np.testing.assert_array_equal(loc_b.cpu().numpy(), loc)
    # three optimiser steps on the same batch reduce its loss
    first = float((loc + conf).mean())
    for _ in range(3):
        m.apply_gradients(m._grads, learning_rate=LR)
        l2, c2, _ = m.forward_backward(x, yd, yl)
    assert float((l2 + c2).mean()) < first


@pytest.mark.gpu
@pytest.mark.parametrize("backbone", ["mobilenet_v2", "vgg16"])
def test_gradient_bucket_events(backbone):
    """Bucket-as-ready exchange, device side (``ssd_net_train_set_buckets`` / ``ssd_net_train_wait_bucket``): a
    second stream that waits for bucket k's completion event and copies the bucket out right away must see the
    FINAL gradients of that bucket -- the flat vector starts NaN-filled, so an event recorded before the last
    kernel that writes into the bucket (weight gradients, BatchNorm / bias reductions, VGG16's l2 term) would
    leak NaN or partial sums into the snapshot -- and the result equals the un-bucketed step bit for bit."""
    import torch
    import ssd_hip as h
    if backbone == "mobilenet_v2":
        from models.ssd_mobilenet_v2 import get_model
    else:
        from models.ssd_vgg16 import get_model
    hp = helpers.hyper_params(backbone)
    w = helpers.synthetic_weights(backbone, hp)
    B = 2
    x = helpers.images(B, 300, seed=31)
    yd, yl = _targets(hp, B, seed=6)
    m = get_model(hp)
    m.set_weights(w)
    m.compile()
    _, _, g0 = m.forward_backward(x, yd, yl)
    g0 = g0.cpu().numpy().copy()
    starts = m._plan_gradient_buckets(B, 5)
    assert starts[0] == 0 and len(starts) == 5
    side = h.new_stream()
    m._grads.fill_(float("nan"))
    snap = torch.full_like(m._grads, float("nan"))
    torch.cuda.synchronize()
    loc, conf, g = m.forward_backward(x, yd, yl)
    bounds = list(starts) + [g.numel()]
    for k in reversed(range(len(starts))):
        h.check(h.lib().ssd_net_train_wait_bucket(m._net, k, h.vp(side.cuda_stream)), "wait_bucket")
        with torch.cuda.stream(side):
            snap[bounds[k]:bounds[k + 1]].copy_(g[bounds[k]:bounds[k + 1]], non_blocking=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g.cpu().numpy(), g0)                 # the bucket plan does not change the arithmetic
    np.testing.assert_array_equal(snap.cpu().numpy(), g0)              # every bucket was final at its event
    with pytest.raises(ValueError):
        arr = (ctypes.c_long * 2)(0, 0)
        h.check(h.lib().ssd_net_train_set_buckets(m._net, 2, arr), "set_buckets")


@pytest.mark.gpu
def test_train_step_vgg16_matches_autograd_oracle():
    """The same check on the VGG16 graph (bias + ReLU convs incl. dilation 6 / VALID / stride 2,
    SAME max-pools incl. the overlapping 3x3 stride-1 pool5, L2Normalization with its learnable
    scale, l2(5e-4) kernel regulariser)."""
    import torch
    from models.ssd_vgg16 import get_model
    from oracle import train_oracle as to
    from ssd_loss import CustomLoss
    hp = helpers.hyper_params("vgg16")
    w = {k: v.copy() for k, v in helpers.synthetic_weights("vgg16", hp).items()}
    B = 2
    x = helpers.images(B, 300, seed=23)
    yd, yl = _targets(hp, B, seed=4)
    m = get_model(hp)
    m.set_weights(w)
    cl = CustomLoss(hp["neg_pos_ratio"], hp["loc_loss_alpha"])
    m.compile(loss=[cl.loc_loss_fn, cl.conf_loss_fn])
    loc, conf, g = m.forward_backward(x, yd, yl)
    loc, conf, g = loc.cpu().numpy(), conf.cpu().numpy(), g.cpu().numpy().copy()
    probs = m.train_fetch("probs", B).reshape(B, -1, hp["total_labels"])
    cl.conf_loss_fn(yl, probs)
    fm = cl.last_final_mask.cpu().numpy()
    masks = []
    for name in to.act_names("vgg16"):
        a = m.train_fetch(name, B)
        masks.append((a > 0).reshape(B, *_hwc(m, name)))
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref = to.train_step("vgg16", hp, w, x, yd, yl, 3.0, 1.0, final_mask=fm, act_masks=masks)
    assert np.abs(probs - ref["probs"]).max() <= 1e-4
    np.testing.assert_allclose(loc, ref["loc"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(conf, ref["conf"], rtol=1e-4, atol=1e-6)
    offs = m.trainable_offsets()
    assert set(offs) == set(ref["grads"])
    errs = []
    for name, (off, shape) in offs.items():
        got = g[off:off + int(np.prod(shape))].reshape(shape)
        rg = ref["grads"][name]
        scale = max(float(np.abs(rg).max()), 1e-2)
        errs.append((float(np.abs(got - rg).max()) / scale, name, scale))
    for e in sorted(errs)[-6:]:
        print("grad %-42s err %.2e of max(|g|max, 1e-2) = %.3e" % (e[1], e[0], e[2]))
    # (a max-pool arg-max that flips between two nearly equal activations moves single entries;
    # the bulk criterion is the L2 norm, the max-norm bound is looser than for MobileNetV2)
    for name, (off, shape) in offs.items():
        got = g[off:off + int(np.prod(shape))].reshape(shape)
        rg = ref["grads"][name]
        assert np.linalg.norm(got - rg) <= 2e-3 * np.linalg.norm(rg) + 1e-6, name
    assert max(errs)[0] <= 2e-2, max(errs)
    # Keras adds sum(model.losses) = 5e-4 * sum(kernel^2) over the regularised convs to `loss` / `val_loss`
    reg = sum(5e-4 * float((np.asarray(v, np.float64) ** 2).sum()) for k, v in w.items()
              if k.endswith("/kernel") and not k[0].isdigit())
    assert reg > 0 and abs(m.regularization_loss() - reg) <= 1e-5 * reg
    tot, lm, cm = m.evaluate_on_batch(x, (yd, yl))
    assert abs(tot - (lm + cm + reg)) <= 1e-5 * tot
    m.apply_gradients(m._grads, learning_rate=LR)
    loc2, conf2, _ = m.forward_backward(x, yd, yl)
    assert float((loc2 + conf2).mean()) < float((loc + conf).mean())


@pytest.mark.gpu
def test_trainer_entry_point_fit(tmp_path, monkeypatch, capsys):
    """trainer.py: fit loop with LR schedule, validation, best-val_loss checkpoint (reference
    trainer.py:57-76) on a few synthetic steps; the checkpoint is a Keras-layout HDF5 file the
    predictor-side loader reads back."""
    import importlib
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_TRAINER_EPOCHS", "2")
    monkeypatch.setenv("SSD_TRAINER_STEPS", "3")
    monkeypatch.setenv("SSD_TRAINER_BATCH", "4")
    monkeypatch.setenv("SSD_TRAINER_AUGMENT", "0")        # (the loss comparison below wants the same batches in both epochs)
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "Epoch 1/2" in out and "Epoch 2/2" in out and "val_loss" in out
    assert len(hist["loss"]) == 2 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
    assert hist["loss"][1] < hist["loss"][0]
    path = os.path.join("trained", "ssd_mobilenet_v2_model_weights.h5")
    assert os.path.exists(path)
    from utils import h5_reader
    w = h5_reader.load_keras_weights(path)
    assert "bn_Conv1/moving_mean" in w and w["Conv1/kernel"].shape == (3, 3, 3, 32)
    # the predictor entry point picks the trained checkpoint up (reference predictor.py:45-46)
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "8")
    predictor = importlib.import_module("predictor")
    b, l, s = predictor.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "no trained weights" not in out and b.shape == (8, 200, 4) and np.isfinite(s).all()
