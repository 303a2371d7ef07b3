"""The IoU-family localisation losses on the device (csrc/ssd_iouloss.hip, ``ssd_loss.IoULocLoss``) against the float64
oracle of tests/iou_loss_cases.py, their bit properties, and their way into the training step, ``evaluate_on_batch`` and
``trainer.main``.

Bars: the ones the two other loss kernels are held to -- losses and per-anchor values rtol 1e-5, atol 1e-7, gradients 1e-6
absolute at the case's grad_scale 1 / B.  They were not widened: four times the worst distance of a plain float32
restatement from the oracle stays inside each of them (tests/test_iou_loss_cpu.py::test_what_float32_costs_on_the_cases
prints and asserts the figures).  The gradients are also held, relative to the case's largest oracle entry, to four times
the restatement's worst relative figure (6.11e-7: a bar of 2.4e-6 of the largest entry).  At the designated
anchors (prediction == target, a kink) only |l| <= 1e-6 and |grad| <= 1 are asserted; no other anchor is left out.

Measured on an MI355X (gfx950), worst over a case's four modes (the case's largest gradient entry in brackets):
  case (B x N)                    |l / oracle - 1|   |loc / oracle - 1|   |grad_deltas - autograd|   of the largest entry
  tiny               (1 x 1)      1.7e-07            1.7e-07              2.3e-08  (8.5e-02)         2.7e-07
  small              (2 x 70)     1.7e-06            2.0e-07              3.8e-09  (6.2e-03)         6.1e-07
  tile_plus_one      (3 x 257)    2.4e-06            1.0e-07              1.8e-09  (4.8e-03)         3.8e-07
  two_tiles_plus_one (2 x 513)    2.4e-06            6.3e-08              8.5e-10  (2.2e-03)         3.8e-07
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import helpers
import iou_loss_cases as ic

pytestmark = pytest.mark.gpu

_RUNS = {}


def _loss(c, mode, base=None):
    from ssd_loss import CustomLoss, IoULocLoss
    return IoULocLoss(base or CustomLoss(3, c.loc_alpha), c.priors, c.var, mode)


def _run(name, mode):
    """One case and mode through IoULocLoss: ``loc_loss_fn`` and ``loss_and_grads``, computed once, shared, left unchanged."""
    if (name, mode) not in _RUNS:
        c = ic.cases()[name]
        il = _loss(c, mode)
        yl, pp = _labels(c)
        r = dict(loc=il.loc_loss_fn(c.yd, c.pd).cpu().numpy(), l=il.last_box_loss.cpu().numpy())
        loc, conf, gd, gz = il.loss_and_grads(c.yd, yl, c.pd, pp)
        r.update(loc2=loc.cpu().numpy(), conf2=conf.cpu().numpy(), gd=gd.cpu().numpy(), gz=gz.cpu().numpy())
        for v in r.values():
            v.setflags(write=False)
        _RUNS[(name, mode)] = r
    return _RUNS[(name, mode)]


_LABELS = {}


def _labels(c, L=21):
    """Seeded labels and probabilities [B,N,L] beside a case's deltas: one-hot, a class where the anchor is positive."""
    if c.name not in _LABELS:
        rng = np.random.default_rng(31)
        B, N = c.yd.shape[:2]
        pos = ic.positives(c.yd)
        yl = np.zeros((B, N, L), np.float32)
        yl[..., 0] = 1
        bi, ni = np.nonzero(pos)
        yl[bi, ni, 0] = 0
        yl[bi, ni, rng.integers(1, L, len(bi))] = 1
        z = (rng.standard_normal((B, N, L)) * 2).astype(np.float32)
        e = np.exp(z - z.max(-1, keepdims=True))
        _LABELS[c.name] = (yl, (e / e.sum(-1, keepdims=True)).astype(np.float32))
    return _LABELS[c.name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("mode", ic.MODES)
@pytest.mark.parametrize("name", list(ic.cases()))
def test_kernel_matches_oracle(name, mode):
    c, o, r = ic.cases()[name], ic.oracle(name, mode), _run(name, mode)
    pos, m = ic.positives(c.yd), ic.compared(c)
    big = np.abs(o["gd"]).max()
    keep = pos & m
    print("%s %s: per-anchor rel %.1e  loc rel %.1e  |grad - oracle| %.1e = %.1e of the largest entry %.1e" % (
        name, mode, np.abs(r["l"][keep] / o["l"][keep] - 1).max() if keep.any() else 0.0,
        np.abs(r["loc2"][o["loc"] != 0] / o["loc"][o["loc"] != 0] - 1).max(), np.abs(r["gd"] - o["gd"])[m].max(),
        np.abs(r["gd"] - o["gd"])[m].max() / big, big))
    np.testing.assert_allclose(r["l"][m], o["l"][m], rtol=ic.LOSS_RTOL, atol=ic.LOSS_ATOL)
    np.testing.assert_allclose(r["loc2"], o["loc"], rtol=ic.LOSS_RTOL, atol=ic.LOSS_ATOL)
    assert np.abs(r["gd"] - o["gd"])[m].max() <= ic.GRAD_ATOL
    assert np.abs(r["gd"] - o["gd"])[m].max() <= 4 * ic.restatement_figures()["grel"] * big
    assert np.isfinite(r["gd"]).all() and np.abs(r["gd"]).max() > 1e-4
    for at in c.marks["equal"]:
        assert abs(r["l"][at]) <= 1e-6 and np.abs(r["gd"][at]).max() <= 1, at
    assert not _bits(r["gd"])[~pos].any() and not _bits(r["l"])[~pos].any()       # exactly +0.0f where the anchor is not positive
    if name == "small":
        assert not _bits(r["gd"][0]).any() and r["loc2"][0] == 0                  # the image without a positive


@pytest.mark.parametrize("mode", ic.MODES)
@pytest.mark.parametrize("name", list(ic.cases()))
def test_alone_and_together_and_twice_give_the_same_bits(name, mode):
    c, r = ic.cases()[name], _run(name, mode)
    np.testing.assert_array_equal(_bits(r["loc"]), _bits(r["loc2"]))
    il = _loss(c, mode)
    yl, pp = _labels(c)
    loc, conf, gd, gz = il.loss_and_grads(c.yd, yl, c.pd, pp)                      # a second run, another object
    for got, key in ((loc, "loc2"), (conf, "conf2"), (gd, "gd"), (gz, "gz")):
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(r[key]))
    np.testing.assert_array_equal(_bits(il.loc_loss_fn(c.yd, c.pd).cpu().numpy()), _bits(r["loc"]))
    np.testing.assert_array_equal(_bits(il.last_box_loss.cpu().numpy()), _bits(r["l"]))


@pytest.mark.parametrize("mode", ic.MODES)
@pytest.mark.parametrize("name", ["small", "two_tiles_plus_one"])
def test_grad_scale_is_an_exact_factor(name, mode):
    """B = 2: the gradients at grad_scale 1 / B are, bit for bit, the gradients at grad_scale 1 times 1 / B."""
    c, r = ic.cases()[name], _run(name, mode)
    assert c.yd.shape[0] == 2
    yl, pp = _labels(c)
    _, _, gd, _ = _loss(c, mode).loss_and_grads(c.yd, yl, c.pd, pp, grad_scale=1.0)
    np.testing.assert_array_equal(_bits(gd.cpu().numpy() * np.float32(0.5)), _bits(r["gd"]))


@pytest.mark.parametrize("kind", ["hard", "focal"])
def test_the_confidence_term_is_the_bases(kind):
    from ssd_loss import CustomLoss, FocalLoss
    c = ic.cases()["two_tiles_plus_one"]
    yl, pp = _labels(c)
    make = (lambda: CustomLoss(3, c.loc_alpha)) if kind == "hard" else (lambda: FocalLoss(c.loc_alpha, 0.25, 2.0))
    base = make()
    _, conf, _, gz = base.loss_and_grads(c.yd, yl, c.pd, pp)
    il = _loss(c, "ciou", base=make())
    _, conf2, gd2, gz2 = il.loss_and_grads(c.yd, yl, c.pd, pp)
    np.testing.assert_array_equal(_bits(conf2.cpu().numpy()), _bits(conf.cpu().numpy()))
    np.testing.assert_array_equal(_bits(gz2.cpu().numpy()), _bits(gz.cpu().numpy()))
    np.testing.assert_array_equal(_bits(gd2.cpu().numpy()), _bits(_run(c.name, "ciou")["gd"]))     # whatever the base
    np.testing.assert_array_equal(_bits(il.conf_loss_fn(yl, pp).cpu().numpy()), _bits(base.conf_loss_fn(yl, pp).cpu().numpy()))
    np.testing.assert_array_equal(_bits(il.last_cross_entropy.cpu().numpy()), _bits(base.last_cross_entropy.cpu().numpy()))
    np.testing.assert_array_equal(_bits(il.last_final_mask.cpu().numpy()), _bits(base.last_final_mask.cpu().numpy()))


# ---------------------------------------------------------------------------------------------- the training step
def _targets(hp, B, seed=3):
    from oracle import bbox_oracle as bo
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=hp["total_labels"], seed=seed)
    return (priors,) + tuple(bo.calculate_actual_outputs(priors, gt, gl, hp))


def _step(m, B, x, yd, yl):
    loc, conf, g = m.forward_backward(x, yd, yl)
    return dict(loc=loc.cpu().numpy(), conf=conf.cpu().numpy(), g=g.cpu().numpy().copy(),
                gz=m.train_fetch("grad_logits", B), gd=m.train_fetch("grad_deltas", B),
                probs=m.train_fetch("probs", B), deltas=m.train_fetch("deltas", B))


@pytest.fixture(scope="module")
def wired():
    """MobileNetV2-SSD300 at B = 2, synthetic weights, no optimizer step anywhere: a fresh model's Huber step under the mining
    loss; on a clone a Huber step, a CIoU step, a Huber step under the focal loss, a CIoU step over it, and the first Huber
    step again; the first model's step once more; then evaluate_on_batch under a compiled IoULocLoss."""
    from models._net import SSDModel
    from ssd_loss import CustomLoss, FocalLoss, IoULocLoss
    hp = helpers.hyper_params("mobilenet_v2")
    B = 2
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.images(B, 300, seed=5)
    priors, yd, yl = _targets(hp, B)
    m = SSDModel("mobilenet_v2", hp, B)
    m.set_weights(w)
    hard, focal = CustomLoss(3, 1), FocalLoss(1.0, alpha=0.25, gamma=2.0)
    ciou_hard = IoULocLoss(hard, priors, hp["variances"], "ciou")
    ciou_focal = IoULocLoss(focal, priors, hp["variances"], "ciou")
    m.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out = dict(B=B, hp=hp, yd=yd, yl=yl, ciou_hard=ciou_hard, ciou_focal=ciou_focal, fresh=_step(m, B, x, yd, yl))
    c = m.clone()
    c.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out["clone_before"] = _step(c, B, x, yd, yl)
    out["offsets"] = c.trainable_offsets()
    c.compile(loss=[ciou_hard.loc_loss_fn, ciou_hard.conf_loss_fn])
    assert c._loss is ciou_hard
    out["clone_ciou_hard"] = _step(c, B, x, yd, yl)
    c.compile(loss=[focal.loc_loss_fn, focal.conf_loss_fn])
    out["clone_focal"] = _step(c, B, x, yd, yl)
    c.compile(loss=[ciou_focal.loc_loss_fn, ciou_focal.conf_loss_fn])
    assert c._loss is ciou_focal
    out["clone_ciou_focal"] = _step(c, B, x, yd, yl)
    c.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out["clone_after"] = _step(c, B, x, yd, yl)
    out["again"] = _step(m, B, x, yd, yl)
    d, p = m(x)
    m.compile(loss=[ciou_hard.loc_loss_fn, ciou_hard.conf_loss_fn])
    out["eval"] = m.evaluate_on_batch(x, (yd, yl))
    out["eval_want"] = (float(ciou_hard.loc_loss_fn(yd, d).mean().item()), float(ciou_hard.conf_loss_fn(yl, p).mean().item()))
    out["eval_huber"] = float(hard.loc_loss_fn(yd, d).mean().item())
    with pytest.raises(ValueError):
        m.compile(loss=[ciou_hard.loc_loss_fn, ciou_hard.conf_loss_fn], neg_pos_ratio=3)
    with pytest.raises(ValueError):
        m.compile(loss=[ciou_hard.loc_loss_fn, ciou_hard.conf_loss_fn], loc_loss_alpha=1)
    return out


@pytest.mark.parametrize("over", ["hard", "focal"])
def test_training_step_runs_the_compiled_iou_loss(wired, over):
    B, N, L = wired["B"], wired["yl"].shape[1], wired["yl"].shape[2]
    s, h = wired["clone_ciou_" + over], wired["clone_before" if over == "hard" else "clone_focal"]
    for key in ("probs", "deltas", "gz", "conf"):                                    # the same forward, the same confidence term
        np.testing.assert_array_equal(_bits(s[key]), _bits(h[key]), err_msg=key)
    loc, conf, gd, gz = wired["ciou_" + over].loss_and_grads(wired["yd"], wired["yl"], s["deltas"].reshape(B, N, 4),
                                                             s["probs"].reshape(B, N, L))
    np.testing.assert_array_equal(_bits(s["gd"]), _bits(gd.cpu().numpy().ravel()))
    np.testing.assert_array_equal(_bits(s["loc"]), _bits(loc.cpu().numpy()))
    np.testing.assert_array_equal(_bits(s["gz"]), _bits(gz.cpu().numpy().ravel()))
    np.testing.assert_array_equal(_bits(s["conf"]), _bits(conf.cpu().numpy()))
    pos = np.repeat(ic.positives(wired["yd"]).ravel(), 4)
    assert pos.sum() >= 40 and (s["gd"][pos] != h["gd"][pos]).mean() > 0.9           # another localisation gradient ...
    assert not _bits(s["gd"])[~pos].any() and (s["loc"] != h["loc"]).all()
    # ... that reaches the parameters: the box heads and what lies below them; a label head's own gradient comes from the
    # logits alone and keeps its bits
    assert np.isfinite(s["g"]).all()
    heads = 0
    for name, (off, shape) in wired["offsets"].items():
        a, b = s["g"][off:off + int(np.prod(shape))], h["g"][off:off + int(np.prod(shape))]
        if "_conv_label_output/" in name:
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=name)
        elif "_conv_boxes_output/" in name:
            reached = (a != 0) | (b != 0)                       # (only the channels of anchors that are positive somewhere)
            heads += int(reached.any())
            assert not reached.any() or (a[reached] != b[reached]).mean() > 0.9, name
    assert heads >= 2
    assert (s["g"] != h["g"]).mean() > 0.25


def test_huber_path_is_unchanged_by_an_iou_step(wired):
    for other in ("clone_before", "clone_after", "again"):
        for key in ("loc", "conf", "g", "gz", "gd", "probs", "deltas"):
            np.testing.assert_array_equal(_bits(wired[other][key]), _bits(wired["fresh"][key]), err_msg="%s %s" % (other, key))


def test_evaluate_on_batch_uses_the_compiled_loss(wired):
    total, lm, cm = wired["eval"]
    assert (lm, cm) == wired["eval_want"] and total == lm + cm            # MobileNetV2: no regularisation term
    assert np.isfinite(lm) and lm > 0 and lm != wired["eval_huber"]


def test_trainer_with_the_giou_loss(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    for k in ("LOSS", "FOCAL_ALPHA", "FOCAL_GAMMA", "FOCAL_PRIOR"):
        monkeypatch.delenv("SSD_TRAINER_" + k, raising=False)
    for k, v in (("LOC_LOSS", "giou"), ("EPOCHS", "1"), ("STEPS", "2"), ("BATCH", "2"), ("AUGMENT", "0")):
        monkeypatch.setenv("SSD_TRAINER_" + k, v)
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "loss: IoULocLoss(CustomLoss(neg_pos_ratio=3, loc_loss_alpha=1), priors=2268, variances=[0.1, 0.1, 0.2, 0.2], mode=giou)" in out
    for key in ("loss", "loc_loss", "conf_loss", "val_loss"):
        assert len(hist[key]) == 1 and np.isfinite(hist[key]).all() and hist[key][0] > 0, key
    assert os.path.exists(os.path.join("trained", "ssd_mobilenet_v2_model_weights.h5"))


# ---------------------------------------------------------------------------------------------- error paths
def test_bad_arguments_are_refused_before_any_launch():
    import ssd_hip as h
    lib = h.lib()
    c = ic.cases()["small"]
    B, N = c.yd.shape[:2]
    priors, yd, pd = (h.to_dev(a) for a in (c.priors, c.yd, c.pd))
    outs = [torch.full(s, -7.0, dtype=torch.float32, device=yd.device) for s in ((B,), (B, N), (B, N, 4))]
    need = lib.ssd_iou_loc_loss_workspace_bytes(B, N)
    assert need >= B * 8
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=yd.device)
    good = (ctypes.c_float * 4)(*[float(v) for v in c.var])

    def var(*v):
        return (ctypes.c_float * 4)(*v)

    def call(priors=priors, variances=good, actual=yd, pred=pd, B=B, N=N, mode=h.LOC_CIOU, grad=outs[2], ws_bytes=need):
        return lib.ssd_iou_loc_loss(h.ptr(priors), variances, h.ptr(actual), h.ptr(pred), B, N, mode, 1.0, h.ptr(outs[0]),
                                    h.ptr(outs[1]), h.ptr(grad), 0.5, h.ptr(ws), ws_bytes, h.stream())

    def skewed(n, shape):
        t = torch.zeros(n + 4, dtype=torch.float32, device=yd.device)[1:1 + n].view(shape)
        assert t.data_ptr() % 16 == 4
        return t

    for kw in (dict(N=0), dict(B=-1), dict(mode=0), dict(mode=5), dict(mode=-1), dict(variances=None),
               dict(variances=var(0.1, 0.1, 0.0, 0.2)), dict(variances=var(-0.1, 0.1, 0.2, 0.2)),
               dict(variances=var(0.1, float("nan"), 0.2, 0.2)), dict(variances=var(0.1, 0.1, 0.2, float("inf"))),
               dict(priors=None), dict(actual=None), dict(pred=None), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(priors=skewed(N * 4, (N, 4))), dict(actual=skewed(B * N * 4, (B, N, 4))),
               dict(pred=skewed(B * N * 4, (B, N, 4))), dict(grad=skewed(B * N * 4, (B, N, 4)))):
        assert call(**kw) == -1, kw                                   # SSD_E_INVALID
        assert lib.ssd_last_error(), kw
    assert call(B=0) == 0                                             # nothing to do: SSD_OK, nothing written
    torch.cuda.synchronize()
    for o in outs:
        assert (o == -7.0).all()                                      # nothing was launched
    with pytest.raises(ValueError):
        h.check(call(mode=7), "ssd_iou_loc_loss")
    assert call() == 0                                                # and the same buffers do go through
    torch.cuda.synchronize()
    assert all((o != -7.0).all() for o in outs)
    # the training step refuses an unknown loc_kind, and a loc_kind without priors or with bad variances, the same way
    from models._net import SSDModel
    from ssd_loss import CustomLoss, IoULocLoss
    m = SSDModel("mobilenet_v2", helpers.hyper_params("mobilenet_v2"), 1)
    il = IoULocLoss(CustomLoss(3, 1), c.priors, c.var, "ciou")
    ok = il.to_native()
    assert ok.priors_dev == il.priors_dev().data_ptr() and ok.loc_kind == h.LOC_CIOU
    unknown, no_priors, bad_var = (il.to_native() for _ in range(3))
    unknown.loc_kind = 5
    no_priors.priors_dev = None
    bad_var.variances[2] = 0.0
    for cfg in (unknown, no_priors, bad_var):
        assert lib.ssd_net_train_forward_backward_cfg(m._net, h.ptr(yd), 1, h.ptr(yd), h.ptr(yd), ctypes.byref(cfg), h.ptr(yd),
                                                      None, None, h.stream()) == -1
        assert lib.ssd_last_error()
