"""The focal loss on the device (csrc/ssd_focal.hip, ``ssd_loss.FocalLoss``) against the oracle of tests/focal_cases.py,
its bit properties, and its way into the training step, ``evaluate_on_batch``, ``set_conf_prior`` and ``trainer.main``.

Bars: the ones the mining kernel is held to -- losses and per-anchor values rtol 1e-5, atol 1e-7 (tests/test_loss.py),
gradients 1e-6 absolute (tests/test_loss_edges_gpu.py).  They were not widened: a plain float32 NumPy restatement of the
formula lies within 8.7e-8 (gradients) and 7.2e-8 relative (losses) of the float64 oracle on these cases
(tests/test_focal_cpu.py::test_what_float32_costs_on_the_cases prints the figures), so 4x that stays inside them.

Measured on an MI355X (gfx950), worst over a case (the largest gradient entry of a case lies between 4.7e-3 and 0.50):
  case (B x N x L, gamma, alpha)               |f / oracle - 1|   |conf / oracle - 1|   |grad_logits - autograd|   |grad_deltas - autograd|
  tiny               (1 x 1 x 2, 0, 1)         2.8e-08            2.8e-08               2.0e-09                    1.5e-08
  small              (2 x 70 x 3, 0.5, 1)      1.5e-07            6.0e-08               8.7e-08                    4.4e-10
  tile_plus_one      (3 x 257 x 21, 2, 0.25)   4.5e-07            7.1e-08               1.4e-09                    1.9e-09
  two_tiles_plus_one (2 x 513 x 21, 5, 0.25)   3.8e-07            5.2e-08               3.3e-09                    2.5e-09
  long_rows          (2 x 65 x 130, 2, 0.25)   1.9e-07            3.3e-08               5.4e-09                    2.5e-09
At gamma 0, alpha 1 the per-anchor value equals the mining kernel's cross-entropy bit for bit on tile_plus_one (the bar is
the loss bar).
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import focal_cases as fc
import helpers

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(name):
    """One case through FocalLoss: the three entry points, computed once, shared by the tests, left unchanged."""
    if name not in _RUNS:
        from ssd_loss import FocalLoss
        c = fc.cases()[name]
        fl = FocalLoss(c.loc_alpha, c.alpha, c.gamma)
        r = dict(conf=fl.conf_loss_fn(c.yl, c.pp).cpu().numpy(), ce=fl.last_cross_entropy.cpu().numpy(),
                 fm=fl.last_final_mask.cpu().numpy(), loc=fl.loc_loss_fn(c.yd, c.pd).cpu().numpy())
        loc, conf, gd, gz = fl.loss_and_grads(c.yd, c.yl, c.pd, c.pp)
        r.update(loc2=loc.cpu().numpy(), conf2=conf.cpu().numpy(), gd=gd.cpu().numpy(), gz=gz.cpu().numpy())
        for v in r.values():
            v.setflags(write=False)
        _RUNS[name] = r
    return _RUNS[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(fc.cases()))
def test_kernel_matches_oracle(name):
    c, o, r = fc.cases()[name], fc.oracle(name), _run(name)
    print("%s: |f - oracle| rel %.1e  conf rel %.1e  |grad_logits| %.1e  |grad_deltas| %.1e" % (
        name, np.abs(r["ce"] / o["f"] - 1).max(), np.abs(r["conf2"] / o["conf"] - 1).max(), np.abs(r["gz"] - o["gz"]).max(),
        np.abs(r["gd"] - o["gd"]).max()))
    assert r["fm"].shape == c.yl.shape[:2] and (r["fm"] == 1).all()                  # no mining: the final mask is all ones
    np.testing.assert_allclose(r["ce"], o["f"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r["conf2"], o["conf"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r["loc2"], o["loc"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r["conf2"], o["conf64"], rtol=1e-5, atol=1e-7)
    assert np.abs(r["gz"] - o["gz"]).max() <= 1e-6 and np.abs(r["gd"] - o["gd"]).max() <= 1e-6
    assert np.isfinite(r["gz"]).all() and np.abs(r["gz"]).max() > 1e-4
    if name == "small":
        assert not r["gz"][c.marks["below"]].any() and not r["gz"][c.marks["above"]].any()     # both clip bounds: exactly 0
        assert np.abs(r["gz"][c.marks["at_bound"]]).min() > 1e-4                               # exactly 1e-7f is inside
        assert not r["gd"][0].any()                                                            # no positive: no loc gradient


@pytest.mark.parametrize("name", list(fc.cases()))
def test_terms_alone_and_together_and_twice_give_the_same_bits(name):
    from ssd_loss import FocalLoss
    c, r = fc.cases()[name], _run(name)
    np.testing.assert_array_equal(_bits(r["conf"]), _bits(r["conf2"]))
    np.testing.assert_array_equal(_bits(r["loc"]), _bits(r["loc2"]))
    fl = FocalLoss(c.loc_alpha, c.alpha, c.gamma)
    yd, pd = fl._pair(c.yd, c.pd, 4)
    yl, pp = fl._pair(c.yl, c.pp, 0)
    _, _, _, _, gd_only, _ = fl._run(yd, pd, None, None, want_grads=True, grad_scale=1.0 / c.yl.shape[0])
    _, _, ce, _, _, gz_only = fl._run(None, None, yl, pp, want_aux=True, want_grads=True, grad_scale=1.0 / c.yl.shape[0])
    np.testing.assert_array_equal(_bits(gd_only.cpu().numpy()), _bits(r["gd"]))
    np.testing.assert_array_equal(_bits(gz_only.cpu().numpy()), _bits(r["gz"]))
    np.testing.assert_array_equal(_bits(ce.cpu().numpy()), _bits(r["ce"]))
    loc, conf, gd, gz = fl.loss_and_grads(c.yd, c.yl, c.pd, c.pp)                               # and a second run
    for got, key in ((loc, "loc2"), (conf, "conf2"), (gd, "gd"), (gz, "gz")):
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(r[key]))


@pytest.mark.parametrize("name", ["small", "two_tiles_plus_one", "long_rows"])
def test_grad_scale_is_an_exact_factor(name):
    """B = 2: the gradients at grad_scale 1 / B are, bit for bit, the gradients at grad_scale 1 times 1 / B."""
    from ssd_loss import FocalLoss
    c, r = fc.cases()[name], _run(name)
    assert c.yl.shape[0] == 2
    _, _, gd, gz = FocalLoss(c.loc_alpha, c.alpha, c.gamma).loss_and_grads(c.yd, c.yl, c.pd, c.pp, grad_scale=1.0)
    np.testing.assert_array_equal(_bits(gz.cpu().numpy() * np.float32(0.5)), _bits(r["gz"]))
    np.testing.assert_array_equal(_bits(gd.cpu().numpy() * np.float32(0.5)), _bits(r["gd"]))


def test_gamma_zero_alpha_one_is_the_mining_kernels_cross_entropy():
    """ce_out of the mining kernel is untouched by its select: with every negative mined (ratio N) or none, it is the
    per-anchor cross-entropy, and the focal value at gamma 0, alpha 1 equals it."""
    from ssd_loss import CustomLoss, FocalLoss
    c = fc.cases()["tile_plus_one"]
    N = c.yl.shape[1]
    cl = CustomLoss(neg_pos_ratio=N, loc_loss_alpha=1.0)
    cl.conf_loss_fn(c.yl, c.pp)
    fl = FocalLoss(1.0, alpha=1.0, gamma=0.0)
    fl.conf_loss_fn(c.yl, c.pp)
    got, want = fl.last_cross_entropy.cpu().numpy(), cl.last_cross_entropy.cpu().numpy()
    print("gamma 0 / alpha 1 against the mining kernel's cross-entropy: worst |difference| %.1e" % np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------- the training step
def _targets(hp, B, seed=3):
    from oracle import bbox_oracle as bo
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=hp["total_labels"], seed=seed)
    return bo.calculate_actual_outputs(priors, gt, gl, hp)


def _step(m, B, x, yd, yl):
    loc, conf, g = m.forward_backward(x, yd, yl)
    return dict(loc=loc.cpu().numpy(), conf=conf.cpu().numpy(), g=g.cpu().numpy().copy(),
                gz=m.train_fetch("grad_logits", B), gd=m.train_fetch("grad_deltas", B),
                probs=m.train_fetch("probs", B), deltas=m.train_fetch("deltas", B))


@pytest.fixture(scope="module")
def wired():
    """MobileNetV2-SSD300 at B = 2, synthetic weights, no optimizer step anywhere: a fresh model's step with CustomLoss; on a
    clone a CustomLoss step, a FocalLoss step and a CustomLoss step again; the first model's CustomLoss step once more; then
    evaluate_on_batch under both losses and set_conf_prior on the clone."""
    from models._net import SSDModel
    from ssd_loss import CustomLoss, FocalLoss
    hp = helpers.hyper_params("mobilenet_v2")
    B = 2
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.images(B, 300, seed=5)
    yd, yl = _targets(hp, B)
    m = SSDModel("mobilenet_v2", hp, B)
    m.set_weights(w)
    hard, focal = CustomLoss(3, 1), FocalLoss(1.0, alpha=0.25, gamma=2.0)
    m.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out = dict(B=B, hp=hp, yd=yd, yl=yl, focal=focal, fresh=_step(m, B, x, yd, yl))
    c = m.clone()
    c.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out["clone_before"] = _step(c, B, x, yd, yl)
    c.compile(loss=[focal.loc_loss_fn, focal.conf_loss_fn])
    assert c._loss is focal
    out["clone_focal"] = _step(c, B, x, yd, yl)
    c.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out["clone_after"] = _step(c, B, x, yd, yl)
    out["again"] = _step(m, B, x, yd, yl)
    # evaluate_on_batch: the compiled loss on the inference forward
    d, p = m(x)
    m.compile(loss=[focal.loc_loss_fn, focal.conf_loss_fn])
    out["eval_focal"] = m.evaluate_on_batch(x, (yd, yl))
    out["eval_focal_want"] = (float(focal.loc_loss_fn(yd, d).mean().item()), float(focal.conf_loss_fn(yl, p).mean().item()))
    m.compile(loss=[hard.loc_loss_fn, hard.conf_loss_fn])
    out["eval_hard"] = m.evaluate_on_batch(x, (yd, yl))
    today = CustomLoss(3.0, 1.0)
    out["eval_hard_want"] = (float(today.loc_loss_fn(yd, d).mean().item()), float(today.conf_loss_fn(yl, p).mean().item()))
    # set_conf_prior
    out["w_before"] = c.get_weights()
    out["prior_names"] = c.set_conf_prior(0.01)
    out["w_after"] = c.get_weights()
    return out


def test_training_step_runs_the_compiled_focal_loss(wired):
    B, N, L = wired["B"], wired["yl"].shape[1], wired["yl"].shape[2]
    s = wired["clone_focal"]
    loc, conf, gd, gz = wired["focal"].loss_and_grads(wired["yd"], wired["yl"], s["deltas"].reshape(B, N, 4),
                                                      s["probs"].reshape(B, N, L))
    np.testing.assert_array_equal(_bits(s["gz"]), _bits(gz.cpu().numpy().ravel()))
    np.testing.assert_array_equal(_bits(s["gd"]), _bits(gd.cpu().numpy().ravel()))
    np.testing.assert_array_equal(_bits(s["loc"]), _bits(loc.cpu().numpy()))
    np.testing.assert_array_equal(_bits(s["conf"]), _bits(conf.cpu().numpy()))
    h = wired["clone_before"]
    np.testing.assert_array_equal(_bits(s["probs"]), _bits(h["probs"]))              # the same forward ...
    assert (s["gz"] != h["gz"]).mean() > 0.5 and (s["conf"] != h["conf"]).all()      # ... another loss
    assert (s["g"] != h["g"]).mean() > 0.5 and np.isfinite(s["g"]).all()
    assert (s["gz"] == 0).mean() < (h["gz"] == 0).mean()                             # mining drops anchors, focal none


def test_mining_path_is_unchanged_by_a_focal_step(wired):
    for other in ("clone_before", "clone_after", "again"):
        for key in ("loc", "conf", "g", "gz", "gd", "probs", "deltas"):
            np.testing.assert_array_equal(_bits(wired[other][key]), _bits(wired["fresh"][key]), err_msg="%s %s" % (other, key))


def test_evaluate_on_batch_uses_the_compiled_loss(wired):
    for kind in ("focal", "hard"):
        total, lm, cm = wired["eval_" + kind]
        want_l, want_c = wired["eval_%s_want" % kind]
        assert (lm, cm) == (want_l, want_c) and total == lm + cm          # MobileNetV2: no regularisation term
    assert wired["eval_focal"][2] != wired["eval_hard"][2]
    assert abs(wired["eval_focal"][1] - wired["eval_hard"][1]) <= 1e-5 * wired["eval_hard"][1]      # the same localisation term


def test_set_conf_prior_writes_every_label_bias_and_nothing_else(wired):
    from models.header import conf_prior_bias
    L = wired["hp"]["total_labels"]
    names = ["%d_conv_label_output/bias" % i for i in range(1, 7)]
    assert wired["prior_names"] == sorted(names)
    for name, before in wired["w_before"].items():
        after = wired["w_after"][name]
        if name in names:
            np.testing.assert_array_equal(after, conf_prior_bias(0.01, L, before.size // L))
            assert after.reshape(-1, L)[0, 0] == np.float32(np.log(0.99 * (L - 1) / 0.01))
        else:
            np.testing.assert_array_equal(_bits(after), _bits(before), err_msg=name)


def test_trainer_with_the_focal_loss(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    for k, v in (("LOSS", "focal"), ("EPOCHS", "1"), ("STEPS", "2"), ("BATCH", "2"), ("AUGMENT", "0"), ("FOCAL_PRIOR", "0.01")):
        monkeypatch.setenv("SSD_TRAINER_" + k, v)
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "loss: FocalLoss(loc_loss_alpha=1, alpha=0.25, gamma=2)" in out and "label heads: prior probability 0.01" in out
    for key in ("loss", "loc_loss", "conf_loss", "val_loss"):
        assert len(hist[key]) == 1 and np.isfinite(hist[key]).all() and hist[key][0] > 0, key
    assert os.path.exists(os.path.join("trained", "ssd_mobilenet_v2_model_weights.h5"))


# ---------------------------------------------------------------------------------------------- error paths
def test_bad_arguments_are_refused_before_any_launch():
    import ssd_hip as h
    lib = h.lib()
    c = fc.cases()["small"]
    B, N, L = c.yl.shape
    yd, pd, yl, pp = (h.to_dev(a) for a in (c.yd, c.pd, c.yl, c.pp))
    outs = [torch.full(s, -7.0, dtype=torch.float32, device=yd.device) for s in ((B,), (B,), (B, N), (B, N), (B, N, 4), (B, N, L))]
    need = lib.ssd_focal_loss_workspace_bytes(B, N, L)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=yd.device)

    def call(alpha=0.25, gamma=2.0, ws_bytes=need, deltas=pd, grad_deltas=outs[4]):
        return lib.ssd_focal_loss(h.ptr(yd), h.ptr(deltas), h.ptr(yl), h.ptr(pp), B, N, L, 1.0, alpha, gamma, h.ptr(outs[0]),
                                  h.ptr(outs[1]), h.ptr(outs[2]), h.ptr(outs[3]), h.ptr(grad_deltas), h.ptr(outs[5]), 0.5,
                                  h.ptr(ws), ws_bytes, h.stream())

    skewed = torch.zeros(B * N * 4 + 4, dtype=torch.float32, device=yd.device)[1:1 + B * N * 4].view(B, N, 4)
    assert skewed.data_ptr() % 16 == 4
    for kw in (dict(gamma=-0.5), dict(alpha=0.0), dict(alpha=-1.0), dict(gamma=float("nan")), dict(alpha=float("inf")),
               dict(ws_bytes=need - 1), dict(deltas=skewed), dict(grad_deltas=skewed)):
        assert call(**kw) == -1, kw                                   # SSD_E_INVALID
        assert lib.ssd_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert (o == -7.0).all()                                      # nothing was launched
    with pytest.raises(ValueError):
        h.check(call(gamma=-0.5), "ssd_focal_loss")
    assert call() == 0                                                # and the same buffers do go through
    torch.cuda.synchronize()
    assert all((o != -7.0).all() for o in outs)
    # the training step refuses an unknown kind and bad focal numbers the same way
    from models._net import SSDModel
    m = SSDModel("mobilenet_v2", helpers.hyper_params("mobilenet_v2"), 1)
    for cfg in (h.LossConfig(2, 3.0, 1.0, 0.25, 2.0), h.LossConfig(h.LOSS_FOCAL, 3.0, 1.0, 0.0, 2.0),
                h.LossConfig(h.LOSS_FOCAL, 3.0, 1.0, 0.25, -1.0)):
        assert lib.ssd_net_train_forward_backward_cfg(m._net, h.ptr(yd), 1, h.ptr(yd), h.ptr(yl), ctypes.byref(cfg), h.ptr(yd),
                                                      None, None, h.stream()) == -1
