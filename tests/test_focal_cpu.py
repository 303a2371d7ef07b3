"""The focal loss away from the GPU: the oracle of tests/focal_cases.py against values worked out by hand, against the
cross-entropy oracle at gamma 0 / alpha 1 and against central differences; what float32 arithmetic costs on the cases (the
figure a bar wider than the mining kernel's would have to come from); and the host side -- ``FocalLoss`` arguments,
``trainer.loss_from_env``, the prior-probability bias."""
import importlib
import math

import numpy as np
import pytest

import focal_cases as fc
from oracle import loss_oracle as lo


def test_three_anchors_by_hand():
    """alpha 0.25, gamma 2, L = 3.  Anchor 0: background target, r0 = 0.5 -> 0.25 * 0.25 * ln 2.  Anchor 1: class 2,
    r2 = 0.25 of an unnormalised row (0.5, 1, 0.5) -> 0.25 * 0.5625 * ln 4.  Anchor 2: class 1 at probability 0, clipped to
    1e-7f -> 0.25 * (1 - 1e-7f)^2 * -ln(1e-7f).  One positive count of 2 -> conf = sum / 2."""
    y = np.array([[[1, 0, 0], [0, 0, 1], [0, 1, 0]]], np.float32)
    q = np.array([[[0.5, 0.25, 0.25], [0.5, 1.0, 0.5], [0.75, 0.0, 0.25]]], np.float32)
    e = float(fc.EPS)
    want = [0.25 * 0.25 * math.log(2), 0.25 * 0.5625 * math.log(4), 0.25 * (1 - e) ** 2 * -math.log(e)]
    got = fc.per_anchor(y, q, 0.25, 2.0)
    np.testing.assert_allclose(got[0], want, rtol=1e-14)
    np.testing.assert_allclose(fc.conf_loss(y, q, 0.25, 2.0), [sum(want) / 2], rtol=1e-14)
    # no positive at all: the denominator is 1
    np.testing.assert_allclose(fc.conf_loss(y[:, :1], q[:, :1], 0.25, 2.0), [want[0]], rtol=1e-14)


@pytest.mark.parametrize("name", list(fc.cases()))
def test_gamma_zero_alpha_one_is_the_cross_entropy(name):
    c = fc.cases()[name]
    ce = lo.cross_entropy(c.yl, c.pp)
    np.testing.assert_allclose(fc.per_anchor(c.yl, c.pp, 1.0, 0.0), ce, rtol=2e-6, atol=2e-7)      # float32 sum of <= 21 logs


@pytest.mark.parametrize("gamma,alpha", [(0.0, 1.0), (0.5, 1.0), (2.0, 0.25), (5.0, 0.25)])
def test_oracle_gradients_against_central_differences(gamma, alpha):
    """float64 throughout, on the smallest shape (two anchors of two classes, away from the clip bounds)."""
    z = np.array([[[0.3, -0.7], [-1.1, 0.4]]], np.float64)
    yl = np.array([[[0, 1], [1, 0]]], np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    zero = np.zeros((1, 2, 4))
    _, _, _, gz = fc.torch_loss_and_grads(zero, yl, zero, p, 1.0, alpha, gamma, r_float32=False)
    h = 1e-6
    fd = np.zeros_like(z)
    for i in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        fd[i] = (fc.objective_from_logits(zp, yl, alpha, gamma) - fc.objective_from_logits(zm, yl, alpha, gamma)) / (2 * h)
    assert np.abs(gz).max() > 1e-3
    np.testing.assert_allclose(gz, fd, rtol=1e-7, atol=1e-9)


def test_cases_hold_what_they_promise():
    cs = fc.cases()
    T = fc.TILE_L21
    assert [c.yl.shape for c in cs.values()] == [(1, 1, 2), (2, 70, 3), (3, T + 1, 21), (2, 2 * T + 1, 21),
                                                  (2, 65, fc.STAGED_MAX_L + 11)]
    assert sorted(c.gamma for c in cs.values()) == [0.0, 0.5, 2.0, 2.0, 5.0] and {c.alpha for c in cs.values()} == {0.25, 1.0}
    o = fc.oracle("small")
    for mark in ("below", "above"):                                   # both clip bounds: the gradient row is exactly 0
        assert not o["gz"][cs["small"].marks[mark]].any()
    assert np.abs(o["gz"][cs["small"].marks["at_bound"]]).min() > 1e-4        # exactly 1e-7f lies inside
    t = cs["tile_plus_one"]
    assert ((t.yl[2] > 0) & (t.yl[2] < 1)).all() and fc.positives(t.yl[2]).all()
    import ssd_hip
    staged = ssd_hip.ctypes.c_int(-1)
    lib = ssd_hip.lib()
    assert lib.ssd_focal_loss_tile(21, ssd_hip.ctypes.byref(staged)) == T and staged.value == 1
    assert lib.ssd_focal_loss_tile(fc.STAGED_MAX_L, ssd_hip.ctypes.byref(staged)) == 64 and staged.value == 1
    assert lib.ssd_focal_loss_tile(fc.STAGED_MAX_L + 1, ssd_hip.ctypes.byref(staged)) == 256 and staged.value == 0
    assert lib.ssd_focal_loss_workspace_bytes(32, 2268, 21) == 32 * 9 * 16


def test_what_float32_costs_on_the_cases():
    """A plain float32 NumPy restatement of the formula against the float64 oracle, printed per case: the figure from which a
    bar above tests/test_loss.py's (losses rtol 1e-5, gradients 1e-6 absolute) would be derived at 4x.  Measured here: the
    worst gradient distance is 8.7e-8 (small, whose largest gradient entry is 0.50) and the worst relative loss distance
    7.2e-8 (long_rows), so the mining kernel's bars stand as they are."""
    worst_g = worst_l = 0.0
    for name, c in fc.cases().items():
        o = fc.oracle(name)
        f, conf, gz = fc.float32_restatement(c)
        dg = float(np.abs(gz - o["gz"]).max())
        dl = float(np.abs(conf / o["conf"] - 1).max())
        print("%-20s |grad - oracle| %.3e   conf relative %.3e   max |grad| %.3e" % (name, dg, dl, np.abs(o["gz"]).max()))
        worst_g, worst_l = max(worst_g, dg), max(worst_l, dl)
    assert worst_g <= 1e-6 / 4 and worst_l <= 1e-5 / 4


def test_focal_loss_arguments():
    from ssd_loss import CustomLoss, FocalLoss
    import ssd_hip
    fl = FocalLoss(1.5)
    assert fl.get_config() == {"loc_loss_alpha": 1.5, "alpha": 0.25, "gamma": 2.0}
    assert FocalLoss(1, alpha="0.5", gamma=0).get_config() == {"loc_loss_alpha": 1.0, "alpha": 0.5, "gamma": 0.0}
    n = fl.to_native()
    assert (n.kind, n.loc_loss_alpha, n.focal_alpha, n.focal_gamma) == (ssd_hip.LOSS_FOCAL, 1.5, 0.25, 2.0)
    m = CustomLoss(3, 1).to_native()
    assert (m.kind, m.neg_pos_ratio, m.loc_loss_alpha) == (ssd_hip.LOSS_HARD_NEGATIVE, 3.0, 1.0)
    assert fl.last_cross_entropy is None and fl.last_final_mask is None
    for kw in (dict(alpha=0), dict(alpha=-1), dict(gamma=-0.5), dict(alpha=float("nan")), dict(gamma=float("inf")),
               dict(alpha="x"), dict(gamma=None), dict(alpha=float("inf"))):
        with pytest.raises(ValueError):
            FocalLoss(1.0, **kw)
    with pytest.raises(ValueError):
        FocalLoss(-1.0)


def test_loss_from_env(monkeypatch):
    from ssd_loss import CustomLoss, FocalLoss
    trainer = importlib.import_module("trainer")
    hp = {"neg_pos_ratio": 3, "loc_loss_alpha": 1}
    for k in ("LOSS", "FOCAL_ALPHA", "FOCAL_GAMMA"):
        monkeypatch.delenv("SSD_TRAINER_" + k, raising=False)
    unset = trainer.loss_from_env(hp)
    assert type(unset) is CustomLoss and (unset.neg_pos_ratio, unset.loc_loss_alpha) == (3.0, 1.0)
    monkeypatch.setenv("SSD_TRAINER_LOSS", "hard")
    assert type(trainer.loss_from_env(hp)) is CustomLoss
    monkeypatch.setenv("SSD_TRAINER_LOSS", " Focal ")
    fl = trainer.loss_from_env(hp)
    assert type(fl) is FocalLoss and fl.get_config() == {"loc_loss_alpha": 1.0, "alpha": 0.25, "gamma": 2.0}
    monkeypatch.setenv("SSD_TRAINER_FOCAL_ALPHA", "0.5")
    monkeypatch.setenv("SSD_TRAINER_FOCAL_GAMMA", "1.5")
    assert trainer.loss_from_env(hp).get_config() == {"loc_loss_alpha": 1.0, "alpha": 0.5, "gamma": 1.5}
    monkeypatch.setenv("SSD_TRAINER_FOCAL_GAMMA", "-1")
    with pytest.raises(ValueError):
        trainer.loss_from_env(hp)
    monkeypatch.setenv("SSD_TRAINER_FOCAL_GAMMA", "two")
    with pytest.raises(ValueError):
        trainer.loss_from_env(hp)
    monkeypatch.setenv("SSD_TRAINER_FOCAL_GAMMA", "2")
    monkeypatch.setenv("SSD_TRAINER_LOSS", "hard")                    # a focal knob beside the mining loss
    with pytest.raises(ValueError):
        trainer.loss_from_env(hp)
    monkeypatch.setenv("SSD_TRAINER_LOSS", "dice")
    with pytest.raises(ValueError):
        trainer.loss_from_env(hp)


@pytest.mark.parametrize("L", [2, 21])
def test_conf_prior_bias(L):
    from models.header import conf_prior_bias
    pi, A = 0.01, 5
    b = conf_prior_bias(pi, L, A)
    assert b.shape == (A * L,) and b.dtype == np.float32
    b = b.reshape(A, L)
    np.testing.assert_allclose(b[:, 0], math.log((1 - pi) * (L - 1) / pi), rtol=1e-6)
    assert not b[:, 1:].any()
    p = np.exp(b.astype(np.float64))
    p /= p.sum(-1, keepdims=True)                                     # a zero kernel: softmax of the bias alone
    np.testing.assert_allclose(p[:, 0], 1 - pi, rtol=1e-6)
    np.testing.assert_allclose(p[:, 1:], pi / (L - 1), rtol=1e-5)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            conf_prior_bias(bad, L, A)
    with pytest.raises(ValueError):
        conf_prior_bias(0.01, 1, A)
