"""The IoU-family localisation losses away from the GPU: the oracle of tests/iou_loss_cases.py against central differences
and against the relations between the four modes; what the cases promise; what float32 arithmetic costs on them (the
figures the bars of tests/test_iou_loss_gpu.py rest on); and the host side -- ``IoULocLoss`` arguments, the longer
``LossConfig``, ``trainer.loc_loss_from_env``."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import iou_loss_cases as ic


@pytest.mark.parametrize("mode", ic.MODES)
def test_oracle_gradients_against_central_differences(mode):
    """float64 throughout, every entry of ``small`` (2 x 70 x 4; the designated anchors sit on a kink and are left out).
    CIoU's ``a`` is held at its value at the point, which is the function its stop-gradient differentiates."""
    c = ic.cases()["small"]
    o = ic.oracle("small", mode)
    a = ic.ciou_weight(c.priors, c.var, c.yd, c.pd) if mode == "ciou" else None
    h = 1e-6
    fd = np.zeros(c.pd.shape)
    pd = c.pd.astype(np.float64)
    for i in np.ndindex(*pd.shape):
        if not ic.positives(c.yd)[i[:2]]:
            continue                                    # the objective does not read a non-positive's prediction at all
        up, dn = pd.copy(), pd.copy()
        up[i] += h
        dn[i] -= h
        fd[i] = (ic.objective(c.priors, c.var, c.yd, up, mode, c.loc_alpha, a) -
                 ic.objective(c.priors, c.var, c.yd, dn, mode, c.loc_alpha, a)) / (2 * h)
    m = ic.compared(c)
    assert np.abs(o["gd"]).max() > 1e-3
    assert not o["gd"][~ic.positives(c.yd)].any()
    np.testing.assert_allclose(o["gd"][m], fd[m], rtol=1e-6, atol=1e-9)


def _boxes(*rows):
    return torch.tensor(rows, dtype=torch.float64)


def test_relations_between_the_modes():
    """giou == iou where one box contains the other (the enclosing box is the union's outer box); ciou == diou where the
    aspect ratios agree (v == 0); diou == iou where the centres coincide (rho2 == 0); and all four differ otherwise."""
    t = _boxes([0.2, 0.2, 0.6, 0.8], [0.2, 0.2, 0.6, 0.8], [0.1, 0.1, 0.5, 0.5], [0.2, 0.2, 0.6, 0.8])
    b = _boxes([0.3, 0.3, 0.5, 0.5],      # inside its target, another centre, another aspect ratio
               [0.1, 0.1, 0.9, 0.9],       # contains its target
               [0.3, 0.2, 0.7, 0.6],       # same aspect ratio (square), overlapping, neither inside
               [0.3, 0.1, 0.5, 0.9])       # the same centre, another aspect ratio, neither inside
    l = {m: ic.box_loss_t(b, t, m).numpy() for m in ic.MODES}
    np.testing.assert_allclose(l["giou"][:2], l["iou"][:2], rtol=0, atol=1e-6)          # eps: (ac - union) / (ac + eps) is 0
    assert np.all(l["giou"][2:] > l["iou"][2:] + 1e-2)
    np.testing.assert_allclose(l["ciou"][2], l["diou"][2], rtol=0, atol=1e-15)
    assert np.all(l["ciou"][[0, 1, 3]] > l["diou"][[0, 1, 3]] + 1e-4)
    np.testing.assert_allclose(l["diou"][3], l["iou"][3], rtol=0, atol=1e-15)
    assert np.all(l["diou"][:3] > l["iou"][:3] + 1e-4)
    # a hand-worked value: two unit-area squares shifted by half a side: inter 0.5, union 1.5, enclosing 1.5 x 1
    v = ic.box_loss_t(_boxes([0.0, 0.5, 1.0, 1.5]), _boxes([0.0, 0.0, 1.0, 1.0]), "diou").item()
    assert abs(v - (1 - 0.5 / 1.5 + 0.25 / (1.5 ** 2 + 1))) < 1e-6
    g = ic.box_loss_t(_boxes([0.0, 2.0, 1.0, 3.0]), _boxes([0.0, 0.0, 1.0, 1.0]), "giou").item()     # disjoint: 1 + 1/3
    assert abs(g - (1 + 1.0 / 3)) < 1e-6


def test_cases_hold_what_they_promise():
    cs = ic.cases()
    T = ic.TILE
    assert [c.yd.shape for c in cs.values()] == [(1, 1, 4), (2, 70, 4), (3, T + 1, 4), (2, 2 * T + 1, 4)]
    assert all(c.priors.shape == (c.yd.shape[1], 4) and c.pd.shape == c.yd.shape for c in cs.values())
    assert ic.positives(cs["tiny"].yd).all()
    assert not ic.positives(cs["small"].yd[0]).any() and ic.positives(cs["small"].yd[1]).sum() >= 10
    import ssd_hip
    assert T == 256                                                  # the shapes above were chosen for this tile
    for B, N in ((32, 2268), (1, 1), (3, T + 1)):                   # B * tiles * 8 bytes, rounded up to a multiple of 256
        assert ssd_hip.lib().ssd_iou_loc_loss_workspace_bytes(B, N) == -(-(B * -(-N // T) * 8) // 256) * 256
    for name, c in cs.items():
        if name == "tiny":
            continue
        pos = ic.positives(c.yd)
        b, t = ic._decode64(c.priors, c.pd, c.var), ic._decode64(c.priors, c.yd, c.var)
        inter_h = np.minimum(b[..., 2], t[..., 2]) - np.maximum(b[..., 0], t[..., 0])
        inter_w = np.minimum(b[..., 3], t[..., 3]) - np.maximum(b[..., 1], t[..., 1])
        disjoint = pos & ((inter_h < 0) | (inter_w < 0))
        assert disjoint.sum() >= 0.1 * pos.sum() and all(disjoint[at] for at in c.marks["disjoint"]), name
        at = c.marks["pred_inside"]
        assert pos[at] and (b[at][:2] > t[at][:2]).all() and (b[at][2:] < t[at][2:]).all(), name
        at = c.marks["target_inside"]
        assert pos[at] and (t[at][:2] > b[at][:2]).all() and (t[at][2:] < b[at][2:]).all(), name
        assert 1 <= len(c.marks["equal"]) <= 3
        for at in c.marks["equal"]:
            assert pos[at] and np.array_equal(c.pd[at], c.yd[at])
        dist = ic.tie_distance(c.priors, c.var, c.yd, c.pd)
        assert dist[pos & ic.compared(c)].min() >= ic.TIE_MARGIN, name
        iou = 1 - ic.oracle(name, "iou")["l"][pos & ~disjoint & ic.compared(c)]
        assert 0.4 < iou.mean() < 0.9, (name, iou.mean())


def test_what_float32_costs_on_the_cases():
    """The kernel's arithmetic in plain float32 NumPy (``float32_restatement``, analytic gradient) against the float64 oracle,
    every case and mode, no anchor left out but the designated ones in the gradient.  Worst over all:
      per-anchor loss  2.40e-6 relative (two_tiles_plus_one, giou; 4.7e-7 absolute)
      per-image loss   1.98e-7 relative (small, iou)
      gradient         2.68e-8 absolute (tiny, giou, largest entry 0.127); 6.11e-7 of the case's largest entry (small, ciou)
    Four times each stays inside rtol 1e-5 / atol 1e-7 (losses) and 1e-6 (gradients), so those bars stand unwidened; the
    relative gradient bar of the GPU test is four times the last figure as computed where the test runs."""
    fig = ic.restatement_figures()
    for row in fig["rows"]:
        print("%-20s %-5s per-anchor %.2e  per-image %.2e  |grad - oracle| %.2e = %.2e of the largest entry %.2e" % row)
    print("worst: per-anchor %.2e  per-image %.2e  gradient %.2e absolute, %.2e relative" % (fig["l"], fig["loc"], fig["g"], fig["grel"]))
    for name, c in ic.cases().items():
        pos, m = ic.positives(c.yd), ic.compared(c)
        for mode in ic.MODES:
            o = ic.oracle(name, mode)
            l, loc, gd = ic.float32_restatement(c, mode)
            assert l.dtype == loc.dtype == gd.dtype == np.float32
            # the bars themselves, at a quarter
            assert np.all(np.abs(l - o["l"])[m] <= (ic.LOSS_ATOL + ic.LOSS_RTOL * np.abs(o["l"])[m]) / 4), (name, mode)
            assert np.all(np.abs(loc - o["loc"]) <= (ic.LOSS_ATOL + ic.LOSS_RTOL * np.abs(o["loc"])) / 4), (name, mode)
            for at in c.marks["equal"]:
                assert abs(l[at]) <= 1e-6 and np.abs(gd[at]).max() <= 1 and np.isfinite(gd[at]).all()
            assert not gd[~pos].any()
    assert fig["g"] <= ic.GRAD_ATOL / 4 and 0 < fig["grel"] < 1e-5        # float32: a relative figure of a few 2^-23


def test_iou_loc_loss_arguments():
    import ssd_hip
    from ssd_loss import CustomLoss, FocalLoss, IoULocLoss
    priors, _, var = ic.pool()
    base = CustomLoss(3, 1.5)
    il = IoULocLoss(base, priors, var)
    assert il.mode == "ciou" and il.loc_loss_alpha == 1.5 and il.neg_pos_ratio == 3.0 and il.num_priors == priors.shape[0]
    assert il.conf_loss is base and il.last_final_mask is None and il.last_cross_entropy is None and il.last_box_loss is None
    cfg = il.get_config()
    assert cfg["mode"] == "ciou" and cfg["num_priors"] == 2268 and cfg["conf_loss"] == {
        "class": "CustomLoss", "neg_pos_ratio": 3.0, "loc_loss_alpha": 1.5}
    np.testing.assert_allclose(cfg["variances"], [0.1, 0.1, 0.2, 0.2], rtol=1e-6)
    assert repr(il) == "IoULocLoss(CustomLoss(neg_pos_ratio=3, loc_loss_alpha=1.5), priors=2268, variances=[0.1, 0.1, 0.2, 0.2], mode=ciou)"
    fl = IoULocLoss(FocalLoss(1.0), priors.tolist(), list(var), mode=" GIoU ")
    assert fl.mode == "giou" and fl.get_config()["conf_loss"]["class"] == "FocalLoss" and not hasattr(fl, "neg_pos_ratio")
    assert repr(fl) == "IoULocLoss(FocalLoss(loc_loss_alpha=1, alpha=0.25, gamma=2), priors=2268, variances=[0.1, 0.1, 0.2, 0.2], mode=giou)"
    for mode, kind in (("iou", ssd_hip.LOC_IOU), ("giou", ssd_hip.LOC_GIOU), ("diou", ssd_hip.LOC_DIOU), ("ciou", ssd_hip.LOC_CIOU)):
        n = IoULocLoss(FocalLoss(2.0, 0.5, 1.0), priors, var, mode).to_native()
        assert (n.kind, n.loc_loss_alpha, n.focal_alpha, n.focal_gamma, n.loc_kind) == (ssd_hip.LOSS_FOCAL, 2.0, 0.5, 1.0, kind)
        np.testing.assert_array_equal(np.array(n.variances[:], np.float32), np.asarray(var, np.float32))
    n = il.to_native()
    assert (n.kind, n.neg_pos_ratio, n.loc_loss_alpha, n.loc_kind) == (ssd_hip.LOSS_HARD_NEGATIVE, 3.0, 1.5, ssd_hip.LOC_CIOU)
    for bad in ("huber", "", "l1", None, 3):
        with pytest.raises(ValueError):
            IoULocLoss(base, priors, var, mode=bad)
    for bad in ([0.1, 0.1, 0.2], [0.1, 0.1, 0.2, 0.0], [0.1, -0.1, 0.2, 0.2], [0.1, 0.1, float("nan"), 0.2],
                [0.1, 0.1, 0.2, float("inf")], None, "abcd", 0.1):
        with pytest.raises(ValueError):
            IoULocLoss(base, priors, bad)
    for bad in (priors[:, :3], priors.reshape(-1), priors[None], np.zeros((0, 4), np.float32), "priors"):
        with pytest.raises(ValueError):
            IoULocLoss(base, bad, var)
    with pytest.raises(TypeError):
        IoULocLoss(il, priors, var)
    with pytest.raises(TypeError):
        IoULocLoss(None, priors, var)


def test_loss_config_mirrors_the_struct():
    import ssd_hip
    from ssd_loss import CustomLoss, FocalLoss
    assert ctypes.sizeof(ssd_hip.LossConfig) == ssd_hip.lib().ssd_loss_config_bytes()
    five = ssd_hip.LossConfig(1, 3.0, 1.0, 0.25, 2.0)                # five positional values, as before: the tail is zero
    assert (five.kind, five.neg_pos_ratio, five.loc_loss_alpha, five.focal_alpha, five.focal_gamma) == (1, 3.0, 1.0, 0.25, 2.0)
    assert five.loc_kind == ssd_hip.LOC_HUBER == 0 and not five.priors_dev and list(five.variances) == [0.0] * 4
    for base in (CustomLoss(3, 1), FocalLoss(1.0)):
        n = base.to_native()
        assert n.loc_kind == 0 and not n.priors_dev and list(n.variances) == [0.0] * 4
    assert [f[0] for f in ssd_hip.LossConfig._fields_][:5] == ["kind", "neg_pos_ratio", "loc_loss_alpha", "focal_alpha", "focal_gamma"]
    assert (ssd_hip.LOC_IOU, ssd_hip.LOC_GIOU, ssd_hip.LOC_DIOU, ssd_hip.LOC_CIOU) == (1, 2, 3, 4)


def test_loc_loss_from_env(monkeypatch):
    from ssd_loss import CustomLoss, FocalLoss, IoULocLoss
    trainer = importlib.import_module("trainer")
    priors, _, var = ic.pool()
    hp = {"neg_pos_ratio": 3, "loc_loss_alpha": 1, "variances": [float(v) for v in var]}
    monkeypatch.delenv("SSD_TRAINER_LOC_LOSS", raising=False)
    for base in (CustomLoss(3, 1), FocalLoss(1.0)):
        assert trainer.loc_loss_from_env(base, priors, hp) is base
        for value in ("huber", " Huber ", ""):
            monkeypatch.setenv("SSD_TRAINER_LOC_LOSS", value)
            assert trainer.loc_loss_from_env(base, priors, hp) is base
        for value in ("iou", "giou", "diou", "ciou", " CIoU "):
            monkeypatch.setenv("SSD_TRAINER_LOC_LOSS", value)
            il = trainer.loc_loss_from_env(base, priors, hp)
            assert type(il) is IoULocLoss and il.conf_loss is base and il.mode == value.strip().lower()
            assert il.variances == hp["variances"] and il.num_priors == priors.shape[0]
        for value in ("l1", "smooth", "eiou"):
            monkeypatch.setenv("SSD_TRAINER_LOC_LOSS", value)
            with pytest.raises(ValueError):
                trainer.loc_loss_from_env(base, priors, hp)
        monkeypatch.delenv("SSD_TRAINER_LOC_LOSS")


def test_compile_refuses_priors_of_another_geometry():
    """The training step reads one prior row per anchor of the model through a bare pointer, so ``compile`` takes an
    ``IoULocLoss`` only when it holds as many prior boxes as the model has anchors (ssd_net_create is host code)."""
    import helpers
    from models._net import SSDModel
    from oracle import bbox_oracle as bo
    from ssd_loss import CustomLoss, FocalLoss, IoULocLoss
    priors, _, var = ic.pool()
    m = SSDModel("mobilenet_v2", helpers.hyper_params("mobilenet_v2"))
    assert m.num_priors == priors.shape[0] == 2268
    good = IoULocLoss(CustomLoss(3, 1), priors, var, "giou")
    m.compile(loss=[good.loc_loss_fn, good.conf_loss_fn])
    assert m._loss is good and m._native_loss.loc_kind == 2
    hp = helpers.hyper_params("vgg16")
    other = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])          # 8732 boxes
    for bad in (priors[:-1], priors[:100], other):
        for base in (CustomLoss(3, 1), FocalLoss(1.0)):
            il = IoULocLoss(base, bad, var)
            with pytest.raises(ValueError, match="prior boxes"):
                m.compile(loss=[il.loc_loss_fn, il.conf_loss_fn])
    assert m._loss is good                                            # a refused compile leaves the compiled loss in place
