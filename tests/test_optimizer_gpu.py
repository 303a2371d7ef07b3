"""Keras SGD / Adam with gradient clipping on the device (csrc/ssd_optim.hip, ssd_net_optimizer_step) against the float64
restatement of tests/optimizer_cases.py.  Shaped like tests/test_finetune_gpu.py::test_adam_leaves_frozen_parameters_alone:
the full 300 x 300 MobileNetV2 net, ``ssd_net_train_begin(net, 1)``, synthetic gradients handed to ``apply_gradients``, no
forward pass (but for the public-path and the trainer test).  ONE model instance serves every case: each case puts the
initial weights back, clears the optimizer state and compiles its optimizer.

Every case runs two consecutive steps, so the slots are exercised from zero and from non-zero; the second step's
reference starts from the DEVICE's state after the first (weights and slots as read back), so each step is held to the
tolerance of one step.  The gradients (optimizer_cases.seeded_gradients) are seeded normals with a per-variable scale
cycling through 0, 0.01, 0.3, 3; the second step's have the first's signs, so nothing cancels.

Tolerances.  Unclipped weights: ``rtol=1e-6, atol=2e-9`` at ``LR = 2e-5``, the existing Adam tests' bar.  Slots and clipped
updates: ``rtol=4e-6`` -- a fixed-tree fp32 sum of 4096 squares errs by at most about 12 roundings (7e-7), the double
sum over a variable's partials adds nothing visible, the square root halves it, three more roundings for scale, multiply
and accumulate.  (Slots get ``atol=1e-37``, below fp32's normal range: no value here comes near it.)

Measured on an MI355X: worst weight error 5.9 % of its bound (the fp32 rounding of the weight itself), worst relative slot
error 3.3e-7 (Adam's slots under ``clipnorm``); global norm of the public-path test's B = 2 gradient 48.39."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import helpers
import optimizer_cases as oc

pytestmark = pytest.mark.gpu

LR = 2e-5
CLIPNORM = 1.0          # between the norms of the small and the large variables (checked by the precondition test)
CLIPVALUE = 0.5
GLOBAL_CLIPNORM = 5.0


def _layer(name):
    return name.rsplit("/", 1)[0]


@pytest.fixture(scope="module")
def ctx():
    import ssd_hip as h
    from models._net import SSDModel
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = helpers.hyper_params("mobilenet_v2")
    m = SSDModel("mobilenet_v2", hp)
    w0 = {k: v.copy() for k, v in helpers.synthetic_weights("mobilenet_v2", hp).items()}
    m.set_weights(w0)
    m.compile(learning_rate=LR)
    h.check(h.lib().ssd_net_train_begin(m._net, 1), "ssd_net_train_begin")
    m._train_batch = 1
    offs = m.trainable_offsets()
    P = int(h.lib().ssd_net_trainable_floats(m._net))
    g1, g2 = oc.seeded_gradients(offs, P, seed=17)
    dev = h.device()
    return {"m": m, "hp": hp, "w0": w0, "offs": offs, "P": P, "g": (g1, g2),
            "gd": (torch.from_numpy(g1).to(dev), torch.from_numpy(g2).to(dev))}


def _fresh(ctx, optimizer, freeze=False):
    """The shared model at its initial weights, everything trainable (or the backbone frozen), zero slots, iteration 0."""
    import ssd_hip as h
    m = ctx["m"]
    m.set_trainable("*", True)
    frozen = set(m.freeze_backbone()) if freeze else set()
    m.set_weights(ctx["w0"])
    h.check(h.lib().ssd_net_optimizer_reset(m._net), "ssd_net_optimizer_reset")
    m.compile(optimizer=optimizer)
    assert h.lib().ssd_net_train_steps(m._net) == 0
    return m, frozen


def _zero_slots(optimizer, weights):
    return {n: {s: np.zeros(w.shape, np.float32) for s in optimizer.slots} for n, w in weights.items()}


def _compare(names, got_w, got_s, want_w, want_s, w_rtol):
    # printed before anything is asserted: the worst error of a weight in units of its bound, the worst relative error of a slot
    worst_w = worst_s = 0.0
    for n in names:
        worst_w = max(worst_w, float((np.abs(got_w[n] - want_w[n]) / (2e-9 + w_rtol * np.abs(want_w[n]))).max()))
        for s, want in want_s[n].items():
            nz = np.asarray(want) != 0
            if nz.any():
                worst_s = max(worst_s, float((np.abs(got_s[n][s][nz] - want[nz]) / np.abs(want[nz])).max()))
    print("worst weight error %.3f of its bound (rtol %.0e, atol 2e-9), worst relative slot error %.2e (bound 4e-6)" % (
        worst_w, w_rtol, worst_s))
    for n in names:
        np.testing.assert_allclose(got_w[n], want_w[n], rtol=w_rtol, atol=2e-9, err_msg=n)
        for s, want in want_s[n].items():
            np.testing.assert_allclose(got_s[n][s], want, rtol=4e-6, atol=1e-37, err_msg="%s:%s" % (n, s))


def _two_steps(ctx, optimizer, grad_scale=1.0):
    """Two steps of `optimizer` on the seeded gradients, each compared with the oracle's step from the device's state."""
    m, _ = _fresh(ctx, optimizer)
    offs = ctx["offs"]
    cfg = {k: v for k, v in optimizer.get_config().items() if k not in ("learning_rate", "amsgrad")}
    clipped = any(cfg[k] is not None for k in ("clipnorm", "clipvalue", "global_clipnorm"))
    w = {n: ctx["w0"][n] for n in offs}
    slots = _zero_slots(optimizer, w)
    for t in (1, 2):
        m.apply_gradients(ctx["gd"][t - 1], grad_scale=grad_scale)
        got_w, st = m.get_weights(), m.get_optimizer_state()
        assert st["kind"] == optimizer.name and st["iterations"] == t
        want_w, want_s = oc.step(optimizer.name, w, slots, oc.split(ctx["g"][t - 1], offs), t, LR, grad_scale, **cfg)
        _compare(offs, got_w, st["slots"], want_w, want_s, 4e-6 if clipped else 1e-6)
        for n in ctx["w0"]:                                  # the moving statistics are no business of the optimizer
            if n not in offs:
                np.testing.assert_array_equal(got_w[n], ctx["w0"][n], err_msg=n)
        # a variable without a gradient does not move (exactly: every update here is a multiple of g); one with a gradient
        # does (asserted where no clip shrinks the step below the weights' last bit)
        still = [n for n in offs if not ctx["g"][t - 1][offs[n][0]:offs[n][0] + got_w[n].size].any()]
        assert 0 < len(still) < len(offs)
        for n in offs:
            if n in still:
                np.testing.assert_array_equal(got_w[n].view(np.uint32), w[n].view(np.uint32), err_msg=n)
            elif not clipped:
                assert (got_w[n] != w[n]).any(), n
        w, slots = {n: got_w[n] for n in offs}, st["slots"]
    return m


# ---------------------------------------------------------------------------------------------- preconditions (inputs only)
def test_preconditions_on_the_inputs(ctx):
    """Conditions on the inputs, not measurements: under CLIPNORM the oracle finds variables above the threshold, below it
    and all-zero in both steps' gradients, the global norm lies above GLOBAL_CLIPNORM, CLIPVALUE cuts some elements and
    leaves others, and some trainable variable starts at an offset that is no multiple of 4 floats (the kernels' 16-byte
    body cannot start at the segment's first element there)."""
    offs = ctx["offs"]
    for g in ctx["g"]:
        norms = {n: float(np.sqrt((a.astype(np.float64) ** 2).sum())) for n, a in oc.split(g, offs).items()}
        above = [n for n, v in norms.items() if v > 2 * CLIPNORM]
        below = [n for n, v in norms.items() if 0 < v < 0.5 * CLIPNORM]
        zero = [n for n, v in norms.items() if v == 0]
        assert above and below and zero, (len(above), len(below), len(zero))
        assert oc.global_norm(list(oc.split(g, offs).values())) > 2 * GLOBAL_CLIPNORM
        assert (np.abs(g) > CLIPVALUE).any() and ((np.abs(g) < CLIPVALUE) & (g != 0)).any()
    odd = [n for n, (off, _) in offs.items() if off % 4]
    assert odd, "no trainable variable starts off a 16-byte boundary"
    sizes = [int(np.prod(s)) for _, s in offs.values()]
    assert min(sizes) < 4096 < max(sizes) and any(s % 4096 for s in sizes if s > 4096)      # one and several segments, ragged tails


# ---------------------------------------------------------------------------------------------- the cases
def _cases():
    import optimizers as o
    return {
        "sgd": lambda: o.SGD(LR),
        "momentum": lambda: o.SGD(LR, momentum=0.9),
        "nesterov": lambda: o.SGD(LR, momentum=0.9, nesterov=True),
        "sgd-clipvalue": lambda: o.SGD(LR, clipvalue=CLIPVALUE),
        "sgd-clipnorm": lambda: o.SGD(LR, momentum=0.9, clipnorm=CLIPNORM),
        "sgd-global-clipnorm": lambda: o.SGD(LR, momentum=0.9, global_clipnorm=GLOBAL_CLIPNORM),
        "sgd-clipnorm-clipvalue": lambda: o.SGD(LR, momentum=0.9, nesterov=True, clipnorm=CLIPNORM, clipvalue=0.001),
        "adam-global-clipnorm": lambda: o.Adam(LR, global_clipnorm=GLOBAL_CLIPNORM),
        "adam-clipnorm": lambda: o.Adam(LR, clipnorm=CLIPNORM),
    }


@pytest.mark.parametrize("case", ["sgd", "momentum", "nesterov", "sgd-clipvalue", "sgd-clipnorm", "sgd-global-clipnorm",
                                  "sgd-clipnorm-clipvalue", "adam-global-clipnorm", "adam-clipnorm"])
def test_two_steps_match_the_oracle(ctx, case):
    """(sgd-clipnorm-clipvalue: after the norm clip at 1.0 a variable of n elements holds values around 1 / sqrt(n); the
    value clip at 0.001 then cuts into the variables below a million elements and leaves the small-gradient ones alone.)"""
    _two_steps(ctx, _cases()[case]())


def test_grad_scale_is_applied_before_the_clip(ctx):
    """At grad_scale 0.5 the norms halve: a variable between CLIPNORM and 2 * CLIPNORM is clipped without it and not with it."""
    import optimizers as o
    offs = ctx["offs"]
    norms = [float(np.sqrt((a.astype(np.float64) ** 2).sum())) for a in oc.split(ctx["g"][0], offs).values()]
    assert any(0.5 * v > CLIPNORM for v in norms) and any(0 < 0.5 * v < CLIPNORM for v in norms)
    _two_steps(ctx, o.SGD(LR, momentum=0.9, clipnorm=CLIPNORM), grad_scale=0.5)


def test_plain_sgd_leaves_the_slots_alone(ctx):
    """momentum == 0: no accumulator is read or written -- a pattern put into the slot survives the step bitwise."""
    import optimizers as o
    m, _ = _fresh(ctx, o.SGD(LR, clipnorm=CLIPNORM))
    st = m.get_optimizer_state()
    rng = np.random.default_rng(3)
    for n in st["slots"]:
        st["slots"][n]["momentum"] = rng.standard_normal(st["slots"][n]["momentum"].shape).astype(np.float32)
    m.set_optimizer_state(st)
    m.apply_gradients(ctx["gd"][0])
    after = m.get_optimizer_state()
    assert after["iterations"] == 1
    for n in st["slots"]:
        np.testing.assert_array_equal(after["slots"][n]["momentum"].view(np.uint32), st["slots"][n]["momentum"].view(np.uint32), err_msg=n)


# ---------------------------------------------------------------------------------------------- bitwise
def test_a_clipped_step_is_reproducible(ctx):
    import optimizers as o
    runs = []
    for _ in range(2):
        m, _ = _fresh(ctx, o.SGD(LR, momentum=0.9, nesterov=True, clipnorm=CLIPNORM, clipvalue=CLIPVALUE))
        m.apply_gradients(ctx["gd"][0])
        m.apply_gradients(ctx["gd"][1])
        runs.append((m.get_weights(), m.get_optimizer_state()["slots"]))
    for n in ctx["offs"]:
        np.testing.assert_array_equal(runs[0][0][n].view(np.uint32), runs[1][0][n].view(np.uint32), err_msg=n)
        np.testing.assert_array_equal(runs[0][1][n]["momentum"].view(np.uint32), runs[1][1][n]["momentum"].view(np.uint32), err_msg=n)


@pytest.mark.parametrize("freeze", [False, True], ids=["all-trainable", "backbone-frozen"])
def test_unclipped_adam_is_ssd_net_adam_step_bit_for_bit(ctx, freeze):
    import optimizers as o
    import ssd_hip as h
    m, _ = _fresh(ctx, o.Adam(LR), freeze)
    for gd in ctx["gd"]:
        m.apply_gradients(gd)
    new_w, new_s = m.get_weights(), m.get_optimizer_state()
    m, frozen = _fresh(ctx, o.Adam(LR), freeze)
    for gd in ctx["gd"]:
        h.check(h.lib().ssd_net_adam_step(m._net, h.ptr(gd), LR, 0.9, 0.999, 1e-7, 1.0, h.stream()), "ssd_net_adam_step")
    old_w, old_s = m.get_weights(), m.get_optimizer_state()
    assert new_s["iterations"] == old_s["iterations"] == 2
    changed = 0
    for n in ctx["offs"]:
        np.testing.assert_array_equal(new_w[n].view(np.uint32), old_w[n].view(np.uint32), err_msg=n)
        for s in ("m", "v"):
            np.testing.assert_array_equal(new_s["slots"][n][s].view(np.uint32), old_s["slots"][n][s].view(np.uint32), err_msg=n)
        changed += int((new_w[n] != ctx["w0"][n]).any())
        if _layer(n) in frozen:
            np.testing.assert_array_equal(new_w[n].view(np.uint32), ctx["w0"][n].view(np.uint32), err_msg=n)
    assert changed > 10 and (not freeze or changed < len(ctx["offs"]) - 100)


def test_a_trainable_elements_update_does_not_depend_on_the_table(ctx):
    """Two unclipped Adam steps with everything trainable, then from the same start under ``freeze_backbone()``: the table
    of segments differs (the frozen variables have none), what happens to an element that is in both does not.  Every
    variable trainable in both runs has the same bits in var, m and v; a frozen one keeps its initial bits and zero slots."""
    import optimizers as o
    runs = []
    for freeze in (False, True):
        m, frozen = _fresh(ctx, o.Adam(LR), freeze)
        for gd in ctx["gd"]:
            m.apply_gradients(gd)
        st = m.get_optimizer_state()
        assert st["iterations"] == 2
        runs.append((m.get_weights(), st["slots"]))
    m.set_trainable("*", True)
    (all_w, all_s), (fr_w, fr_s) = runs
    live = [n for n in ctx["offs"] if _layer(n) not in frozen]
    assert len(frozen) == 104 and 0 < len(live) < len(ctx["offs"])
    for n in ctx["offs"]:
        if n in live:
            np.testing.assert_array_equal(fr_w[n].view(np.uint32), all_w[n].view(np.uint32), err_msg=n)
            for s in ("m", "v"):
                np.testing.assert_array_equal(fr_s[n][s].view(np.uint32), all_s[n][s].view(np.uint32), err_msg="%s:%s" % (n, s))
        else:
            np.testing.assert_array_equal(fr_w[n].view(np.uint32), ctx["w0"][n].view(np.uint32), err_msg=n)
            assert not fr_s[n]["m"].any() and not fr_s[n]["v"].any(), n
    assert sum(int((all_w[n] != ctx["w0"][n]).any()) for n in live) > 10


def test_the_scalar_and_the_16_byte_path_give_the_same_bits(ctx):
    """Two unclipped Adam steps at grad_scale 0.5 from a gradient buffer that is 16-byte aligned (head, 16-byte body and tail
    loops) and from the same values 4 bytes further on (every element through the scalar loop): the same bits in var, m and v.
    Adam's roundings are spelled out in the source, so they do not depend on the loop an element goes through."""
    import optimizers as o
    P = ctx["P"]
    runs = []
    for shift in (0, 1):
        m, _ = _fresh(ctx, o.Adam(LR))
        for gd in ctx["gd"]:
            buf = torch.empty(P + 4, dtype=torch.float32, device=gd.device)
            base = (-(buf.data_ptr() // 4)) % 4                  # first element of buf on a 16-byte boundary
            g = buf[base + shift:base + shift + P]
            g.copy_(gd)
            assert g.data_ptr() % 16 == 4 * shift
            m.apply_gradients(g, grad_scale=0.5)
        torch.cuda.synchronize()
        st = m.get_optimizer_state()
        assert st["iterations"] == 2
        runs.append((m.get_weights(), st["slots"]))
    (a_w, a_s), (u_w, u_s) = runs
    for n in ctx["offs"]:
        np.testing.assert_array_equal(u_w[n].view(np.uint32), a_w[n].view(np.uint32), err_msg=n)
        for s in ("m", "v"):
            np.testing.assert_array_equal(u_s[n][s].view(np.uint32), a_s[n][s].view(np.uint32), err_msg="%s:%s" % (n, s))
    assert sum(int((a_w[n] != ctx["w0"][n]).any()) for n in ctx["offs"]) > 100


# ---------------------------------------------------------------------------------------------- frozen ranges
def test_frozen_ranges_stay_out_of_norm_and_update(ctx):
    """freeze_backbone() under SGD momentum + global_clipnorm: the frozen ranges of the gradient hold 1e30 (their squares
    overflow fp32: one of them in the norm and every scale is 0 or NaN), the slots start from a random pattern.  Frozen weights
    and accumulators stay bitwise, the rest matches the oracle's step over the trainable variables alone."""
    import optimizers as o
    opt = o.SGD(LR, momentum=0.9, global_clipnorm=GLOBAL_CLIPNORM)
    m, frozen = _fresh(ctx, opt, freeze=True)
    offs = ctx["offs"]
    live = [n for n in offs if _layer(n) not in frozen]
    assert 0 < len(live) < len(offs) and len(frozen) == 104
    st = m.get_optimizer_state()
    rng = np.random.default_rng(23)
    for n in offs:
        # (the sign of the step's own term -lr * g, so that the accumulator does not cancel)
        a = np.abs(rng.standard_normal(offs[n][1])).astype(np.float32) * np.float32(1e-5)
        st["slots"][n]["momentum"] = -a * np.sign(ctx["g"][0][offs[n][0]:offs[n][0] + a.size].reshape(a.shape)).astype(np.float32)
    m.set_optimizer_state(st)
    g = ctx["g"][0].copy()
    for n in offs:
        if _layer(n) in frozen:
            g[offs[n][0]:offs[n][0] + int(np.prod(offs[n][1]))] = 1e30
    m.apply_gradients(torch.from_numpy(g).to(ctx["gd"][0].device))
    got_w, after = m.get_weights(), m.get_optimizer_state()
    for n in offs:
        if _layer(n) in frozen:
            np.testing.assert_array_equal(got_w[n].view(np.uint32), ctx["w0"][n].view(np.uint32), err_msg=n)
            np.testing.assert_array_equal(after["slots"][n]["momentum"].view(np.uint32), st["slots"][n]["momentum"].view(np.uint32), err_msg=n)
    want_w, want_s = oc.step("sgd", {n: ctx["w0"][n] for n in live}, {n: st["slots"][n] for n in live}, oc.split(g, offs, live), 1, LR,
                             momentum=0.9, global_clipnorm=GLOBAL_CLIPNORM)
    assert oc.global_norm(list(oc.split(g, offs, live).values())) > 2 * GLOBAL_CLIPNORM
    _compare(live, got_w, after["slots"], want_w, want_s, 4e-6)
    assert all(np.isfinite(got_w[n]).all() for n in offs)
    m.set_trainable("*", True)


# ---------------------------------------------------------------------------------------------- kinds
def test_kind_switch_needs_a_reset(ctx):
    import optimizers as o
    import ssd_hip as h
    lib = h.lib()
    m, _ = _fresh(ctx, o.Adam(LR))
    m.apply_gradients(ctx["gd"][0])
    before = m.get_weights()
    sgd = o.SGD(LR, momentum=0.9).to_native()
    rc = lib.ssd_net_optimizer_step(m._net, h.ptr(ctx["gd"][0]), ctypes.byref(sgd), LR, 1.0, h.stream())
    assert rc == -4 and "ssd_net_optimizer_reset" in lib.ssd_last_error().decode()
    assert lib.ssd_net_train_steps(m._net) == 1                   # nothing ran: Adam's m was not taken for a momentum
    after = m.get_weights()
    for n in ctx["offs"]:
        np.testing.assert_array_equal(after[n].view(np.uint32), before[n].view(np.uint32), err_msg=n)
    m.compile(optimizer=o.Adam(LR, clipvalue=1.0))               # the same kind keeps the state
    assert lib.ssd_net_train_steps(m._net) == 1 and any(s["m"].any() for s in m.get_optimizer_state()["slots"].values())
    m.compile(optimizer=o.SGD(LR, momentum=0.9))                  # another kind: fresh slots, iteration 0
    st = m.get_optimizer_state()
    assert st["kind"] == "sgd" and st["iterations"] == 0 and set(next(iter(st["slots"].values()))) == {"momentum"}
    assert not any(s["momentum"].any() for s in st["slots"].values())
    m.apply_gradients(ctx["gd"][0])
    assert lib.ssd_net_train_steps(m._net) == 1
    # ... and the other way round: ssd_net_adam_step on SGD's accumulator
    assert lib.ssd_net_adam_step(m._net, h.ptr(ctx["gd"][0]), LR, 0.9, 0.999, 1e-7, 1.0, h.stream()) == -4
    with pytest.raises(ValueError):
        m.set_optimizer_state({"kind": "adam", "iterations": 0, "slots": {}})


# ---------------------------------------------------------------------------------------------- resuming a run
@pytest.fixture(scope="module")
def second(ctx):
    from models._net import SSDModel
    m = SSDModel("mobilenet_v2", ctx["hp"])
    m.set_weights(ctx["w0"])
    return m


def test_state_round_trip_resumes_bitwise(ctx, second, tmp_path):
    import optimizers as o
    make = lambda: o.Adam(LR, global_clipnorm=GLOBAL_CLIPNORM)
    m, _ = _fresh(ctx, make())
    seq = [ctx["gd"][0], ctx["gd"][1], ctx["gd"][0], ctx["gd"][1], ctx["gd"][0]]
    for gd in seq[:3]:
        m.apply_gradients(gd)
    m.save_optimizer_state(str(tmp_path / "opt.npz"))
    m.save_weights(str(tmp_path / "w.npz"))
    for gd in seq[3:]:
        m.apply_gradients(gd)
    want_w, want_s = m.get_weights(), m.get_optimizer_state()
    assert want_s["iterations"] == 5
    second.compile(optimizer=make())
    second.load_weights(str(tmp_path / "w.npz"))
    second.load_optimizer_state(str(tmp_path / "opt.npz"))
    assert second.get_optimizer_state()["iterations"] == 3
    for gd in seq[3:]:
        second.apply_gradients(gd)
    got_w, got_s = second.get_weights(), second.get_optimizer_state()
    assert got_s["iterations"] == 5 and got_s["kind"] == "adam"
    for n in want_w:
        np.testing.assert_array_equal(got_w[n].view(np.uint32), want_w[n].view(np.uint32), err_msg=n)
    for n in ctx["offs"]:
        for s in ("m", "v"):
            np.testing.assert_array_equal(got_s["slots"][n][s].view(np.uint32), want_s["slots"][n][s].view(np.uint32), err_msg=n)
    assert sum(int((want_w[n] != ctx["w0"][n]).any()) for n in ctx["offs"]) > 100       # (a quarter of the variables has no gradient)


# ---------------------------------------------------------------------------------------------- the public path
def test_train_on_batch_under_sgd_with_global_clipnorm(ctx, second):
    """B = 2: ``train_on_batch`` on one model, the same batch through ``forward_backward`` plus the float64 oracle on a second.
    The threshold is a quarter of the measured global norm, so the clip acts."""
    import optimizers as o
    from oracle import bbox_oracle as bo
    hp, offs = ctx["hp"], ctx["offs"]
    B = 2
    x = helpers.images(B, 300, seed=41)
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=hp["total_labels"], seed=3)
    yd, yl = bo.calculate_actual_outputs(priors, gt, gl, hp)
    second.set_weights(ctx["w0"])
    second.compile()
    _, _, g = second.forward_backward(x, yd, yl)
    g = g.cpu().numpy().copy()
    assert np.isfinite(g).all()
    gn = float(oc.global_norm(list(oc.split(g, offs).values())))
    c = gn / 4.0
    print("global norm of the B=2 gradient %.4g, global_clipnorm %.4g" % (gn, c))
    assert gn > 0
    opt = o.SGD(LR, momentum=0.9, global_clipnorm=c)
    m, _ = _fresh(ctx, opt)
    loss, loc, conf = m.train_on_batch(x, (yd, yl))
    assert np.isfinite([loss, loc, conf]).all()
    got_w, st = m.get_weights(), m.get_optimizer_state()
    assert st["iterations"] == 1
    w = {n: ctx["w0"][n] for n in offs}
    want_w, want_s = oc.step("sgd", w, _zero_slots(opt, w), oc.split(g, offs), 1, LR, momentum=0.9, global_clipnorm=c)
    _compare(offs, got_w, st["slots"], want_w, want_s, 4e-6)
    # the clip acted: the accumulator is -lr * g / 4, not -lr * g
    big = max(offs, key=lambda n: float(np.abs(oc.split(g, offs, [n])[n]).max()))
    ratio = float(np.abs(st["slots"][big]["momentum"]).max() / (LR * np.abs(oc.split(g, offs, [big])[big]).max()))
    assert 0.2 < ratio < 0.3, ratio


# ---------------------------------------------------------------------------------------------- trainer.main
def test_trainer_sgd_with_global_clipnorm(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_TRAINER_OPTIMIZER", "sgd")
    monkeypatch.setenv("SSD_TRAINER_GLOBAL_CLIPNORM", "10")
    monkeypatch.setenv("SSD_TRAINER_EPOCHS", "1")
    monkeypatch.setenv("SSD_TRAINER_STEPS", "2")
    monkeypatch.setenv("SSD_TRAINER_BATCH", "2")
    monkeypatch.setenv("SSD_TRAINER_AUGMENT", "0")
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "optimizer: SGD(" in out and "momentum=0.9" in out and "global_clipnorm=10.0" in out
    assert np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
    assert os.path.exists(os.path.join("trained", "ssd_mobilenet_v2_model_weights.h5"))
