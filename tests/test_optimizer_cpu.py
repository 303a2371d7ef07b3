"""Keras SGD / Adam with gradient clipping, the part that needs no device: the ``optimizers`` classes (Keras signatures,
defaults, validation), what ``SSDModel.compile(optimizer=...)`` accepts, the argument checks of the C ABI that come before
any launch (include/ssd_hip.h, ssd_net_optimizer_*), the trainer's environment switches, and the float64 restatement
(tests/optimizer_cases.py) against its hand-computed three-element cases -- the device tests hold the kernels to that
restatement, so it is held to pencil and paper here."""
import ctypes
import importlib

import numpy as np
import pytest

import helpers
import optimizer_cases as oc


@pytest.fixture(scope="module")
def model():
    from models._net import SSDModel
    return SSDModel("mobilenet_v2", helpers.hyper_params("mobilenet_v2"))


# ---------------------------------------------------------------------------------------------- the classes
def test_keras_defaults():
    import optimizers
    import ssd_hip as h
    s = optimizers.SGD()
    assert s.get_config() == dict(learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None,
                                  global_clipnorm=None)
    a = optimizers.Adam()
    assert a.get_config() == dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None,
                                  clipvalue=None, global_clipnorm=None)
    assert (s.kind, a.kind) == (h.OPT_SGD, h.OPT_ADAM) and (s.name, a.name) == ("sgd", "adam")
    n = optimizers.SGD(0.1, 0.9, True, clipnorm=2.0, clipvalue=0.5).to_native()
    assert (n.kind, n.nesterov) == (h.OPT_SGD, 1)
    assert (n.momentum, n.clipnorm, n.clipvalue, n.global_clipnorm) == (np.float32(0.9), 2.0, 0.5, 0.0)
    n = optimizers.Adam(global_clipnorm=10).to_native()
    assert (n.kind, n.beta1, n.beta2, n.eps) == (h.OPT_ADAM, np.float32(0.9), np.float32(0.999), np.float32(1e-7))
    assert (n.clipnorm, n.clipvalue, n.global_clipnorm) == (0.0, 0.0, 10.0)
    assert optimizers.SGD(lr=0.5).learning_rate == 0.5                     # Keras' legacy spelling


def test_validation():
    import optimizers
    for bad in (dict(momentum=-0.1), dict(momentum=1.5), dict(momentum="x"), dict(learning_rate=-1.0), dict(clipnorm=0.0),
                dict(clipvalue=-1.0), dict(global_clipnorm=float("nan")), dict(clipnorm=1.0, global_clipnorm=1.0)):
        with pytest.raises(ValueError):
            optimizers.SGD(**bad)
    for bad in (dict(beta_1=1.0), dict(beta_2=-0.5), dict(beta_2=1.0), dict(epsilon=-1e-7), dict(clipnorm=1.0, global_clipnorm=2.0)):
        with pytest.raises(ValueError):
            optimizers.Adam(**bad)
    with pytest.raises(NotImplementedError):
        optimizers.Adam(amsgrad=True)
    for cls in (optimizers.SGD, optimizers.Adam):
        with pytest.raises(NotImplementedError):
            cls(decay=1e-4)
        with pytest.raises(TypeError):
            cls(no_such_argument=1)
    assert optimizers.SGD(momentum=1.0).momentum == 1.0 and optimizers.Adam(beta_1=0.0).beta_1 == 0.0      # the closed ends


def test_compile_accepts(model):
    import optimizers
    import ssd_hip as h
    model.compile()
    assert isinstance(model._optimizer, optimizers.Adam) and model._optimizer.learning_rate == 1e-3
    model.compile(learning_rate=3e-4, beta_1=0.8, beta_2=0.99, epsilon=1e-6)                # None: Adam from the keywords
    assert model._optimizer.get_config() == dict(learning_rate=3e-4, beta_1=0.8, beta_2=0.99, epsilon=1e-6, amsgrad=False,
                                                 clipnorm=None, clipvalue=None, global_clipnorm=None)
    model.compile(optimizer="sgd")
    assert isinstance(model._optimizer, optimizers.SGD) and model._optimizer.learning_rate == 0.01
    model.compile(optimizer="Adam")
    assert isinstance(model._optimizer, optimizers.Adam)
    mine = optimizers.SGD(0.05, momentum=0.9, nesterov=True, global_clipnorm=5.0)
    model.compile(optimizer=mine)                          # (another kind before any training state: the reset is a no-op)
    assert model._optimizer is mine and model._native_optimizer.kind == h.OPT_SGD
    assert model._native_optimizer.global_clipnorm == 5.0 and model._native_optimizer.nesterov == 1
    for bad in (1e-3, "rmsprop", object(), optimizers.SGD, ["sgd"]):
        with pytest.raises(TypeError):
            model.compile(optimizer=bad)
    assert model._optimizer is mine                        # a refused compile changes nothing


# ---------------------------------------------------------------------------------------------- the C ABI
def test_abi_refuses_bad_arguments_before_any_launch(model):
    import ssd_hip as h
    lib, net = h.lib(), model._net
    buf = (ctypes.c_float * 4)()
    g = ctypes.cast(buf, ctypes.c_void_p)

    def opt(**kw):
        o = h.Optimizer(kind=h.OPT_SGD, beta1=0.9, beta2=0.999, eps=1e-7, momentum=0.9, nesterov=0, clipnorm=0.0, clipvalue=0.0,
                        global_clipnorm=0.0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def step(o, net=net, g=g):
        return lib.ssd_net_optimizer_step(net, g, ctypes.byref(o) if o is not None else None, 1e-3, 1.0, None)
    assert step(opt(), net=None) == -1 and step(opt(), g=None) == -1 and step(None) == -1
    for bad in (dict(kind=2), dict(kind=-1), dict(momentum=-0.1), dict(momentum=1.5), dict(momentum=float("nan")),
                dict(kind=h.OPT_ADAM, beta1=1.0), dict(kind=h.OPT_ADAM, beta1=-0.1), dict(kind=h.OPT_ADAM, beta2=1.0),
                dict(kind=h.OPT_ADAM, beta2=-0.1), dict(clipnorm=1.0, global_clipnorm=2.0),
                dict(kind=h.OPT_ADAM, clipnorm=1.0, global_clipnorm=2.0)):
        assert step(opt(**bad)) == -1, bad
        assert lib.ssd_last_error()
    # valid descriptions get as far as the state check: there is no training state on this net (SSD_E_STATE)
    for ok in (dict(), dict(momentum=0.0), dict(momentum=1.0, nesterov=1), dict(kind=h.OPT_ADAM), dict(kind=h.OPT_ADAM, beta1=0.0),
               dict(clipnorm=1.0, clipvalue=1.0), dict(global_clipnorm=1.0), dict(kind=h.OPT_ADAM, clipvalue=0.1),
               dict(kind=h.OPT_ADAM, momentum=7.0), dict(beta1=7.0)):          # the other kind's fields are not looked at
        assert step(opt(**ok)) == -4, ok
    P = lib.ssd_net_trainable_floats(net)
    assert P > 0
    for slot in (b"m", b"v"):
        assert lib.ssd_net_optimizer_get_state(net, slot, None, 0) == P                      # the query needs no state
        assert lib.ssd_net_optimizer_get_state(net, slot, buf, 4) == -1                      # too small
        assert lib.ssd_net_optimizer_set_state(net, slot, buf, 4) == -1                      # a wrong count
        assert lib.ssd_net_optimizer_set_state(net, slot, None, P) == -1
    for slot in (b"momentum", b"", b"M"):
        assert lib.ssd_net_optimizer_get_state(net, slot, None, 0) == -1, slot
        assert slot.decode() in lib.ssd_last_error().decode()
        assert lib.ssd_net_optimizer_set_state(net, slot, buf, P) == -1, slot
    assert lib.ssd_net_optimizer_get_state(None, b"m", None, 0) == -1 and lib.ssd_net_optimizer_get_state(net, None, None, 0) == -1
    assert lib.ssd_net_optimizer_reset(None) == -1 and lib.ssd_net_optimizer_reset(net) == 0
    assert lib.ssd_net_train_set_steps(net, -1) == -1 and lib.ssd_net_train_set_steps(None, 0) == -1
    assert lib.ssd_net_train_set_steps(net, 3) == -4 and lib.ssd_net_train_steps(net) == 0


def test_adam_step_is_the_optimizer_step_under_another_signature(model):
    """``ssd_net_adam_step`` fills an ``ssd_optimizer`` and calls ``ssd_net_optimizer_step``, so its checks are that function's,
    in that function's order: NULL arguments, then the betas, then the training state.  A net that has its training state
    and a bad beta needs a device; what is reachable here is the order: a NULL net or gradient returns -1, a beta outside
    [0, 1) returns -1 although this net has no training state (the beta check does not sit behind the state check, it comes
    first), and good arguments get as far as the state check (-4)."""
    import ssd_hip as h
    lib, net = h.lib(), model._net
    buf = (ctypes.c_float * 4)()
    g = ctypes.cast(buf, ctypes.c_void_p)

    def step(net=net, g=g, b1=0.9, b2=0.999):
        return lib.ssd_net_adam_step(net, g, 1e-3, b1, b2, 1e-7, 1.0, None)
    assert step(net=None) == -1 and step(g=None) == -1 and step(net=None, g=None) == -1
    for bad in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-0.1), dict(b1=float("nan"))):
        assert step(**bad) == -1, bad
        assert b"[0, 1)" in lib.ssd_last_error()
    assert step() == -4 and step(b1=0.0, b2=0.0) == -4


# ---------------------------------------------------------------------------------------------- the trainer's switches
def test_trainer_reads_the_environment(monkeypatch):
    import optimizers
    trainer = importlib.import_module("trainer")
    names = ("OPTIMIZER", "MOMENTUM", "NESTEROV", "CLIPNORM", "CLIPVALUE", "GLOBAL_CLIPNORM")
    for n in names:
        monkeypatch.delenv("SSD_TRAINER_" + n, raising=False)
    assert trainer.optimizer_from_env() is None                          # nothing set: compile() builds the reference's Adam
    monkeypatch.setenv("SSD_TRAINER_OPTIMIZER", "sgd")
    o = trainer.optimizer_from_env()
    assert isinstance(o, optimizers.SGD) and o.momentum == 0.9 and not o.nesterov and o.learning_rate == 1e-3
    monkeypatch.setenv("SSD_TRAINER_MOMENTUM", "0.5")
    monkeypatch.setenv("SSD_TRAINER_NESTEROV", "1")
    monkeypatch.setenv("SSD_TRAINER_GLOBAL_CLIPNORM", "10")
    monkeypatch.setenv("SSD_TRAINER_CLIPVALUE", "0.5")
    o = trainer.optimizer_from_env()
    assert (o.momentum, o.nesterov, o.global_clipnorm, o.clipvalue, o.clipnorm) == (0.5, True, 10.0, 0.5, None)
    monkeypatch.setenv("SSD_TRAINER_CLIPNORM", "1")
    with pytest.raises(ValueError):
        trainer.optimizer_from_env()                                     # clipnorm and global_clipnorm
    monkeypatch.delenv("SSD_TRAINER_GLOBAL_CLIPNORM")
    monkeypatch.setenv("SSD_TRAINER_OPTIMIZER", "adam")
    o = trainer.optimizer_from_env()
    assert isinstance(o, optimizers.Adam) and (o.clipnorm, o.clipvalue) == (1.0, 0.5)
    monkeypatch.setenv("SSD_TRAINER_OPTIMIZER", "rmsprop")
    with pytest.raises(ValueError):
        trainer.optimizer_from_env()


# ---------------------------------------------------------------------------------------------- the float64 restatement
@pytest.mark.parametrize("case", oc.HAND_SGD, ids=[c[0] for c in oc.HAND_SGD])
def test_oracle_sgd_by_hand(case):
    _, var, accum, g, lr, momentum, nesterov, want_var, want_accum = case
    sentinel = object()
    got_var, got_accum = oc.sgd_update(var, sentinel if accum is None else accum, g, lr, momentum, nesterov)
    np.testing.assert_array_equal(got_var, np.array(want_var))           # (dyadic numbers: exact)
    if accum is None:
        assert got_accum is sentinel                                     # momentum 0: no accumulator is read or written
    else:
        np.testing.assert_array_equal(got_accum, np.array(want_accum))


def test_oracle_nesterov_against_the_plain_update():
    """var_nesterov - var_plain = momentum * accum_new - lr * g - accum_new, element by element; the accumulators agree."""
    rng = np.random.default_rng(5)
    var, accum, g = rng.standard_normal((3, 3))
    v_n, a_n = oc.sgd_update(var, accum, g, 0.125, 0.75, True)
    v_p, a_p = oc.sgd_update(var, accum, g, 0.125, 0.75, False)
    np.testing.assert_array_equal(a_n, a_p)
    np.testing.assert_allclose(v_n - v_p, 0.75 * a_p - 0.125 * g - a_p, rtol=0, atol=1e-15)
    assert (v_n != v_p).all()


@pytest.mark.parametrize("case", oc.HAND_CLIP, ids=[c[0] for c in oc.HAND_CLIP])
def test_oracle_clips_by_hand(case):
    name, g, kw, want = case
    got = oc.clip_gradients({"x": g}, **kw)["x"]
    if name == "norm-below":
        np.testing.assert_allclose(got, want, rtol=4 * np.finfo(np.float64).eps, atol=0)        # unchanged to rounding
    else:
        np.testing.assert_array_equal(got, np.array(want))
    assert np.isfinite(got).all()                                        # the all-zero gradient never becomes NaN


def test_oracle_global_norm_by_hand():
    grads, c, want = oc.HAND_GLOBAL
    assert oc.global_norm(list(grads.values())) == 13.0
    got = oc.clip_gradients(grads, global_clipnorm=c)
    for n in grads:
        np.testing.assert_array_equal(got[n], np.array(want[n]))
    # below the threshold the scale is c * (1 / c): the gradient to rounding; all-zero gradients stay zero
    got = oc.clip_gradients(grads, global_clipnorm=26.0)
    for n in grads:
        np.testing.assert_allclose(got[n], np.array(grads[n]), rtol=4 * np.finfo(np.float64).eps, atol=0)
    zero = oc.clip_gradients({"a": np.zeros(3), "b": np.zeros(2)}, global_clipnorm=2.0)
    assert not zero["a"].any() and not zero["b"].any() and np.isfinite(zero["a"]).all()
    with pytest.raises(ValueError):
        oc.clip_gradients(grads, clipnorm=1.0, global_clipnorm=1.0)
    # a frozen variable is simply not handed in: the norm of the rest does not see it
    assert oc.global_norm([grads["a"]]) == 5.0


def test_oracle_adam_with_a_clip_by_hand():
    c = oc.HAND_ADAM
    zeros = np.zeros(3)
    w, s = oc.step("adam", {"x": np.array(c["var"])}, {"x": {"m": zeros, "v": zeros}}, {"x": np.array(c["g"])}, 1, c["lr"],
                   beta_1=c["beta_1"], beta_2=c["beta_2"], epsilon=c["epsilon"], clipvalue=c["clipvalue"])
    np.testing.assert_array_equal(s["x"]["m"], np.array(c["want_m"]))
    np.testing.assert_array_equal(s["x"]["v"], np.array(c["want_v"]))
    np.testing.assert_allclose(w["x"], np.array(c["want_var"]), rtol=1e-15, atol=0)
    # without a clip the restatement is oracle/train_oracle.py's fp32 Adam to fp32 rounding
    from oracle import train_oracle as to
    rng = np.random.default_rng(9)
    var, g = rng.standard_normal((2, 3)).astype(np.float32)
    m, v = (0.1 * g).astype(np.float32), (0.001 * g * g).astype(np.float32)
    want = to.adam_step(var, m, v, g, 2)
    got = oc.adam_update(var, m, v, g, 2)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=5e-7, atol=0)


def test_oracle_grad_scale_comes_before_the_clip():
    """g = grads * grad_scale is what is clipped: [6, 8, 24] at scale 0.5 is [3, 4, 12], norm 13, clipped to 6.5 -> half."""
    w, s = oc.step("sgd", {"x": np.zeros(3)}, {"x": {"momentum": None}}, {"x": np.array([6.0, 8.0, 24.0])}, 1, 1.0, grad_scale=0.5,
                   clipnorm=6.5)
    np.testing.assert_array_equal(w["x"], -np.array([1.5, 2.0, 6.0]))
