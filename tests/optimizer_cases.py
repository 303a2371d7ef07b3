"""Float64 NumPy restatement of the optimizers of ``ssd_net_optimizer_step`` -- TF 2.x Keras semantics, [3P] restated from
the TensorFlow sources (``training_ops`` ``ApplyKerasMomentum`` / ``ApplyAdam``, ``tf.clip_by_norm``,
``tf.clip_by_global_norm``, OptimizerV2's clip order), TensorFlow itself is not executable here -- plus the
hand-computed three-element cases the restatement is held to (tests/test_optimizer_cpu.py) and the seeded gradients
the device tests share (tests/test_optimizer_gpu.py).

Conventions: ``g`` is the AVERAGED gradient ``grads_flat * grad_scale``; clipping acts on it.  A "variable" is one entry
of the parameter table (kernel, bias, gamma, beta, L2-norm scale; the label and the box kernel of a fused head conv are
two).  Everything is computed in float64 from the fp32 inputs; the hyper-parameters are taken at the fp32 value the C ABI
carries.  Frozen variables do not appear in the dicts handed in: they are not counted in any norm."""
import numpy as np

f64 = np.float64


def _f(x):
    """A hyper-parameter as the ABI carries it: rounded to fp32, then exact in float64."""
    return f64(np.float32(x))


# ---------------------------------------------------------------------------------------------- clipping
def clip_by_norm(g, c):
    """tf.clip_by_norm: s = sum(g*g); norm = sqrt(s) if s > 0 else s; (g * c) / max(norm, c).  An all-zero gradient is
    divided by c and stays zero (never 0 / 0)."""
    g = np.asarray(g, f64)
    c = _f(c)
    s = (g * g).sum()
    norm = np.sqrt(s) if s > 0 else s
    return (g * c) / max(norm, c)


def global_norm(grads):
    return np.sqrt(sum((np.asarray(g, f64) ** 2).sum() for g in grads))


def clip_by_global_norm(grads, c):
    """tf.clip_by_global_norm over a list: gn = sqrt(sum of all s); every g times c * min(1 / gn, 1 / c)."""
    c = _f(c)
    gn = global_norm(grads)
    with np.errstate(divide="ignore"):
        scale = c * min(f64(1.0) / gn, f64(1.0) / c)
    return [np.asarray(g, f64) * scale for g in grads]


def clip_by_value(g, c):
    c = _f(c)
    return np.minimum(np.maximum(np.asarray(g, f64), -c), c)


def clip_gradients(grads, clipnorm=None, clipvalue=None, global_clipnorm=None):
    """OptimizerV2's order on a dict name -> averaged gradient of the TRAINABLE variables: the norm clip (per variable, or
    global) first, the value clip second.  ``clipnorm`` and ``global_clipnorm`` exclude each other (ValueError, as Keras)."""
    if clipnorm is not None and global_clipnorm is not None:
        raise ValueError("Cannot accept both `clipnorm` and `global_clipnorm`")
    names = list(grads)
    out = [np.asarray(grads[n], f64) for n in names]
    if clipnorm is not None:
        out = [clip_by_norm(g, clipnorm) for g in out]
    if global_clipnorm is not None:
        out = clip_by_global_norm(out, global_clipnorm)
    if clipvalue is not None:
        out = [clip_by_value(g, clipvalue) for g in out]
    return dict(zip(names, out))


# ---------------------------------------------------------------------------------------------- updates
def sgd_update(var, accum, g, lr, momentum=0.0, nesterov=False):
    """ApplyKerasMomentum -> (var, accum).  momentum == 0: var -= lr * g and the accumulator is passed through untouched
    (it is neither read nor written)."""
    var, g = np.asarray(var, f64), np.asarray(g, f64)
    lr, momentum = _f(lr), _f(momentum)
    if momentum == 0:
        return var - lr * g, accum
    accum = momentum * np.asarray(accum, f64) - lr * g
    if nesterov:
        return var + (momentum * accum - lr * g), accum
    return var + accum, accum


def adam_update(var, m, v, g, t, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    """ApplyAdam (Keras Adam, non-amsgrad) at step t >= 1 -> (var, m, v)."""
    var, m, v, g = (np.asarray(a, f64) for a in (var, m, v, g))
    lr, b1, b2, eps = _f(lr), _f(beta_1), _f(beta_2), _f(epsilon)
    alpha = f64(np.float32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))
    m = m + (g - m) * (1.0 - b1)
    v = v + (g * g - v) * (1.0 - b2)
    return var - alpha * m / (np.sqrt(v) + eps), m, v


def step(kind, weights, slots, grads, t, lr, grad_scale=1.0, momentum=0.0, nesterov=False, beta_1=0.9, beta_2=0.999,
         epsilon=1e-7, clipnorm=None, clipvalue=None, global_clipnorm=None):
    """One optimizer step over dicts keyed by variable name (trainable variables only).  ``slots``: name -> {"momentum": a}
    (sgd) or {"m": a, "v": a} (adam).  Returns (weights, slots) in float64."""
    g = {n: np.asarray(grads[n], f64) * _f(grad_scale) for n in weights}
    g = clip_gradients(g, clipnorm, clipvalue, global_clipnorm)
    new_w, new_s = {}, {}
    for n in weights:
        if kind == "sgd":
            new_w[n], acc = sgd_update(weights[n], slots[n]["momentum"], g[n], lr, momentum, nesterov)
            new_s[n] = {"momentum": acc}
        elif kind == "adam":
            new_w[n], m, v = adam_update(weights[n], slots[n]["m"], slots[n]["v"], g[n], t, lr, beta_1, beta_2, epsilon)
            new_s[n] = {"m": m, "v": v}
        else:
            raise ValueError(kind)
    return new_w, new_s


# ---------------------------------------------------------------------------------------------- hand-computed cases
# Three elements each, worked with pencil and exact decimal / rational arithmetic; hyper-parameters are chosen exactly
# representable in fp32 (0.5, 0.25, 0.125, 2, ...) so that the ABI's rounding plays no part.
HAND_SGD = [
    # (name, var, accum, g, lr, momentum, nesterov, want var, want accum)
    ("plain", [1.0, -2.0, 0.5], None, [2.0, -4.0, 0.0], 0.25, 0.0, False, [0.5, -1.0, 0.5], None),
    # accum = 0.5 * [1, -1, 0] - 0.25 * [2, -4, 0] = [0, 0.5, 0]; var += accum
    ("momentum", [1.0, -2.0, 0.5], [1.0, -1.0, 0.0], [2.0, -4.0, 0.0], 0.25, 0.5, False, [1.0, -1.5, 0.5], [0.0, 0.5, 0.0]),
    # accum = 0.5 * [2, 2, -4] - 0.25 * [2, -4, 8] = [0.5, 2, -4]; var += 0.5 * accum - 0.25 * g = [-0.25, 2, -4]
    ("nesterov", [1.0, -2.0, 0.5], [2.0, 2.0, -4.0], [2.0, -4.0, 8.0], 0.25, 0.5, True, [0.75, 0.0, -3.5], [0.5, 2.0, -4.0]),
    # the same inputs without nesterov: var += accum
    ("nesterov-off", [1.0, -2.0, 0.5], [2.0, 2.0, -4.0], [2.0, -4.0, 8.0], 0.25, 0.5, False, [1.5, 0.0, -3.5], [0.5, 2.0, -4.0]),
]
HAND_CLIP = [
    # (name, g, kwargs, want)
    ("value", [3.0, -0.25, -7.0], dict(clipvalue=0.5), [0.5, -0.25, -0.5]),
    # |g| = 13 > 6.5: g * 6.5 / 13 = g / 2
    ("norm-above", [3.0, 4.0, 12.0], dict(clipnorm=6.5), [1.5, 2.0, 6.0]),
    # |g| = 13 < 26: (g * 26) / 26 = g up to rounding
    ("norm-below", [3.0, 4.0, 12.0], dict(clipnorm=26.0), [3.0, 4.0, 12.0]),
    ("norm-zero", [0.0, 0.0, 0.0], dict(clipnorm=2.0), [0.0, 0.0, 0.0]),
    # norm first (g / 2 = [1.5, 2, 6]), value second
    ("norm-then-value", [3.0, 4.0, 12.0], dict(clipnorm=6.5, clipvalue=2.0), [1.5, 2.0, 2.0]),
]
# global norm over two variables: sqrt(3^2 + 4^2 + 0 + 12^2 + 0 + 0) = 13; c = 3.25 -> scale 3.25 * min(1/13, 1/3.25) = 0.25
HAND_GLOBAL = ({"a": [3.0, 4.0, 0.0], "b": [12.0, 0.0, 0.0]}, 3.25, {"a": [0.75, 1.0, 0.0], "b": [3.0, 0.0, 0.0]})
# Adam, step 1 from zero slots with beta_1 = 0.5, beta_2 = 0.75, eps = 0, lr = 0.5: m = g / 2, v = g^2 / 4, alpha = lr *
# sqrt(1 - 0.75) / (1 - 0.5) = 0.5; var -= 0.5 * (g / 2) / (|g| / 2) = 0.5 * sign(g).  Under clipvalue 1 the slots are those
# of the clipped gradient [1, -1, 0.5]: the clip acts BEFORE the moments.
HAND_ADAM = dict(var=[1.0, 1.0, 1.0], g=[4.0, -2.0, 0.5], lr=0.5, beta_1=0.5, beta_2=0.75, epsilon=0.0, clipvalue=1.0,
                 want_var=[0.5, 1.5, 0.5], want_m=[0.5, -0.5, 0.25], want_v=[0.25, 0.25, 0.0625])


# ---------------------------------------------------------------------------------------------- device-test gradients
SCALES = (0.0, 0.01, 0.3, 3.0)


def seeded_gradients(offsets, total, seed):
    """Two flat fp32 gradients for two consecutive steps over the trainable layout ``offsets`` (name -> (offset, shape)).
    Step 1: standard normals times a per-variable scale that cycles through SCALES in table order (every fourth
    variable is all-zero); step 2: step 1 times a factor drawn from [0.5, 1.5) -- the same sign element by element, so
    neither an accumulator nor a moment cancels."""
    rng = np.random.default_rng(seed)
    g1 = np.zeros((total,), np.float32)
    for i, (name, (off, shape)) in enumerate(offsets.items()):
        n = int(np.prod(shape))
        g1[off:off + n] = (rng.standard_normal(n) * SCALES[i % len(SCALES)]).astype(np.float32)
    g2 = (g1 * rng.uniform(0.5, 1.5, total).astype(np.float32)).astype(np.float32)
    return g1, g2


def split(flat, offsets, names=None):
    """name -> the variable's slice of a flat vector, reshaped."""
    return {n: flat[off:off + int(np.prod(shape))].reshape(shape) for n, (off, shape) in offsets.items()
            if names is None or n in names}
