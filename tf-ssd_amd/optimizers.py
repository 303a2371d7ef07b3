"""``tensorflow.keras.optimizers.SGD`` / ``Adam`` as the reference's trainer imports them (reference trainer.py:4), with the
Keras signatures and defaults.  An instance only carries hyper-parameters: the slots (Adam's moments, SGD's momentum
accumulator) live in the native training state and the update is ``ssd_net_optimizer_step`` (include/ssd_hip.h has the
arithmetic), which ``SSDModel.apply_gradients`` calls with ``to_native()``.

Gradient clipping follows OptimizerV2: ``clipnorm`` (``tf.clip_by_norm`` per variable), ``global_clipnorm``
(``tf.clip_by_global_norm`` over all trainable variables; excludes ``clipnorm``), ``clipvalue`` (after the norm clip).
Not built: ``amsgrad=True`` and the legacy ``decay`` argument raise NotImplementedError."""
import ssd_hip as _h


def _number(name, value, lo=None, hi=None, hi_open=False):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, value))
    if value != value:
        raise ValueError("%s is NaN" % name)
    if lo is not None and value < lo or hi is not None and (value >= hi if hi_open else value > hi):
        raise ValueError("%s must lie in [%g, %g%s, got %r" % (name, lo, hi, ")" if hi_open else "]", value))
    return value


class Optimizer(object):
    kind = None
    name = None

    def __init__(self, learning_rate, clipnorm=None, clipvalue=None, global_clipnorm=None, **kwargs):
        if "decay" in kwargs:
            raise NotImplementedError("%s: the legacy `decay` argument is not built; pass learning_rate= per step "
                                      "(the trainer's LearningRateScheduler does)" % type(self).__name__)
        if "lr" in kwargs:
            learning_rate = kwargs.pop("lr")
        if kwargs:
            raise TypeError("%s: unexpected keyword arguments %s" % (type(self).__name__, sorted(kwargs)))
        self.learning_rate = _number("learning_rate", learning_rate, 0.0, float("inf"))
        if clipnorm is not None and global_clipnorm is not None:
            raise ValueError("Cannot accept both `clipnorm` and `global_clipnorm`, got %r and %r" % (clipnorm, global_clipnorm))
        for n, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm)):
            if v is not None:
                v = _number(n, v)
                if not 0.0 < v < float("inf"):
                    raise ValueError("%s must be a positive finite number, got %r" % (n, v))
            setattr(self, n, v)

    def _clips(self):
        return dict(clipnorm=self.clipnorm or 0.0, clipvalue=self.clipvalue or 0.0, global_clipnorm=self.global_clipnorm or 0.0)

    def get_config(self):
        raise NotImplementedError

    def to_native(self):
        """The ``struct ssd_optimizer`` of these hyper-parameters."""
        raise NotImplementedError

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % kv for kv in self.get_config().items()))


class SGD(Optimizer):
    """Keras ``SGD``: ``accum = momentum * accum - lr * g; var += accum`` (``nesterov``: ``var += momentum * accum -
    lr * g``); with ``momentum == 0`` plain ``var -= lr * g`` and no accumulator."""
    kind = _h.OPT_SGD
    name = "sgd"
    slots = ("momentum",)

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, **kwargs):
        Optimizer.__init__(self, learning_rate, clipnorm, clipvalue, global_clipnorm, **kwargs)
        self.momentum = _number("momentum", momentum, 0.0, 1.0)
        self.nesterov = bool(nesterov)

    def get_config(self):
        return dict(learning_rate=self.learning_rate, momentum=self.momentum, nesterov=self.nesterov,
                    clipnorm=self.clipnorm, clipvalue=self.clipvalue, global_clipnorm=self.global_clipnorm)

    def to_native(self):
        return _h.Optimizer(kind=self.kind, beta1=0.0, beta2=0.0, eps=0.0, momentum=self.momentum,
                            nesterov=int(self.nesterov), **self._clips())


class Adam(Optimizer):
    """Keras ``Adam`` (TF ``ApplyAdam`` form, non-amsgrad)."""
    kind = _h.OPT_ADAM
    name = "adam"
    slots = ("m", "v")

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, clipnorm=None,
                 clipvalue=None, global_clipnorm=None, **kwargs):
        if amsgrad:
            raise NotImplementedError("Adam(amsgrad=True) is not built")
        Optimizer.__init__(self, learning_rate, clipnorm, clipvalue, global_clipnorm, **kwargs)
        self.beta_1 = _number("beta_1", beta_1, 0.0, 1.0, hi_open=True)
        self.beta_2 = _number("beta_2", beta_2, 0.0, 1.0, hi_open=True)
        self.epsilon = _number("epsilon", epsilon, 0.0, float("inf"))
        self.amsgrad = False

    def get_config(self):
        return dict(learning_rate=self.learning_rate, beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon,
                    amsgrad=False, clipnorm=self.clipnorm, clipvalue=self.clipvalue, global_clipnorm=self.global_clipnorm)

    def to_native(self):
        return _h.Optimizer(kind=self.kind, beta1=self.beta_1, beta2=self.beta_2, eps=self.epsilon, momentum=0.0,
                            nesterov=0, **self._clips())


def get(identifier, **adam_kwargs):
    """What ``SSDModel.compile(optimizer=...)`` accepts: an instance, ``"sgd"`` / ``"adam"`` (Keras defaults), or None --
    Adam from the keyword arguments.  Anything else raises TypeError."""
    if identifier is None:
        return Adam(**adam_kwargs)
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str) and identifier.lower() in ("sgd", "adam"):
        return SGD() if identifier.lower() == "sgd" else Adam()
    raise TypeError("optimizer must be an optimizers.SGD / optimizers.Adam instance, 'sgd', 'adam' or None, got %r" % (identifier,))
