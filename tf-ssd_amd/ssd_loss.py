"""Drop-in for the reference's ``ssd_loss.py``: ``CustomLoss`` with
``loc_loss_fn`` / ``conf_loss_fn``.  Both terms are evaluated by ONE HIP kernel per image
(``ssd_loss`` in include/ssd_hip.h, csrc/ssd_loss.hip): Huber over the positives, categorical
cross-entropy on renormalised + clipped probabilities, 3:1 hard-negative mining through a
radix select of the loss rank, per-image normalisation.  No torch math on this path.

``FocalLoss`` has the same surface with Keras' ``CategoricalFocalCrossentropy(alpha, gamma)`` in place of the mining
(``ssd_focal_loss``, csrc/ssd_focal.hip: parallel over anchors, every anchor counts).

``IoULocLoss`` puts an IoU-family loss on the decoded boxes (IoU / GIoU / DIoU / CIoU: ``ssd_iou_loc_loss``,
csrc/ssd_iouloss.hip) in place of the Huber term of either of the two; the confidence term stays theirs."""
import ctypes

import numpy as np
import torch

import ssd_hip as _h


class CustomLoss(object):
    """reference ssd_loss.py:3-65."""

    def __init__(self, neg_pos_ratio, loc_loss_alpha):
        self.neg_pos_ratio = float(neg_pos_ratio)
        self.loc_loss_alpha = float(loc_loss_alpha)
        self.last_final_mask = None        # diagnostics: the reference's final_mask of the last conf call
        self.last_cross_entropy = None

    def _run(self, yd, pd, yl, pl, want_aux=False, want_grads=False, grad_scale=1.0):
        ref = pd if pd is not None else pl
        B, N = ref.shape[0], ref.shape[1]
        L = pl.shape[2] if pl is not None else 1
        dev = ref.device
        lib = _h.lib()
        loc = torch.empty((B,), dtype=torch.float32, device=dev) if pd is not None else None
        conf = torch.empty((B,), dtype=torch.float32, device=dev) if pl is not None else None
        ce = torch.empty((B, N), dtype=torch.float32, device=dev) if (want_aux and pl is not None) else None
        mask = torch.empty((B, N), dtype=torch.float32, device=dev) if (want_aux and pl is not None) else None
        gd = torch.empty_like(pd) if (want_grads and pd is not None) else None
        gz = torch.empty_like(pl) if (want_grads and pl is not None) else None
        ws = _h.workspace(lib.ssd_loss_workspace_bytes(B, N))
        _h.check(lib.ssd_loss(_h.ptr(yd), _h.ptr(pd), _h.ptr(yl), _h.ptr(pl), B, N, L, self.neg_pos_ratio,
                              self.loc_loss_alpha, _h.ptr(loc), _h.ptr(conf), _h.ptr(ce), _h.ptr(mask), _h.ptr(gd),
                              _h.ptr(gz), float(grad_scale), _h.ptr(ws), ws.numel(), _h.stream()), "ssd_loss")
        return loc, conf, ce, mask, gd, gz

    def to_native(self):
        """The ``ssd_loss_config`` of a training step compiled with this loss."""
        return _h.LossConfig(_h.LOSS_HARD_NEGATIVE, self.neg_pos_ratio, self.loc_loss_alpha, 0.25, 2.0)

    @staticmethod
    def _pair(actual, pred, last):
        a, p = _h.to_dev(actual), _h.to_dev(pred)
        if a.dim() != 3 or a.shape != p.shape or (last and a.shape[2] != last):
            raise ValueError("bad shapes %s / %s" % (tuple(a.shape), tuple(p.shape)))
        return a, p

    def loc_loss_fn(self, actual_deltas, pred_deltas):
        """reference ssd_loss.py:8-33 -> loc_loss [B]."""
        yd, pd = self._pair(actual_deltas, pred_deltas, 4)
        return self._run(yd, pd, None, None)[0]

    def conf_loss_fn(self, actual_labels, pred_labels):
        """reference ssd_loss.py:35-65 -> conf_loss [B]."""
        yl, pl = self._pair(actual_labels, pred_labels, 0)
        _, conf, ce, mask, _, _ = self._run(None, None, yl, pl, want_aux=True)
        self.last_cross_entropy, self.last_final_mask = ce, mask
        return conf

    def loss_and_grads(self, actual_deltas, actual_labels, pred_deltas, pred_labels, grad_scale=None):
        """Both terms + the gradients of the Keras objective mean_b(loc_b + conf_b) w.r.t. the
        predicted deltas and the softmax LOGITS (what the training step back-propagates)."""
        yd, pd = self._pair(actual_deltas, pred_deltas, 4)
        yl, pl = self._pair(actual_labels, pred_labels, 0)
        gs = 1.0 / pd.shape[0] if grad_scale is None else grad_scale
        loc, conf, _, _, gd, gz = self._run(yd, pd, yl, pl, want_grads=True, grad_scale=gs)
        return loc, conf, gd, gz


def _number(name, value, lo, lo_open=False):
    """A finite float >= lo (> lo with ``lo_open``), refused the way ``optimizers._number`` refuses."""
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, value))
    if value != value:
        raise ValueError("%s is NaN" % name)
    if value == float("inf") or (value <= lo if lo_open else value < lo):
        raise ValueError("%s must lie in %s%g, inf), got %r" % (name, "(" if lo_open else "[", lo, value))
    return value


class FocalLoss(CustomLoss):
    """The localisation term of ``CustomLoss`` and, for the confidence term, Keras'
    ``CategoricalFocalCrossentropy(alpha=0.25, gamma=2.0)`` summed over ALL anchors of an image and divided by its
    positive count (1 when it has none): no mining, ``last_final_mask`` is all ones and ``last_cross_entropy`` the
    per-anchor focal value.  include/ssd_hip.h (``ssd_focal_loss``) states the arithmetic."""

    def __init__(self, loc_loss_alpha, alpha=0.25, gamma=2.0):
        self.loc_loss_alpha = _number("loc_loss_alpha", loc_loss_alpha, 0.0)
        self.alpha = _number("alpha", alpha, 0.0, lo_open=True)
        self.gamma = _number("gamma", gamma, 0.0)
        self.last_final_mask = None
        self.last_cross_entropy = None

    def get_config(self):
        return {"loc_loss_alpha": self.loc_loss_alpha, "alpha": self.alpha, "gamma": self.gamma}

    def __repr__(self):
        return "FocalLoss(loc_loss_alpha=%g, alpha=%g, gamma=%g)" % (self.loc_loss_alpha, self.alpha, self.gamma)

    def to_native(self):
        return _h.LossConfig(_h.LOSS_FOCAL, 0.0, self.loc_loss_alpha, self.alpha, self.gamma)

    def _run(self, yd, pd, yl, pl, want_aux=False, want_grads=False, grad_scale=1.0):
        ref = pd if pd is not None else pl
        B, N = ref.shape[0], ref.shape[1]
        L = pl.shape[2] if pl is not None else 1
        dev = ref.device
        lib = _h.lib()
        loc = torch.empty((B,), dtype=torch.float32, device=dev) if pd is not None else None
        conf = torch.empty((B,), dtype=torch.float32, device=dev) if pl is not None else None
        ce = torch.empty((B, N), dtype=torch.float32, device=dev) if (want_aux and pl is not None) else None
        mask = torch.empty((B, N), dtype=torch.float32, device=dev) if (want_aux and pl is not None) else None
        gd = torch.empty_like(pd) if (want_grads and pd is not None) else None
        gz = torch.empty_like(pl) if (want_grads and pl is not None) else None
        ws = _h.workspace(lib.ssd_focal_loss_workspace_bytes(B, N, L))
        _h.check(lib.ssd_focal_loss(_h.ptr(yd), _h.ptr(pd), _h.ptr(yl), _h.ptr(pl), B, N, L, self.loc_loss_alpha, self.alpha,
                                    self.gamma, _h.ptr(loc), _h.ptr(conf), _h.ptr(ce), _h.ptr(mask), _h.ptr(gd), _h.ptr(gz),
                                    float(grad_scale), _h.ptr(ws), ws.numel(), _h.stream()), "ssd_focal_loss")
        return loc, conf, ce, mask, gd, gz


LOC_MODES = {"iou": _h.LOC_IOU, "giou": _h.LOC_GIOU, "diou": _h.LOC_DIOU, "ciou": _h.LOC_CIOU}


class IoULocLoss(object):
    """``conf_loss`` (a ``CustomLoss`` or a ``FocalLoss``) with its Huber localisation term replaced by an IoU-family loss
    between the boxes decoded from the actual and from the predicted deltas: ``mode`` = ``iou`` | ``giou`` | ``diou`` |
    ``ciou``, the definitions of ``torchvision.ops`` with boxes in (y1, x1, y2, x2) order; include/ssd_hip.h
    (``ssd_iou_loc_loss``) states the arithmetic.  ``prior_boxes`` [N,4] and ``variances`` [4] are what the decoder uses;
    the prior tensor is kept alive on the device.  ``conf_loss`` supplies ``loc_loss_alpha`` and the confidence term
    (``last_final_mask`` / ``last_cross_entropy`` are its own); ``last_box_loss`` is the per-anchor value of the last
    ``loc_loss_fn`` call (0 where the anchor is not positive)."""

    def __init__(self, conf_loss, prior_boxes, variances, mode="ciou"):
        if not isinstance(conf_loss, CustomLoss):
            raise TypeError("conf_loss must be a CustomLoss or a FocalLoss, got %r" % (conf_loss,))
        key = mode.strip().lower() if isinstance(mode, str) else mode
        if key not in LOC_MODES:
            raise ValueError("mode must be one of %s, got %r" % (", ".join(sorted(LOC_MODES)), mode))
        try:
            var = [float(v) for v in variances]
        except (TypeError, ValueError):
            raise ValueError("variances must be four numbers, got %r" % (variances,))
        if len(var) != 4 or not all(0.0 < v < float("inf") for v in var):
            raise ValueError("variances must be four finite numbers > 0, got %r" % (variances,))
        if isinstance(prior_boxes, torch.Tensor):
            priors = prior_boxes.detach().to(torch.float32).contiguous()
        else:
            try:
                priors = torch.from_numpy(np.array(prior_boxes, np.float32))
            except (TypeError, ValueError):
                raise ValueError("prior_boxes must be an [N,4] array, got %r" % (prior_boxes,))
        if priors.dim() != 2 or priors.shape[1] != 4 or priors.shape[0] < 1:
            raise ValueError("prior_boxes must be [N,4], got %s" % (tuple(priors.shape),))
        self.conf_loss = conf_loss
        self.mode = key
        self.variances = var
        self.loc_loss_alpha = conf_loss.loc_loss_alpha
        if hasattr(conf_loss, "neg_pos_ratio"):
            self.neg_pos_ratio = conf_loss.neg_pos_ratio
        self._priors = priors            # as given
        self._on_device = {}             # device -> the tensor there (priors_dev)
        self._var = (ctypes.c_float * 4)(*var)
        self.last_box_loss = None

    @property
    def last_final_mask(self):
        return self.conf_loss.last_final_mask

    @property
    def last_cross_entropy(self):
        return self.conf_loss.last_cross_entropy

    @property
    def num_priors(self):
        return int(self._priors.shape[0])

    def get_config(self):
        base = self.conf_loss
        conf = dict(base.get_config()) if isinstance(base, FocalLoss) else {"neg_pos_ratio": base.neg_pos_ratio,
                                                                             "loc_loss_alpha": base.loc_loss_alpha}
        conf["class"] = type(base).__name__
        return {"mode": self.mode, "variances": list(self.variances), "num_priors": self.num_priors, "conf_loss": conf}

    def __repr__(self):
        base = repr(self.conf_loss) if isinstance(self.conf_loss, FocalLoss) else "CustomLoss(neg_pos_ratio=%g, loc_loss_alpha=%g)" % (
            self.conf_loss.neg_pos_ratio, self.conf_loss.loc_loss_alpha)
        return "IoULocLoss(%s, priors=%d, variances=[%s], mode=%s)" % (
            base, self.num_priors, ", ".join("%g" % v for v in self.variances), self.mode)

    def priors_dev(self):
        """The prior tensor on the current device: uploaded once per device and kept for this object's lifetime, because a
        compiled model holds its bare pointer (``to_native``)."""
        dev = _h.device()
        if dev not in self._on_device:
            self._on_device[dev] = self._priors if self._priors.device == dev else self._priors.to(dev).contiguous()
        return self._on_device[dev]

    def to_native(self):
        """The ``ssd_loss_config`` of a training step compiled with this loss: the base's, with the localisation kind, the
        device priors (NULL while no device is visible: the training step refuses that) and the variances appended."""
        cfg = self.conf_loss.to_native()
        cfg.loc_kind = LOC_MODES[self.mode]
        cfg.priors_dev = self.priors_dev().data_ptr() if torch.cuda.is_available() else None
        cfg.variances = self._var
        return cfg

    def _run(self, yd, pd, want_grads=False, grad_scale=1.0):
        B, N = pd.shape[0], pd.shape[1]
        if N != self.num_priors:
            raise ValueError("%d anchors against %d prior boxes" % (N, self.num_priors))
        lib = _h.lib()
        priors = self.priors_dev()
        loc = torch.empty((B,), dtype=torch.float32, device=pd.device)
        box = torch.empty((B, N), dtype=torch.float32, device=pd.device)
        gd = torch.empty_like(pd) if want_grads else None
        ws = _h.workspace(lib.ssd_iou_loc_loss_workspace_bytes(B, N))
        _h.check(lib.ssd_iou_loc_loss(_h.ptr(priors), self._var, _h.ptr(yd), _h.ptr(pd), B, N, LOC_MODES[self.mode],
                                      self.loc_loss_alpha, _h.ptr(loc), _h.ptr(box), _h.ptr(gd), float(grad_scale), _h.ptr(ws),
                                      ws.numel(), _h.stream()), "ssd_iou_loc_loss")
        return loc, box, gd

    def loc_loss_fn(self, actual_deltas, pred_deltas):
        """-> loc_loss [B]: ``loc_loss_alpha`` times the mean of the per-anchor loss over the image's positives."""
        yd, pd = CustomLoss._pair(actual_deltas, pred_deltas, 4)
        loc, self.last_box_loss, _ = self._run(yd, pd)
        return loc

    def conf_loss_fn(self, actual_labels, pred_labels):
        """The base's confidence term -> conf_loss [B]."""
        return self.conf_loss.conf_loss_fn(actual_labels, pred_labels)

    def loss_and_grads(self, actual_deltas, actual_labels, pred_deltas, pred_labels, grad_scale=None):
        """Both terms + the gradients of mean_b(loc_b + conf_b) w.r.t. the predicted deltas (through the decode) and the
        softmax LOGITS: the base's confidence kernel on the labels alone, then ``ssd_iou_loc_loss``."""
        yd, pd = CustomLoss._pair(actual_deltas, pred_deltas, 4)
        yl, pl = CustomLoss._pair(actual_labels, pred_labels, 0)
        gs = 1.0 / pd.shape[0] if grad_scale is None else grad_scale
        _, conf, _, _, _, gz = self.conf_loss._run(None, None, yl, pl, want_grads=True, grad_scale=gs)
        loc, _, gd = self._run(yd, pd, want_grads=True, grad_scale=gs)
        return loc, conf, gd, gz
