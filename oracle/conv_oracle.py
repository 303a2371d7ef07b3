"""Float64 oracle of the general dense convolution (include/ssd_hip.h ``ssd_conv_desc``): ``H != W``, ``kh != kw``, four
separate pads, a stride and a dilation, NHWC x HWIO -- a plain loop over the kernel taps, no padded copy of the input and no
im2col, so that it shares no index arithmetic with oracle/net_oracle.py (which pads, then gathers columns) and none with the
kernels (which decode ``m -> (b, oy, ox)`` and ``tap -> (ky, kx)`` from flat indices).

* ``conv2d_f64``   the convolution;
* ``epilogue_f64`` what every conv kernel applies behind it: ``* scale + shift``, the activation, ``+ residual``;
* ``head_f64``     the SSD head on six feature maps as the net lays it out (models/header.py:43-67): per level a label conv
  and a box conv, 3x3 SAME with bias, reshaped to ``[B, H W A, L]`` / ``[B, H W A, 4]``, concatenated over the levels, softmax
  over the labels.

Self-tests: tests/test_conv_geometry_cpu.py (against torch's float64 conv2d, against net_oracle.conv2d, a hand-worked answer,
and five wrong restatements that the GPU bar must tell from the right one)."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2


def out_size(size, k, stride, dilation, before, after):
    """Output extent of one axis (``ssd_conv_out_size``)."""
    return (size + before + after - ((k - 1) * dilation + 1)) // stride + 1


def _tap_range(size, out, stride, off):
    """Outputs o in [0, out) whose input index o * stride + off lies in [0, size): (first, last + 1)."""
    lo = 0 if off >= 0 else (-off + stride - 1) // stride
    hi = min(out, (size - 1 - off) // stride + 1) if size - 1 - off >= 0 else 0
    return lo, max(hi, lo)


def conv2d_f64(x, w, stride=1, dilation=1, pads=(0, 0, 0, 0)):
    """x [B, H, W, Cin], w [kh, kw, Cin, Cout], pads (top, bottom, left, right) -> float64 [B, Ho, Wo, Cout]."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, H, W, Cin = x.shape
    kh, kw, wc, Cout = w.shape
    assert wc == Cin, (x.shape, w.shape)
    pt, pb, pl, pr = pads
    Ho = out_size(H, kh, stride, dilation, pt, pb)
    Wo = out_size(W, kw, stride, dilation, pl, pr)
    assert Ho >= 1 and Wo >= 1, (Ho, Wo)
    out = np.zeros((B, Ho, Wo, Cout), np.float64)
    for ky in range(kh):
        oy0, oy1 = _tap_range(H, Ho, stride, ky * dilation - pt)
        if oy1 <= oy0:
            continue
        iy0 = oy0 * stride + ky * dilation - pt
        for kx in range(kw):
            ox0, ox1 = _tap_range(W, Wo, stride, kx * dilation - pl)
            if ox1 <= ox0:
                continue
            ix0 = ox0 * stride + kx * dilation - pl
            patch = x[:, iy0:iy0 + (oy1 - oy0 - 1) * stride + 1:stride, ix0:ix0 + (ox1 - ox0 - 1) * stride + 1:stride, :]
            out[:, oy0:oy1, ox0:ox1, :] += patch @ w[ky, kx]
    return out


def epilogue_f64(y, scale=None, shift=None, act=ACT_NONE, residual=None):
    """``y * scale + shift``, activation (0 none, 1 ReLU, 2 ReLU6), ``+ residual`` -- the order of the kernels' epilogue."""
    y = np.asarray(y, np.float64)
    if scale is not None:
        y = y * np.asarray(scale, np.float64)
    if shift is not None:
        y = y + np.asarray(shift, np.float64)
    if act == ACT_RELU:
        y = np.maximum(y, 0.0)
    elif act == ACT_RELU6:
        y = np.minimum(np.maximum(y, 0.0), 6.0)
    elif act != ACT_NONE:
        raise ValueError("unknown activation %r" % (act,))
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return y


def softmax_f64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def head_f64(feats, heads, total_labels):
    """feats: the feature maps [B, H, W, C] of the levels; heads: per level (label kernel [3, 3, C, A L], label bias,
    box kernel [3, 3, C, A 4], box bias).  Returns (deltas [B, P, 4], probs [B, P, L]) in float64, P = sum H W A."""
    labels, boxes = [], []
    for f, (wl, bl, wb, bb) in zip(feats, heads):
        B = f.shape[0]
        labels.append(epilogue_f64(conv2d_f64(f, wl, 1, 1, (1, 1, 1, 1)), None, bl).reshape(B, -1, total_labels))
        boxes.append(epilogue_f64(conv2d_f64(f, wb, 1, 1, (1, 1, 1, 1)), None, bb).reshape(B, -1, 4))
    return np.concatenate(boxes, 1), softmax_f64(np.concatenate(labels, 1))
