"""TEST INFRASTRUCTURE ONLY -- teacher-forced float64 backward (and forward) of ONE layer at a time.

The end-to-end gradient checks (tests/test_train.py) let ~50 layers of fp32 error accumulate and can
only bound a tensor's error against its largest entry.  Here every layer's backward is recomputed in
float64 from the OTHER implementation's own tensors -- the layer's input activation, its ``pre`` /
``mean`` / ``var`` (BatchNorm layers), the gradient of its output tensor and its weights -- so that no
error travels from layer to layer and every ELEMENT can be held to the a-priori fp32 bound.

The metric.  For a compared element

    E = |got - ref64| / (u * A),        u = 2^-24,

where A is the sum of the absolute values of the terms that make the element up: the same formula
with every factor replaced by its absolute value and every subtraction by an addition, propagated
through the layer exactly as the value is (``layer_backward(..., absolute=True)``).  The fp32 error
bound of a sum of K products is E <= K + c; a correct kernel in any summation order sits near 1
(rounding errors walk randomly), a dropped / duplicated / misplaced term of typical size near
1 / (K u).  The bar is ``E_BAR`` = 16; elements with A == 0 must match exactly.

A "layer" is what the training step treats as one: conv (or depthwise conv) + BatchNorm (batch
statistics) + ReLU6 [+ residual add], conv + bias + ReLU, a head conv pair, max-pool, L2
normalisation.  Non-differentiable choices (ReLU / ReLU6 pass-masks, max-pool arg-max ties) come
from the checked implementation's own activations.

Every formula below is written once, generic in the torch dtype: ``dtype=torch.float64`` is the
oracle, ``dtype=torch.float32`` the plain fp32 restatement tests/test_layer_grad_cpu.py measures the
floor of the metric with.  Measured worst E of that fp32 restatement against the float64 oracle
(tests/test_layer_grad_cpu.py, tiny random layers, torch-CPU on one thread; the figures follow the BLAS's summation
order and move by a few tenths from host to host):

    dense 3x3 s1 2.4   dense 3x3 s2 2.7   dense 3x3 dilated 3.0   1x1 1.4   depthwise s1 1.2
    depthwise s2 correct_pad 2.0   BN + ReLU6 1.1   BN + residual 1.2   bias + ReLU 2.0
    max-pool 2/2 0.0   max-pool 3/1 SAME 1.7   L2-norm 3.8

The FORWARD of the same layers is held the same way (``layer_forward`` / ``check_forward_graph``: each output from the
other implementation's own input tensor; a BatchNorm layer's ``out`` from its own ``pre`` / ``mean`` / ``var``, so that
neither the conv's nor the statistics' error reaches it).  The fp32 restatement's worst E there
(tests/test_layer_forward_cpu.py, same conditions), ``pre`` / ``out``:

    dense 3x3 s1 - / 2.1   dense 3x3 s2 - / 1.7   dense 3x3 dilated - / 1.6   1x1 + BN 2.3 / 2.3
    depthwise s1 + BN + ReLU6 2.3 / 1.6   depthwise s2 correct_pad 2.0 / 2.2   1x1 + BN + ReLU6 2.5 / 2.4
    1x1 + BN + residual 2.8 / 1.9   1x1 bias + ReLU - / 2.1   frozen BN + ReLU6 + residual - / 1.6
    max-pools 0.0 (bit for bit)   L2-norm 3.3   head deltas 1.1, probs 0.6
and of six subtly wrong forwards built from the reference formulas alone (each has to exceed 4 x E_BAR = 64):
    tap skipped at the last output column: pre 4.5e6      both operands cut to 16 significand bits: pre 291 (K = 144),
    deltas 282, probs 101 (K = 288)      istd without eps: out 1.4e4      residual added before the activation: out 1.4e7
    ReLU in place of ReLU6: out 8.3e6      head halves swapped at the split column: probs 3.6e9, deltas 2.9e7

Beside the max of E, ``e_stats`` / ``Report`` carry its root mean square over the compared elements with A > 0: at long K
(the inference graphs reach 9216) operands rounded to 16 significand bits score a max E below 16, while the RMS keeps a
factor >= 37 over the fp32 restatement's.  ``forward_yardstick`` gives both reference-only yardsticks of a dense conv or head
on the input of the comparison (tests/test_layer_infer_cpu.py, tests/test_layer_infer_gpu.py).

Layouts: activations NHWC, kernels HWIO, depthwise kernels [3,3,C,1] (Keras).  Only tests/ imports
this module."""
import numpy as np
import torch

from oracle import net_oracle as no

U = 2.0 ** -24
E_BAR = 16.0
BN_EPS = no.BN_EPS
BN_MOMENTUM = 0.999
L2_REG = 5e-4       # VGG16: kernel_regularizer=l2(5e-4) on the backbone / extra convs (not on the heads)


# ------------------------------------------------------------------ graph description
def _pads(spec, H, W):
    k, s, d = spec["k"], spec["stride"], spec.get("dil", 1)
    if spec["pad"] == "same":
        _, pt, pb = no.same_pads(H, k, s, d)
        _, pl, pr = no.same_pads(W, k, s, d)
    elif spec["pad"] == "correct":
        pt, pb = no.correct_pad(H, k)
        pl, pr = no.correct_pad(W, k)
    elif spec["pad"] == "valid":
        pt = pb = pl = pr = 0
    else:
        pt, pb, pl, pr = spec["pad"]
    return pt, pb, pl, pr


def _conv(name, tin, tout, k=1, stride=1, pad="same", dil=1, bn=None, bias=False, act=None, res=None, kind="conv"):
    return dict(kind=kind, name=name, tin=tin, tout=tout, k=k, stride=stride, pad=pad, dil=dil, bn=bn, bias=bias,
                act=act, res=res)


def head_specs(hyper_params, feats):
    L = hyper_params["total_labels"]
    out = []
    for i, (f, ars) in enumerate(zip(feats, hyper_params["aspect_ratios"]), start=1):
        out.append(dict(kind="head", name="%d_conv_heads" % i, tin=f, tout=None, k=3, stride=1, pad="same", dil=1,
                        level=i - 1, anchors=len(ars) + 1, labels=L))
    return out


def mobilenet_v2_layers(hyper_params):
    """The MobileNetV2-SSD training graph, one entry per layer of the training step, in forward order
    (oracle/net_oracle.py:mobilenet_v2_ssd_forward)."""
    Ls = [_conv("Conv1", "input", "Conv1_relu", 3, 2, "correct", bn="bn_Conv1", act="relu6"),
          _conv("expanded_conv_depthwise", "Conv1_relu", "expanded_conv_depthwise_relu", 3, 1, "same",
                bn="expanded_conv_depthwise_BN", act="relu6", kind="dw"),
          _conv("expanded_conv_project", "expanded_conv_depthwise_relu", "expanded_conv_project_BN",
                bn="expanded_conv_project_BN")]
    x, cin = "expanded_conv_project_BN", 16
    for k, (cout, s) in enumerate(no._MBV2_BLOCKS, start=1):
        p = "block_%d_" % k
        Ls.append(_conv(p + "expand", x, p + "expand_relu", bn=p + "expand_BN", act="relu6"))
        Ls.append(_conv(p + "depthwise", p + "expand_relu", p + "depthwise_relu", 3, s, "correct" if s == 2 else "same",
                        bn=p + "depthwise_BN", act="relu6", kind="dw"))
        Ls.append(_conv(p + "project", p + "depthwise_relu", p + "out", bn=p + "project_BN",
                        res=x if (cin == cout and s == 1) else None))
        x, cin = p + "out", cout
    Ls.append(_conv("Conv_1", x, "out_relu", bn="Conv_1_bn", act="relu6"))
    feats, x = ["block_13_expand_relu", "out_relu"], "out_relu"
    for i in range(1, 5):
        Ls.append(_conv("extra%d_1" % i, x, "extra%d_1" % i, 1, 1, "valid", bias=True, act="relu"))
        Ls.append(_conv("extra%d_2" % i, "extra%d_1" % i, "extra%d_2" % i, 3, 2, "same", bias=True, act="relu"))
        x = "extra%d_2" % i
        feats.append(x)
    return Ls + head_specs(hyper_params, feats)


def vgg16_layers(hyper_params):
    """The VGG16-SSD training graph (oracle/net_oracle.py:vgg16_ssd_forward)."""
    Ls, x = [], "input"

    def c(name, k=3, stride=1, pad="same", dil=1):
        nonlocal x
        Ls.append(dict(_conv(name, x, name, k, stride, pad, dil, bias=True, act="relu"), l2=L2_REG))
        x = name

    def pool(name, k, stride):
        nonlocal x
        Ls.append(dict(kind="pool", name=name, tin=x, tout=name, k=k, stride=stride, pad="same"))
        x = name
    c("conv1_1"); c("conv1_2"); pool("pool1", 2, 2)
    c("conv2_1"); c("conv2_2"); pool("pool2", 2, 2)
    c("conv3_1"); c("conv3_2"); c("conv3_3"); pool("pool3", 2, 2)
    c("conv4_1"); c("conv4_2"); c("conv4_3"); pool("pool4", 2, 2)
    c("conv5_1"); c("conv5_2"); c("conv5_3"); pool("pool5", 3, 1)
    c("conv6", dil=6); c("conv7", k=1)
    c("conv8_1", 1, 1, "valid"); c("conv8_2", 3, 2, "same")
    c("conv9_1", 1, 1, "valid"); c("conv9_2", 3, 2, "same")
    c("conv10_1", 1, 1, "valid"); c("conv10_2", 3, 1, "valid")
    c("conv11_1", 1, 1, "valid"); c("conv11_2", 3, 1, "valid")
    Ls.append(dict(kind="l2norm", name="l2_normalization", tin="conv4_3", tout="l2_normalization"))
    return Ls + head_specs(hyper_params, ["l2_normalization", "conv7", "conv8_2", "conv9_2", "conv10_2", "conv11_2"])


def layers(backbone, hyper_params):
    return mobilenet_v2_layers(hyper_params) if backbone == "mobilenet_v2" else vgg16_layers(hyper_params)


def tensor_shapes(specs, weights, S=300):
    """{tensor or "pre:<layer>": (H, W, C)} of a graph description at input size S."""
    shapes = {"input": (S, S, 3)}
    for s in specs:
        H, W, C = shapes[s["tin"]]
        if s["kind"] in ("l2norm", "head"):
            out = (H, W, C)
        elif s["kind"] == "conv":
            out = out_hw(s, H, W) + (weights[s["name"] + "/kernel"].shape[3],)
        else:
            out = out_hw(s, H, W) + (C,)
        if s["tout"]:
            shapes[s["tout"]] = out
        shapes["pre:" + s["name"]] = out
    return shapes


def layer_kind(spec):
    """The class a layer's worst E is reported under."""
    if spec["kind"] in ("pool", "l2norm", "head"):
        return spec["kind"] if spec["kind"] != "pool" else "pool%d/%d" % (spec["k"], spec["stride"])
    tail = "bn+res" if spec["res"] else ("bn+" + spec["act"] if spec["bn"] and spec["act"] else
                                         ("bn" if spec["bn"] else "bias+relu"))
    if spec["kind"] == "dw":
        return "dw s%d %s" % (spec["stride"], tail)
    return "conv %dx%d s%d%s %s" % (spec["k"], spec["k"], spec["stride"], " d%d" % spec["dil"] if spec["dil"] > 1 else "", tail)


# ------------------------------------------------------------------ the linear parts (any dtype)
def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def conv_backward(x, w, g, stride, dil, pads, need_dx=True, round_dx=None):
    """dX, dW of out = conv2d(x NHWC, w HWIO) under the upstream gradient g [B,Ho,Wo,Cout]: per tap one
    GEMM each (dW[tap] = X_tap^T G, dXpad[tap window] += G W[tap]^T).  round_dx (e.g. ``bf16_rne``) rounds the two
    operands of the DATA gradient, g and w, before they are multiplied (dW keeps the unrounded g)."""
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    pt, pb, pl, pr = pads
    Ho, Wo = g.shape[1], g.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    dxp = torch.zeros_like(xp) if need_dx else None
    dw = torch.empty_like(w)
    g2 = g.reshape(-1, Cout)
    gq, wq = (round_dx(g2).to(g.dtype), round_dx(w).to(w.dtype)) if round_dx and need_dx else (g2, w)
    for ky in range(kh):
        for kx in range(kw):
            ys, xs = ky * dil, kx * dil
            sl = (slice(None), slice(ys, ys + (Ho - 1) * stride + 1, stride), slice(xs, xs + (Wo - 1) * stride + 1, stride))
            dw[ky, kx] = xp[sl].reshape(-1, Cin).t() @ g2
            if need_dx:
                dxp[sl] += (gq @ wq[ky, kx].t()).reshape(B, Ho, Wo, Cin)
    dx = dxp[:, pt:pt + H, pl:pl + W] if need_dx else None
    return dx, dw


def depthwise_backward(x, w, g, stride, pads):
    """dX, dW of the 3x3 depthwise conv (w [3,3,C,1])."""
    B, H, W, C = x.shape
    pt, pb, pl, pr = pads
    Ho, Wo = g.shape[1], g.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    dxp = torch.zeros_like(xp)
    dw = torch.empty_like(w)
    for ky in range(3):
        for kx in range(3):
            sl = (slice(None), slice(ky, ky + (Ho - 1) * stride + 1, stride), slice(kx, kx + (Wo - 1) * stride + 1, stride))
            dw[ky, kx, :, 0] = (xp[sl] * g).sum((0, 1, 2))
            dxp[sl] += g * w[ky, kx, :, 0]
    return dxp[:, pt:pt + H, pl:pl + W], dw


def out_hw(spec, H, W):
    pt, pb, pl, pr = _pads(spec, H, W)
    keff = (spec["k"] - 1) * spec.get("dil", 1) + 1
    return (H + pt + pb - keff) // spec["stride"] + 1, (W + pl + pr - keff) // spec["stride"] + 1


def pool_windows(x, spec):
    """[k*k, B, Ho, Wo, C] window cells of the SAME max-pool (padded cells -inf) and the pads."""
    B, H, W, C = x.shape
    k, s = spec["k"], spec["stride"]
    pt, pb, pl, pr = _pads(spec, H, W)
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb), value=float("-inf"))
    Ho, Wo = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    cells = [xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] for ky in range(k) for kx in range(k)]
    return torch.stack(cells), (pt, pb, pl, pr), (Ho, Wo)


def pool_backward(x, g, spec):
    """dX of the max-pool (an input cell receives dY of every window whose FIRST maximum in row-major
    order it is) and ``tied``: input cells that share the maximum of some window with another cell --
    which of them receives the gradient is a convention, so the elementwise comparison leaves them out."""
    B, H, W, C = x.shape
    k, s = spec["k"], spec["stride"]
    cells, (pt, pb, pl, pr), (Ho, Wo) = pool_windows(x, spec)
    mx = cells.max(0).values
    ismax = cells == mx
    first = ismax & (ismax.cumsum(0) == 1)
    tie = ismax & (ismax.sum(0) > 1)
    dxp = torch.zeros((B, H + pt + pb, W + pl + pr, C), dtype=g.dtype)
    tp = torch.zeros((B, H + pt + pb, W + pl + pr, C), dtype=torch.bool)
    i = 0
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + (Ho - 1) * s + 1, s), slice(kx, kx + (Wo - 1) * s + 1, s))
            dxp[sl] += g * first[i]
            tp[sl] |= tie[i]
            i += 1
    return dxp[:, pt:pt + H, pl:pl + W], tp[:, pt:pt + H, pl:pl + W]


# ------------------------------------------------------------------ one layer
def layer_backward(spec, t, dtype=torch.float64, absolute=False, round_dx=None):
    """Local backward of one layer.  ``t``: dict of arrays -- x (input activation), dout (gradient of the
    output tensor) and, by kind, out (output activation: pass-masks), pre / mean / var (BatchNorm), w, gamma,
    w_label / w_box / g_label / g_box (head).  Returns {key: tensor}: "dx" (this layer's CONTRIBUTION to the
    gradient of its input), "dres" (to the residual tensor), "dw", "dgamma", "dbeta", "dbias", "dw_label", ... .
    absolute=True returns A, the absolute-value sum of each element's terms."""
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    sub = (lambda a, b: a + b) if absolute else (lambda a, b: a - b)
    kind = spec["kind"]
    x = ab(_t(t["x"], dtype))
    r = {}
    if kind == "pool":
        r["dx"], r["tied"] = pool_backward(_t(t["x"], dtype), ab(_t(t["dout"], dtype)), spec)
        return r
    if kind == "l2norm":
        xs = _t(t["x"], dtype)
        g, gamma = ab(_t(t["dout"], dtype)), ab(_t(t["gamma"], dtype))
        rs = torch.rsqrt(torch.clamp((xs * xs).sum(-1, keepdim=True), min=1e-12))          # >= 0: the same in A
        r["dgamma"] = (g * x * rs).sum((0, 1, 2))
        r["dx"] = sub(gamma * rs * g, x * rs ** 3 * (gamma * g * x).sum(-1, keepdim=True))
        return r
    pads = _pads(spec, x.shape[1], x.shape[2])
    if kind == "head":
        for part in ("label", "box"):
            w, g = ab(_t(t["w_" + part], dtype)), ab(_t(t["g_" + part], dtype))
            dx, r["dw_" + part] = conv_backward(x, w, g, 1, 1, pads, round_dx=round_dx)
            r["dx"] = dx if "dx" not in r else r["dx"] + dx
            r["dbias_" + part] = g.sum((0, 1, 2))
        return r
    w = ab(_t(t["w"], dtype))
    dout = ab(_t(t["dout"], dtype))
    if spec["res"]:
        r["dres"] = dout
    if spec["act"]:
        out = _t(t["out"], dtype)
        mask = (out > 0) & (out < 6) if spec["act"] == "relu6" else out > 0
        dz = dout * mask
    else:
        dz = dout
    if spec["bn"]:
        M = dz.shape[0] * dz.shape[1] * dz.shape[2]
        gamma, mean = ab(_t(t["gamma"], dtype)), ab(_t(t["mean"], dtype))
        istd = torch.rsqrt(_t(t["var"], dtype) + BN_EPS)
        xh = sub(ab(_t(t["pre"], dtype)), mean) * istd
        r["dbeta"] = dz.sum((0, 1, 2))
        r["dgamma"] = (dz * xh).sum((0, 1, 2))
        dpre = gamma * istd * sub(sub(dz, r["dbeta"] / M), xh * (r["dgamma"] / M))
    else:
        dpre = dz
        if spec["bias"]:
            r["dbias"] = dz.sum((0, 1, 2))
    if kind == "dw":
        r["dx"], r["dw"] = depthwise_backward(x, w, dpre, spec["stride"], pads)
    else:
        r["dx"], r["dw"] = conv_backward(x, w, dpre, spec["stride"], spec["dil"], pads,
                                         need_dx=spec["tin"] != "input", round_dx=round_dx)
        if r["dx"] is None:
            del r["dx"]
    if spec.get("l2"):           # kernel_regularizer=l2(c): d(c sum w^2)/dw = 2 c w
        r["dw"] = r["dw"] + 2.0 * spec["l2"] * w
    return r


# ------------------------------------------------------------------ one layer, forward
def conv_forward(x, w, stride, dil, pads, round_ops=None):
    """conv2d(x NHWC, w HWIO): per tap one GEMM.  round_ops (e.g. ``bf16_rne``) rounds BOTH operands once before they
    are multiplied (the bf16 mode's rule, as conv_backward(round_dx=...) states it for the data gradient)."""
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    pt, pb, pl, pr = pads
    if round_ops:
        x, w = round_ops(x).to(x.dtype), round_ops(w).to(w.dtype)
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    Ho = (H + pt + pb - ((kh - 1) * dil + 1)) // stride + 1
    Wo = (W + pl + pr - ((kw - 1) * dil + 1)) // stride + 1
    out = torch.zeros((B * Ho * Wo, Cout), dtype=x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            ys, xs = ky * dil, kx * dil
            sl = (slice(None), slice(ys, ys + (Ho - 1) * stride + 1, stride), slice(xs, xs + (Wo - 1) * stride + 1, stride))
            out += xp[sl].reshape(-1, Cin) @ w[ky, kx]
    return out.reshape(B, Ho, Wo, Cout)


def depthwise_forward(x, w, stride, pads):
    """The 3x3 depthwise conv (w [3,3,C,1])."""
    B, H, W, C = x.shape
    pt, pb, pl, pr = pads
    xp = torch.nn.functional.pad(x, (0, 0, pl, pr, pt, pb))
    Ho, Wo = (H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1
    out = torch.zeros((B, Ho, Wo, C), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] * w[ky, kx, :, 0]
    return out


def _act(z, act):
    return z.clamp(0.0, 6.0) if act == "relu6" else (z.clamp(min=0.0) if act == "relu" else z)


def softmax_forward(z, a_z, absolute=False):
    """softmax over the last axis of the logits z and, with ``absolute``, its A to first order in the logits' own A:
    p_i = e_i / S with e_j = exp(z_j - m), m = max_j z_j.  dp_i = p_i (dz_i - sum_j p_j dz_j); besides the logit's A_z the
    exponent z_j - m is evaluated with a relative error on d_j = |z_j - m| (the subtraction and the exp's argument
    reduction), and the exp, the sum and the division add a unit each of the result:
        A_p,i = p_i (A_z,i + sum_j p_j A_z,j + d_i + sum_j p_j d_j + 1)."""
    m = z.max(-1, keepdim=True).values
    e = torch.exp(z - m)
    p = e / e.sum(-1, keepdim=True)
    if not absolute:
        return p
    d = (z - m).abs()
    return p * (a_z + (p * a_z).sum(-1, keepdim=True) + d + (p * d).sum(-1, keepdim=True) + 1.0)


def layer_forward(spec, t, dtype=torch.float64, absolute=False, round_ops=None):
    """Forward of one layer from the other implementation's own tensors.  ``t``: x (input activation) and, by kind, w,
    gamma, beta, bias, res (the residual tensor); BatchNorm on batch statistics: pre / mean / var AS THE DEVICE HOLDS THEM
    (``out`` is evaluated from those, so that no error of the conv or of the statistics reaches it); a frozen BatchNorm:
    moving_mean / moving_var instead (no pre: the conv epilogue applies the folded scale / shift); head: w_label / b_label /
    w_box / b_box.  Returns {key: tensor}:
      "pre"             BatchNorm layers on batch statistics: conv(x, w);                A = conv(|x|, |w|)
      "out"             ... act(gamma (pre - mean) istd + beta) + res, istd = rsqrt(var + eps);
                                                    A = |gamma| (|pre| + |mean|) istd + |beta| + |res|
                        (covers the subtract-first form and the folded scale / shift form alike)
                        frozen: act(fscale conv + fshift) + res, fscale = gamma rsqrt(moving_var + eps),
                        fshift = beta - moving_mean fscale;  A = |fscale| conv(|x|, |w|) + |beta| + |moving_mean fscale| + |res|
                        bias layers: act(conv + bias);       A = conv(|x|, |w|) + |bias|
                        pool: the window maximum, A = 0 (bit for bit);  L2 norm: gamma x rsqrt(max(sum x^2, 1e-12)),
                        A = |gamma x| rs
      "deltas", "probs" heads: conv(x, w_box) + b_box [B,H,W,a*4]; softmax over L of conv(x, w_label) + b_label
                        [B,H,W,a*L] (A: softmax_forward)
    absolute=True returns A.  round_ops: see conv_forward (dense convs only; the depthwise conv is fp32 in both modes)."""
    ab = (lambda v: v.abs()) if absolute else (lambda v: v)
    kind = spec["kind"]
    xs = _t(t["x"], dtype)
    if kind == "pool":
        cells, _, _ = pool_windows(xs, spec)
        mx = cells.max(0).values
        return {"out": torch.zeros_like(mx) if absolute else mx}
    if kind == "l2norm":
        rs = torch.rsqrt(torch.clamp((xs * xs).sum(-1, keepdim=True), min=1e-12))
        return {"out": ab(_t(t["gamma"], dtype) * xs) * rs}
    pads = _pads(spec, xs.shape[1], xs.shape[2])
    if kind == "head":
        L = spec["labels"]
        lin = lambda x, w, b: conv_forward(x, w, 1, 1, pads, round_ops) + b
        r = {"deltas": lin(ab(xs), ab(_t(t["w_box"], dtype)), ab(_t(t["b_box"], dtype)))}
        z = lin(xs, _t(t["w_label"], dtype), _t(t["b_label"], dtype))
        a_z = lin(xs.abs(), _t(t["w_label"], dtype).abs(), _t(t["b_label"], dtype).abs()) if absolute else z
        sh = z.shape
        r["probs"] = softmax_forward(z.reshape(sh[:3] + (-1, L)), a_z.reshape(sh[:3] + (-1, L)), absolute).reshape(sh)
        return r
    x, w = ab(xs), ab(_t(t["w"], dtype))
    conv = depthwise_forward(x, w, spec["stride"], pads) if kind == "dw" else \
        conv_forward(x, w, spec["stride"], spec["dil"], pads, round_ops)
    r = {}
    if spec["bn"] and "moving_var" not in t:
        r["pre"] = conv
        gamma, beta = ab(_t(t["gamma"], dtype)), ab(_t(t["beta"], dtype))
        istd = torch.rsqrt(_t(t["var"], dtype) + BN_EPS)
        pre, mean = ab(_t(t["pre"], dtype)), ab(_t(t["mean"], dtype))
        z = gamma * ((pre + mean) if absolute else (pre - mean)) * istd + beta
    elif spec["bn"]:
        fscale = _t(t["gamma"], dtype) * torch.rsqrt(_t(t["moving_var"], dtype) + BN_EPS)
        shift_mean = _t(t["moving_mean"], dtype) * fscale
        z = fscale.abs() * conv + _t(t["beta"], dtype).abs() + shift_mean.abs() if absolute else \
            fscale * conv + (_t(t["beta"], dtype) - shift_mean)
    else:
        z = conv + ab(_t(t["bias"], dtype)) if spec["bias"] else conv
    out = z if absolute else _act(z, spec["act"])
    if spec["res"]:
        out = out + ab(_t(t["res"], dtype))
    r["out"] = out
    return r


def batch_stats(pre, dtype=torch.float64):
    """mean, biased variance over (B,H,W) and their A: the two-pass formulas mean = sum x / M, var = sum (x - mean)^2 / M
    with absolute values and the subtraction as an addition -- A_mean = sum |x| / M, A_var = sum (|x| + |mean|)^2 / M."""
    p = _t(pre, dtype)
    M = p.shape[0] * p.shape[1] * p.shape[2]
    mean = p.sum((0, 1, 2)) / M
    var = ((p - mean) ** 2).sum((0, 1, 2)) / M
    a_mean = p.abs().sum((0, 1, 2)) / M
    a_var = ((p.abs() + mean.abs()) ** 2).sum((0, 1, 2)) / M
    return mean, var, a_mean, a_var, M


def moving_update(moving_mean, moving_var, mean, var, M):
    """Keras moving averages after one training forward (the formula of tests/test_train.py: Bessel-corrected
    variance, momentum 0.999), float32 like the oracle there."""
    f = np.float32
    mu, va = np.asarray(mean, f), (np.asarray(var, np.float64) * (M / max(M - 1, 1))).astype(f)
    mm, mv = np.asarray(moving_mean, f), np.asarray(moving_var, f)
    return mm - (mm - mu) * f(1.0 - BN_MOMENTUM), mv - (mv - va) * f(1.0 - BN_MOMENTUM)


# ------------------------------------------------------------------ the metric
def e_stats(got, ref, A, exclude=None):
    """max E over the elements, its flat index, and the root mean square of E over the compared elements with A > 0
    (excluded elements left out).  NaN / A == 0 mismatches count as E = inf in the max (and, where A > 0, in the RMS)."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = ref.detach().numpy().reshape(-1) if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64).reshape(-1)
    A = A.detach().numpy().reshape(-1) if isinstance(A, torch.Tensor) else np.asarray(A, np.float64).reshape(-1)
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.where(A > 0, err / (U * A), np.where(err == 0, 0.0, np.inf))
    E[~np.isfinite(got)] = np.inf                     # NaN / inf read back: an unwritten or broken element
    keep = A > 0
    if exclude is not None:
        ex = exclude.numpy().reshape(-1) if isinstance(exclude, torch.Tensor) else np.asarray(exclude).reshape(-1)
        E = np.where(ex, 0.0, E)
        keep = keep & ~ex.astype(bool)
    if E.size == 0:
        return 0.0, -1, 0.0
    i = int(np.argmax(E))
    with np.errstate(over="ignore", invalid="ignore"):
        rms = float(np.sqrt(np.mean(E[keep] ** 2))) if keep.any() else 0.0
    return float(E[i]), i, rms


def e_metric(got, ref, A, exclude=None):
    """max E over the elements, its flat index, and the count of NaN / A == 0 mismatches (E = inf there)."""
    return e_stats(got, ref, A, exclude)[:2]


def e_rms(got, ref, A, exclude=None):
    """The RMS companion of ``e_metric``: sqrt(mean E^2) over the compared elements with A > 0."""
    return e_stats(got, ref, A, exclude)[2]


class Report(object):
    """Worst E per layer kind and where, the largest RMS of E of that kind next to it; ``fails`` lists everything above
    the bar; ``stats`` holds (max E, RMS of E) of every compared tensor under (layer, what)."""
    def __init__(self, bar=E_BAR):
        self.bar, self.worst, self.worst_rms, self.stats, self.fails, self.compared = bar, {}, {}, {}, [], 0

    def add(self, kind, layer, what, got, ref, A, exclude=None):
        E, i, rms = e_stats(got, ref, A, exclude)
        self.compared += 1
        self.stats[(layer, what)] = (E, rms)
        key = "%s: %s" % (kind, what.split(":")[0])
        if key not in self.worst or E > self.worst[key][0]:
            self.worst[key] = (E, layer, what)
        if key not in self.worst_rms or rms > self.worst_rms[key][0]:
            self.worst_rms[key] = (rms, layer, what)
        if not E <= self.bar:
            self.fails.append("%s %s: E = %.3g at flat index %d" % (layer, what, E, i))
        return E

    def lines(self):
        return ["worst E %-44s %8.3f  (%s %s)   rms %.3f (%s)" % (k, v[0], v[1], v[2], self.worst_rms[k][0], self.worst_rms[k][1])
                for k, v in sorted(self.worst.items())]


# ------------------------------------------------------------------ a whole graph, teacher forced
def bf16_rne(a):
    """fp32 value (the argument is first rounded to float32, as the checked implementation holds it) -> nearest
    bfloat16, ties to even; returned as a float64 tensor.  |x| rounds to |round(x)|: the same function serves A."""
    return _t(a, torch.float32).to(torch.bfloat16).to(torch.float64)


def cut16(a, rounded=False):
    """fp32 value -> its leading 16 significand bits, as a float32 tensor: truncated (what a three-way bf16 split that lost
    its third plane multiplies) or, ``rounded``, rounded to nearest with ties to even (the weaker cut: half the error)."""
    i = _t(a, torch.float32).contiguous().view(torch.int32)
    if rounded:
        i = i + 0x7F + ((i >> 8) & 1)            # sign-magnitude bits: the same addition serves both signs
    return (i & -256).view(torch.float32)


def rne16(a):
    """``cut16(a, rounded=True)`` as a float64 tensor: a ``round_ops`` of conv_forward.  |x| rounds to |round(x)|."""
    return cut16(a, rounded=True).to(torch.float64)


TWO_PLANE_A = 2.0 ** -33 / U


def two_plane_allowance(ref):
    """What A grows by for a tensor kept as the two-plane fp16 pair only: the pair holds x within 2^-22 |x| + 2^-33
    (csrc/ssd_bf16x3.h), i.e. within u (4 |x| + 2^-9)."""
    return 4.0 * ref.abs() + TWO_PLANE_A


def forward_yardstick(spec, t, round_ops=None, ref=None, A=None):
    """Reference-only yardsticks of one dense conv / head layer on the input of the comparison, per output key:
      "r32": (max E, RMS E) of ``layer_forward(..., dtype=torch.float32)`` -- the plain fp32 restatement (in the form
             ``round_ops`` names, so that a bf16-mode layer is measured against its own definition);
      "r16": the same for the float64 forward with both matrix operands ROUNDED to nearest to 16 significand bits
             (always on the unrounded form: under bf16 operands the cut is the identity).
    Both against the float64 forward and its A (``ref`` / ``A``: those of the form ``round_ops``, where the caller has them)."""
    assert spec["kind"] in ("conv", "head"), spec["kind"]
    if ref is None:
        ref, A = layer_forward(spec, t, round_ops=round_ops), layer_forward(spec, t, absolute=True, round_ops=round_ops)
    f32 = layer_forward(spec, t, dtype=torch.float32, round_ops=round_ops)
    if round_ops is not None:
        ref16, A16 = layer_forward(spec, t), layer_forward(spec, t, absolute=True)
    else:
        ref16, A16 = ref, A
    c16 = layer_forward(spec, t, round_ops=rne16)
    keys = [k for k in ref if k != "pre"] if "moving_var" in t or not spec.get("bn") else ["pre"]
    return {k: {"r32": e_stats(f32[k].numpy(), ref[k], A[k])[::2], "r16": e_stats(c16[k].numpy(), ref16[k], A16[k])[::2]}
            for k in keys}


def check_graph(specs, fetch, weights, grads, hyper_params, B, report, moving_after=None,
                moving_before=None, progress=None, only=None, params=True, round_dx=None):
    """Hold a training step of another implementation to the float64 layer oracle.

    specs: ``layers(backbone, hp)`` (entries may carry "l2").  fetch(name) -> NHWC float32 array of a training
    activation, "grad:<tensor>", "pre:<layer>" ([B,Ho,Wo,C]), "mean:<layer>", "var:<layer>" ([C]) or the head
    gradients "grad_logits" [B,N,L] / "grad_deltas" [B,N,4].  weights / grads: {Keras parameter name: array}.
    moving_before / moving_after: the parameters before / after the step (BatchNorm moving averages), optional.
    only: set of layer names -- run these layers only; a tensor's gradient is then compared when ALL its consumers are in
    the set.  params=False: data gradients only (no parameter gradients, no batch statistics).  round_dx: see
    conv_backward (the bf16 mode: dense-conv data gradients from once-rounded operands).  Under round_dx each dense
    conv's contribution is admitted in two forms, both operands rounded or neither (the same conv on an fp32 tile), and
    a tensor passes if ONE combination of its consumers' forms meets the bar.
    Returns {"layers": n compared, "pool_excluded": share of max-pool input cells left out as ties}."""
    consumers = {}
    for s in specs:
        consumers.setdefault(s["tin"], []).append(s["name"])
        if s.get("res"):
            consumers.setdefault(s["res"], []).append(s["name"] + " (residual)")
    contrib = {}                  # tensor -> [sum of contributions, sum of A, consumers still missing, exclude]
    fm = hyper_params["feature_map_shapes"]
    lvl_off = np.cumsum([0] + [f * f * (len(a) + 1) for f, a in zip(fm, hyper_params["aspect_ratios"])])
    n_layers, pool_cells, pool_tied = 0, 0, 0

    def put(tensor, alts, n_cons, exclude=None):
        # alts: the admissible (value, A) forms of this contribution (one; two for a dense conv under round_dx)
        c = contrib.setdefault(tensor, [[(0, 0)], n_cons, None])
        c[0], c[1] = [(v0 + v, a0 + a) for v0, a0 in c[0] for v, a in alts], c[1] - 1
        if exclude is not None:
            c[2] = exclude
        if c[1] == 0:
            got = fetch("grad:" + tensor)
            v, a = min(c[0], key=lambda va: e_metric(got, va[0], va[1], c[2])[0]) if len(c[0]) > 1 else c[0][0]
            report.add(kind, s["name"], "grad:" + tensor, got, v, a, c[2])
            del contrib[tensor]

    for s in reversed(specs):
        if only is not None and s["name"] not in only:
            continue
        kind = layer_kind(s)
        t = {"x": fetch(s["tin"])}
        if s["kind"] == "head":
            a, L, i = s["anchors"], s["labels"], s["level"]
            H, W = t["x"].shape[1], t["x"].shape[2]
            lo, hi = int(lvl_off[i]), int(lvl_off[i + 1])
            t["g_label"] = fetch("grad_logits")[:, lo:hi].reshape(B, H, W, a * L)
            t["g_box"] = fetch("grad_deltas")[:, lo:hi].reshape(B, H, W, a * 4)
            t["w_label"] = weights["%d_conv_label_output/kernel" % (i + 1)]
            t["w_box"] = weights["%d_conv_boxes_output/kernel" % (i + 1)]
        elif s["kind"] == "l2norm":
            t["dout"], t["gamma"] = fetch("grad:" + s["tout"]), weights["l2_normalization/scale"]
        elif s["kind"] == "pool":
            t["dout"] = fetch("grad:" + s["tout"])
        else:
            t["dout"] = fetch("grad:" + s["tout"])
            t["w"] = weights[s["name"] + ("/depthwise_kernel" if s["kind"] == "dw" else "/kernel")]
            if s["act"]:
                t["out"] = fetch(s["tout"])
            if s["bn"]:
                t["pre"], t["mean"], t["var"] = fetch("pre:" + s["name"]), fetch("mean:" + s["name"]), fetch("var:" + s["name"])
                t["gamma"] = weights[s["bn"] + "/gamma"]
            if s["bn"] and params:
                mean, var, a_mean, a_var, M = batch_stats(t["pre"])
                report.add(kind, s["name"], "mean", t["mean"], mean, a_mean)
                report.add(kind, s["name"], "var", t["var"], var, a_var)
                if moving_after is not None:
                    mm, mv = moving_update(moving_before[s["bn"] + "/moving_mean"], moving_before[s["bn"] + "/moving_variance"],
                                           mean.numpy(), var.numpy(), M)
                    np.testing.assert_allclose(moving_after[s["bn"] + "/moving_mean"], mm, rtol=1e-5, atol=1e-6, err_msg=s["bn"])
                    np.testing.assert_allclose(moving_after[s["bn"] + "/moving_variance"], mv, rtol=1e-5, atol=1e-6, err_msg=s["bn"])
        ref = layer_backward(s, t, round_dx=round_dx)
        A = layer_backward(s, t, absolute=True, round_dx=round_dx)
        n_layers += 1
        names = {"dw": s["name"] + ("/depthwise_kernel" if s["kind"] == "dw" else "/kernel"), "dbias": s["name"] + "/bias"}
        if s["kind"] == "l2norm":
            names["dgamma"] = "l2_normalization/scale"
        elif s["kind"] == "head":
            i = s["level"] + 1
            names = {"dw_label": "%d_conv_label_output/kernel" % i, "dbias_label": "%d_conv_label_output/bias" % i,
                     "dw_box": "%d_conv_boxes_output/kernel" % i, "dbias_box": "%d_conv_boxes_output/bias" % i}
        elif s.get("bn"):
            names["dgamma"], names["dbeta"] = s["bn"] + "/gamma", s["bn"] + "/beta"
        for key, pname in names.items():
            if key in ref and params:
                report.add(kind, s["name"], key + ":" + pname, grads[pname], ref[key], A[key])
        if s["kind"] == "pool":
            tied = ref["tied"]
            pool_cells += tied.numel()
            pool_tied += int(tied.sum())
            # mass conservation per image and channel stands in for the tied cells
            got = fetch("grad:" + s["tin"]) if len(consumers[s["tin"]]) == 1 and params else None
            if got is not None:
                gout = torch.from_numpy(t["dout"]).to(torch.float64)
                report.add(kind, s["name"], "mass:" + s["tin"], got.astype(np.float64).sum((1, 2)), gout.sum((1, 2)),
                           gout.abs().sum((1, 2)))
        if "dres" in ref:
            put(s["res"], [(ref["dres"], A["dres"])], len(consumers[s["res"]]))
        if "dx" in ref:
            alts = [(ref["dx"], A["dx"])]
            if round_dx and s["kind"] in ("conv", "head"):       # ... or the same conv on an fp32 tile: no operand rounded
                alts.append((layer_backward(s, t)["dx"], layer_backward(s, t, absolute=True)["dx"]))
            put(s["tin"], alts, len(consumers[s["tin"]]), ref.get("tied"))
        if progress:
            progress(s["name"])
    assert only is not None or not contrib, "tensors with consumers that never ran: %s" % sorted(contrib)
    return {"layers": n_layers, "pool_excluded": pool_tied / pool_cells if pool_cells else 0.0}


def check_forward_graph(specs, fetch, weights, hyper_params, B, report, only=None, frozen=(), round_ops=None,
                        yardstick=None, planes=None):
    """Hold the training FORWARD of another implementation to the float64 layer oracle: every layer's outputs
    (layer_forward) recomputed from the implementation's own input tensor ``fetch(s["tin"])`` and compared through
    ``report.add``.  ``fetch`` as in check_graph, plus "probs" [B,N,L] and "deltas" [B,N,4] (a head's slices are taken at
    the level's anchor offset, as check_graph slices the head gradients).  frozen: names of the layers whose BatchNorm is
    frozen -- folded on the moving statistics of ``weights``; their "pre:" / "mean:" / "var:" are NOT fetched (a frozen
    layer never writes them).  round_ops: the bf16 mode -- a dense conv's outputs are admitted in two forms, both operands
    rounded once or neither (the same conv on an fp32 tile); one launch writes all outputs of a layer, so ONE form must
    meet the bar for all of them (the form with the smaller worst E is the one reported).
    yardstick: a dict that receives, per dense conv / head layer, ``forward_yardstick`` of the reported form on the same
    input, {layer: {key: {"r32": (max, rms), "r16": (max, rms)}}}.  planes: {tensor name: number of planes} of the output
    tensors the implementation keeps as planes ONLY -- 3 (the exact split) needs nothing; 2 (the fp16 pair): the tensor's A
    grows by ``two_plane_allowance`` of the reference.
    Returns {"layers": n, "clamps": {ReLU6 layer: (share of sixes, share of zeros) of the ORACLE's out}}."""
    fm = hyper_params["feature_map_shapes"]
    lvl_off = np.cumsum([0] + [f * f * (len(a) + 1) for f, a in zip(fm, hyper_params["aspect_ratios"])])
    n_layers, clamps = 0, {}
    for s in specs:
        if only is not None and s["name"] not in only:
            continue
        kind = layer_kind(s)
        t = {"x": fetch(s["tin"])}
        got = {}
        if s["kind"] == "head":
            i, L = s["level"], s["labels"]
            H, W = t["x"].shape[1], t["x"].shape[2]
            lo, hi = int(lvl_off[i]), int(lvl_off[i + 1])
            got["probs"] = fetch("probs")[:, lo:hi].reshape(B, H, W, s["anchors"] * L)
            got["deltas"] = fetch("deltas")[:, lo:hi].reshape(B, H, W, s["anchors"] * 4)
            for part, key in (("label", "label"), ("boxes", "box")):
                t["w_" + key] = weights["%d_conv_%s_output/kernel" % (i + 1, part)]
                t["b_" + key] = weights["%d_conv_%s_output/bias" % (i + 1, part)]
        elif s["kind"] == "l2norm":
            t["gamma"] = weights["l2_normalization/scale"]
            got["out"] = fetch(s["tout"])
        elif s["kind"] == "pool":
            got["out"] = fetch(s["tout"])
        else:
            t["w"] = weights[s["name"] + ("/depthwise_kernel" if s["kind"] == "dw" else "/kernel")]
            got["out"] = fetch(s["tout"])
            if s["res"]:
                t["res"] = fetch(s["res"])
            if s["bias"]:
                t["bias"] = weights[s["name"] + "/bias"]
            if s["bn"]:
                t["gamma"], t["beta"] = weights[s["bn"] + "/gamma"], weights[s["bn"] + "/beta"]
                if s["name"] in frozen:
                    t["moving_mean"], t["moving_var"] = weights[s["bn"] + "/moving_mean"], weights[s["bn"] + "/moving_variance"]
                else:
                    for k in ("pre", "mean", "var"):
                        t[k] = fetch(k + ":" + s["name"])
                    got["pre"] = t["pre"]
        forms = [(layer_forward(s, t, round_ops=round_ops), layer_forward(s, t, absolute=True, round_ops=round_ops))]
        form_ops = round_ops if s["kind"] in ("conv", "head") else None
        if round_ops and s["kind"] in ("conv", "head"):
            forms.append((layer_forward(s, t), layer_forward(s, t, absolute=True)))
            worst = [max(e_metric(got[k], ref[k], A[k])[0] for k in got) for ref, A in forms]
            if int(np.argmin(worst)) == 1:
                forms, form_ops = forms[1:], None
        ref, A = forms[0]
        assert set(ref) == set(got), (s["name"], sorted(ref), sorted(got))
        if yardstick is not None and s["kind"] in ("conv", "head"):
            yardstick[s["name"]] = forward_yardstick(s, t, round_ops=form_ops, ref=ref, A=A)
        if planes and s["tout"] and planes.get(s["tout"]) == 2:
            A = dict(A, out=A["out"] + two_plane_allowance(ref["out"]))
        for k in sorted(got):
            report.add(kind, s["name"], k + ":" + (s["tout"] or s["name"]), got[k], ref[k], A[k])
        if s.get("act") == "relu6":
            o = ref["out"]
            clamps[s["name"]] = (float((o == 6).double().mean()), float((o == 0).double().mean()))
        n_layers += 1
    return {"layers": n_layers, "clamps": clamps}
