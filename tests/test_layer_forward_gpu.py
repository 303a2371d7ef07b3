"""The FORWARD of the training step (csrc/ssd_train.hip: train_forward_layer) against the float64 LAYER oracle
(oracle/layer_grad_oracle.py: layer_forward / check_forward_graph).

One device training step, then every layer's forward is recomputed in float64 from the device's own input tensor of that
layer and compared element by element in E = |got - ref64| / (2^-24 A), A the absolute-value sum of the element's terms;
bar E <= 16 (the formulas, their A and the CPU proof that this bar separates a right forward from a subtly wrong one:
tests/test_layer_forward_cpu.py).  Compared per layer: ``pre`` (the conv in front of a BatchNorm), ``out`` (BatchNorm on
the device's own pre / mean / var + activation + residual; conv + bias + ReLU; the folded form of a frozen BatchNorm;
the L2 norm), max-pools bit for bit, and per head the level's slices of ``deltas`` and ``probs``.  The batch statistics
themselves stay with tests/test_layer_grad_gpu.py.

Which dense-conv tile wrote a layer is decided by timing on the device (launch_conv): the bar has to hold for whichever
ran.  ``helpers.clamp_weights`` makes both clamps of every ReLU6 fire under batch statistics (asserted on the ORACLE's
maps: >= 1 % sixes and >= 10 % zeros in each), so that act_fwd's upper clamp and the ``z < 6`` side of the backward's
pass-mask are really exercised; the first test therefore passes its step through check_graph (the backward) as well.

Worst E measured on an MI355X (bar 16), MobileNetV2 B = 2 / VGG16 B = 1, with the layer it occurred at and the tile the
step's log (SSD_HIP_TRAIN_AUTOTUNE=2) names for it:
  pre (conv in front of BatchNorm)  1x1 5.8 (block_13_expand, K = 96, mfma_1x1_4x1_k32), + residual 4.3 (block_7_project),
                                    project without residual 5.7 (block_10_project); stem 3x3 s2 3.8 (Conv1, direct);
                                    depthwise s1 4.0 (expanded_conv_depthwise), s2 3.7 (block_3_depthwise)
  out, BatchNorm apply              + ReLU6 3.0, + residual 3.9 (block_2_project), plain 3.8; behind the depthwise 2.9 / 2.8
  out, bias + ReLU                  1x1 3.9 (extra1_1, mfma_1x1_4x1_k64) / 4.7 (conv7, mfma_1x2_2x2_k64); 3x3 s1 7.6 (conv2_2,
                                    K = 1152, split-bf16 mfma3_2x4_4x2); dilation 6 5.7 (conv6, mfma_1x1_4x1_k64);
                                    3x3 s2 3.6 (extra1_2) / 4.1 (conv8_2, mfma_1x1_4x1_k64)
  heads                             deltas 3.7 (level 3, K = 4608, mfma_1x1_4x1_k64) / 3.7 (VGG16 level 2, K = 9216);
                                    probs 2.2 (level 2, K = 11520) / 2.2 (VGG16 level 1)
  pools                             0 (bit for bit);  L2 norm 3.7
  bf16 mode                         pre 5.5 (block_11_expand), bias + ReLU 3.7, heads deltas 1.8 / probs 0.9 (the timing put all six heads,
                                    the extras and about half of the 1x1 convs on bf16_* tiles -- held in the rounded form --
                                    and the rest on mfma_* tiles)
  frozen backbone                   folded conv epilogue 4.4 (expanded_conv_project), + ReLU6 2.5, + residual 3.8;
                                    folded depthwise 3.1 / 2.3; stem 3.0
  the backward of the clamp_weights step (check_graph)   10.3 (grad of block_13_expand_relu), batch variance 12.5 (Conv_1)
Every VALU kernel (depthwise, bn_apply_kernel, pools, L2 norm, softmax) sits at the CPU restatement's floor of <= 4; the
matrix-core convs reach 5.8 on fp32 MFMA tiles and 7.6 on the split-bf16 tile, as in the backward.  No tensor needed a bar
of its own.  ReLU6 maps of the oracle: fewest sixes 6.4 % (expanded_conv_depthwise), fewest zeros 30.8 % (block_8_expand);
frozen: 4.5 % (Conv1) / 33.7 % (block_8_depthwise)."""
import numpy as np
import pytest
import torch

import helpers
from oracle import layer_grad_oracle as lg
from test_layer_grad_gpu import _targets

pytestmark = pytest.mark.gpu

MIN_SIXES, MIN_ZEROS = 0.01, 0.10          # the block oracle's numbers (tests/test_block_oracle_gpu.py)


def _step(backbone, B, x, w, precision="fp32", freeze=False):
    """One device training step; returns what the two graph checks need."""
    from models._net import SSDModel
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = helpers.hyper_params(backbone)
    w = {k: v.copy() for k, v in w.items()}
    yd, yl = _targets(hp, B)
    m = SSDModel(backbone, hp, precision=precision)
    m.set_weights(w)
    frozen_keras = set(m.freeze_backbone()) if freeze else set()
    m.compile()
    _, _, g = m.forward_backward(x, yd, yl)
    g = g.cpu().numpy().copy()
    assert np.isfinite(g).all()
    specs = lg.layers(backbone, hp)
    shapes = lg.tensor_shapes(specs, w)
    N, L = yl.shape[1], hp["total_labels"]
    flat = {"grad_logits": L, "grad_deltas": 4, "probs": L, "deltas": 4}
    cache = {}

    def fetch(name):
        if name not in cache:
            if name == "input":
                cache[name] = x
            elif name in flat:
                cache[name] = m.train_fetch(name, B).reshape(B, N, flat[name])
            elif name.startswith(("mean:", "var:")):
                cache[name] = m.train_fetch(name, B)
            else:
                key = name[5:] if name.startswith("grad:") else name
                cache[name] = m.train_fetch(name, B).reshape((B,) + shapes[key])
        return cache[name]
    grads = {name: g[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in m.trainable_offsets().items()}
    frozen = {s["name"] for s in specs if s.get("bn") and s["bn"] in frozen_keras}
    return dict(m=m, hp=hp, w=w, specs=specs, fetch=fetch, grads=grads, after=m.get_weights(), frozen=frozen, B=B)


def _check_forward(st, **kw):
    report = lg.Report()
    info = lg.check_forward_graph(st["specs"], st["fetch"], st["w"], st["hp"], st["B"], report, frozen=st["frozen"], **kw)
    for line in report.lines():
        print(line)
    print("forward: %d layers, %d tensors compared" % (info["layers"], report.compared))
    return report, info


def _assert_clamps(info, n=35):
    """Both clamps of every ReLU6 map fire -- on the float64 oracle's maps, not the device's."""
    c = info["clamps"]
    assert len(c) == n
    lo6, lo0 = min(c, key=lambda k: c[k][0]), min(c, key=lambda k: c[k][1])
    print("ReLU6 maps: fewest sixes %.2f %% (%s), fewest zeros %.2f %% (%s)" % (100 * c[lo6][0], lo6, 100 * c[lo0][1], lo0))
    assert c[lo6][0] >= MIN_SIXES and c[lo0][1] >= MIN_ZEROS, (lo6, c[lo6], lo0, c[lo0])


def _counts(specs):
    bn = sum(1 for s in specs if s.get("bn"))
    bias = sum(1 for s in specs if s.get("bias"))
    heads = sum(1 for s in specs if s["kind"] == "head")
    return bn, bias, heads


def test_mobilenet_v2_every_layer_forward_fp32():
    """MobileNetV2-SSD300, B = 2 (the smallest batch with non-degenerate batch statistics), clamp_weights: every output
    of all 66 layers -- the Cin = 3 stem, depthwise s1 and correct_pad s2, 1x1 expands / projects with and without the
    residual, the bias + ReLU extras (1x1 VALID, 3x3 s2 SAME), the six fused head convs with their softmax.  The same step
    then goes through check_graph: the backward at the same bar on tensors where the ``z < 6`` mask really cuts."""
    st = _step("mobilenet_v2", 2, helpers.images(2, 300, seed=41), helpers.clamp_weights("mobilenet_v2"))
    report, info = _check_forward(st)
    bn, bias, heads = _counts(st["specs"])
    assert (bn, bias, heads) == (52, 8, 6)
    assert info["layers"] == 66 and report.compared == bn * 2 + bias + heads * 2 == 124
    _assert_clamps(info)
    assert not report.fails, "\n".join(report.fails[:20])
    back = lg.Report()
    binfo = lg.check_graph(st["specs"], st["fetch"], st["w"], st["grads"], st["hp"], 2, back, moving_after=st["after"],
                           moving_before=st["w"])
    for line in back.lines():
        print(line)
    assert binfo["layers"] == 66 and back.compared == 52 * 5 + 8 * 2 + 6 * 4 + 60
    assert not back.fails, "\n".join(back.fails[:20])


def test_vgg16_every_layer_forward_fp32():
    """VGG16-SSD300, B = 1 (no BatchNorm), synthetic_weights: 23 conv outputs (dilation 6, VALID and stride-2 SAME convs,
    K up to 4608), the 5 pools bit for bit (2/2 on odd maps, the overlapping 3/1), the L2 norm at scale 20, 12 head
    tensors."""
    st = _step("vgg16", 1, helpers.images(1, 300, seed=43), helpers.synthetic_weights("vgg16"))
    report, info = _check_forward(st)
    assert info["layers"] == 35 and report.compared == 23 + 5 + 1 + 12 == 41
    assert not info["clamps"]
    assert not report.fails, "\n".join(report.fails[:20])


def test_mobilenet_v2_forward_bf16():
    """precision="bf16", B = 2, clamp_weights.  The rule, from the code: launch_conv (csrc/ssd_train.hip) lets a bf16 net
    choose among the "bf16_*" tiles (csrc/ssd_conv3.hip), the fp32-MFMA "mfma_*" tiles and, for the Cin = 3 stem, the
    fp32 direct kernel (conv_config_allowed: CONV_NET_BF16), by timing.  A "bf16_*" tile multiplies both operands rounded
    ONCE to bf16, nearest with ties to even -- the weights when pack_split_kernel writes their fourth plane (rne1), the
    activations when the tile stages them (csrc/ssd_bf16x3.h: bf16_mode, rne1 / rne2) -- products and sums in fp32; every
    other admitted kernel rounds NO operand.  Which ran is not observable, so the oracle computes both forms in float64 and
    one of them must meet E <= 16 on ALL outputs of the layer (one launch writes them).  Unlike the backward (where a
    BatchNorm layer's dY is not observable: 10 tensors), every dense conv's input is a fetched tensor: all 35 dense convs and
    6 head pairs are held.  The depthwise conv (launch_dwconv3x3: fp32 FMAs, no precision argument) and bn_apply_kernel
    are fp32 in both modes and are held as in the fp32 test."""
    st = _step("mobilenet_v2", 2, helpers.images(2, 300, seed=41), helpers.clamp_weights("mobilenet_v2"), precision="bf16")
    report, info = _check_forward(st, round_ops=lg.bf16_rne)
    assert info["layers"] == 66 and report.compared == 124
    _assert_clamps(info)
    assert not report.fails, "\n".join(report.fails[:20])


def test_mobilenet_v2_forward_frozen_backbone():
    """freeze_backbone(), B = 2, clamp_weights: the 52 backbone layers run folded on the moving statistics --
    bn_fold_jobs_kernel, the dense conv's epilogue with scale / shift / activation / residual, the depthwise kernel with
    fscale -- and are held to act(fscale conv + fshift) + res; their ``pre`` / ``mean`` / ``var`` are not written and not
    fetched, and their moving averages must stay bit for bit.  Extras and heads as in the fp32 test.  The images carry a
    gain of 1.5: a frozen BatchNorm does not normalise it away, and without it the stem's map (images in [0, 1) against
    moving statistics that are not its own) holds 0.8 % sixes, below the clamp condition; with it 4.5 %."""
    x = helpers.images(2, 300, seed=41) * np.float32(1.5)
    st = _step("mobilenet_v2", 2, x, helpers.clamp_weights("mobilenet_v2"), freeze=True)
    assert len(st["frozen"]) == 52
    report, info = _check_forward(st)
    assert info["layers"] == 66 and report.compared == 52 + 8 + 6 * 2
    _assert_clamps(info)
    for s in st["specs"]:
        if s["name"] in st["frozen"]:
            for v in ("/moving_mean", "/moving_variance"):
                assert np.array_equal(st["after"][s["bn"] + v], st["w"][s["bn"] + v]), s["bn"] + v
    assert not report.fails, "\n".join(report.fails[:20])
