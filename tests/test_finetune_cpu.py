"""Fine-tuning with frozen layers (Keras ``layer.trainable = False``), the part that needs no device: the trainable flags
through the library (ssd_net_set_trainable / ssd_net_get_trainable) and through the Python proxies and patterns, the name
sets of ``freeze_backbone``, and the backward PLAN (ssd_net_train_plan) -- a pure function of the graph and the flags --
which is what makes the pruning of the backward checkable without a GPU.  The expected plan is derived here from the
oracle's own graph description (oracle/layer_grad_oracle.py: which layer has a BatchNorm, a residual input, which
tensor it reads), not from the library."""
import ctypes

import pytest

import helpers
from oracle import layer_grad_oracle as lg


def _model(backbone):
    from models._net import SSDModel
    return SSDModel(backbone, helpers.hyper_params(backbone))


@pytest.fixture(scope="module")
def mbv2():
    return _model("mobilenet_v2")


@pytest.fixture(scope="module")
def vgg():
    return _model("vgg16")


@pytest.fixture(autouse=True)
def _all_trainable(mbv2, vgg):
    """Every test starts from (and leaves) the default: everything trainable."""
    for m in (mbv2, vgg):
        m.set_trainable("*", True)
    yield
    for m in (mbv2, vgg):
        m.set_trainable("*", True)


def _applicable(spec):
    """Every bit of an all-trainable step that applies to a layer of the oracle's graph description."""
    import ssd_hip as h
    if spec["kind"] == "pool":
        return h.PLAN_DGRAD
    f = h.PLAN_WGRAD | (0 if spec["tin"] == "input" else h.PLAN_DGRAD)
    if spec["kind"] == "head":
        return f | h.PLAN_WGRAD2
    if spec["kind"] == "l2norm":
        return f
    if spec["bn"]:
        f |= h.PLAN_BN_BATCH | h.PLAN_BN_PARAMS
    if spec["res"]:
        f |= h.PLAN_RESGRAD
    return f


def _specs(backbone):
    return lg.layers(backbone, helpers.hyper_params(backbone))


def test_names_are_validated_and_round_trip_through_the_library(mbv2):
    import ssd_hip as h
    lib = h.lib()
    net = mbv2._net
    for name in ("Conv1", "bn_Conv1", "block_3_depthwise_BN", "extra2_1", "4_conv_boxes_output", "4_conv_label_output"):
        assert lib.ssd_net_get_trainable(net, name.encode()) == 1
        assert lib.ssd_net_set_trainable(net, name.encode(), 0) == 0
        assert lib.ssd_net_get_trainable(net, name.encode()) == 0
        assert lib.ssd_net_set_trainable(net, name.encode(), 1) == 0
        assert lib.ssd_net_get_trainable(net, name.encode()) == 1
    # a parameter name, a tensor name, a native (fused head) layer name and a layer of the other backbone are no Keras layers
    for bad in ("Conv1/kernel", "Conv1_relu", "4_conv_heads", "conv1_1", "l2_normalization", "", "bn_Conv1/moving_mean"):
        assert lib.ssd_net_set_trainable(net, bad.encode(), 0) == -1, bad
        assert bad in lib.ssd_last_error().decode() or not bad
        assert lib.ssd_net_get_trainable(net, bad.encode()) == -1, bad
    assert mbv2.non_trainable_layer_names() == []
    f = ctypes.c_int(0)
    assert lib.ssd_net_train_plan(net, -1, ctypes.byref(f)) == -1
    assert lib.ssd_net_train_plan(net, lib.ssd_net_num_layers(net), ctypes.byref(f)) == -1


def test_python_proxies_and_patterns(mbv2, vgg):
    layer = mbv2.get_layer("block_5_project_BN")
    assert layer.name == "block_5_project_BN" and layer.trainable is True
    layer.trainable = False
    assert layer.trainable is False and mbv2.non_trainable_layer_names() == ["block_5_project_BN"]
    assert "block_5_project_BN" not in mbv2.trainable_layer_names()
    assert len(mbv2.trainable_layer_names()) == len(mbv2.layer_names()) - 1
    layer.trainable = True
    with pytest.raises(ValueError):
        mbv2.get_layer("no_such_layer")
    with pytest.raises(ValueError):
        mbv2.set_trainable(["no_such_*"], False)
    got = mbv2.set_trainable(["block_1_*", "*_conv_boxes_output"], False)
    assert got == ["block_1_expand", "block_1_expand_BN", "block_1_depthwise", "block_1_depthwise_BN", "block_1_project",
                   "block_1_project_BN"] + ["%d_conv_boxes_output" % i for i in range(1, 7)]
    assert mbv2.non_trainable_layer_names() == got
    # patterns are case-sensitive: Conv1 (the stem) is not conv1
    with pytest.raises(ValueError):
        mbv2.set_trainable("conv1", False)
    assert vgg.set_trainable("l2_*", False) == ["l2_normalization"]
    assert vgg.get_layer("l2_normalization").trainable is False


def test_freeze_backbone_name_sets(mbv2, vgg):
    names = mbv2.layer_names()
    assert len(names) == 52 * 2 + 8 + 12            # 52 conv + BatchNorm pairs, 8 extras, 6 label and 6 box convs
    frozen = mbv2.freeze_backbone()
    assert frozen == [n for n in names if not n.startswith("extra") and not n[0].isdigit()] and len(frozen) == 104
    assert mbv2.non_trainable_layer_names() == frozen
    assert mbv2.trainable_layer_names() == [n for n in names if n.startswith("extra") or n[0].isdigit()]
    mbv2.set_trainable("*", True)
    no_bn = mbv2.freeze_backbone(batch_norm=False)
    assert len(no_bn) == 52 and not [n for n in no_bn if n.endswith(("_BN", "_bn")) or n == "bn_Conv1"]
    assert set(frozen) - set(no_bn) == set(mbv2.batch_norm_layer_names())
    want = ["conv%d_%d" % (b, i) for b, n in ((1, 2), (2, 2), (3, 3), (4, 3), (5, 3)) for i in range(1, n + 1)]
    assert vgg.freeze_backbone() == want and vgg.freeze_backbone(batch_norm=False) == want
    assert vgg.non_trainable_layer_names() == want
    assert "conv6" in vgg.trainable_layer_names() and "l2_normalization" in vgg.trainable_layer_names()


@pytest.mark.parametrize("backbone", ["mobilenet_v2", "vgg16"])
def test_plan_all_trainable_has_every_applicable_bit(backbone, mbv2, vgg):
    m = mbv2 if backbone == "mobilenet_v2" else vgg
    plan = m.train_plan()
    specs = _specs(backbone)
    assert sorted(plan) == sorted(s["name"] for s in specs)
    for s in specs:
        assert plan[s["name"]] == _applicable(s), s["name"]


def test_plan_mobilenet_backbone_frozen(mbv2):
    import ssd_hip as h
    mbv2.freeze_backbone()
    plan = mbv2.train_plan()
    for s in _specs("mobilenet_v2"):
        name = s["name"]
        if s["kind"] == "head":
            # levels 1 and 2 read backbone tensors (block_13_expand_relu, out_relu): no data gradient; 3-6 read the extras
            want = h.PLAN_WGRAD | h.PLAN_WGRAD2 | (h.PLAN_DGRAD if s["level"] >= 2 else 0)
        elif name.startswith("extra"):
            want = h.PLAN_WGRAD | (0 if name == "extra1_1" else h.PLAN_DGRAD)        # extra1_1's input is out_relu
        else:
            want = h.PLAN_SKIP                                                      # no backbone layer is in the backward
        assert plan[name] == want, name


def test_plan_one_batchnorm_frozen(mbv2):
    import ssd_hip as h
    mbv2.get_layer("block_5_project_BN").trainable = False
    plan = mbv2.train_plan()
    for s in _specs("mobilenet_v2"):
        want = _applicable(s)
        if s["name"] == "block_5_project":
            want &= ~(h.PLAN_BN_BATCH | h.PLAN_BN_PARAMS)
            assert want & h.PLAN_WGRAD and want & h.PLAN_DGRAD and want & h.PLAN_RESGRAD      # block 5 has a residual input
        assert plan[s["name"]] == want, s["name"]


def test_plan_only_the_stem_conv_trainable(mbv2):
    import ssd_hip as h
    mbv2.set_trainable("*", False)
    mbv2.get_layer("Conv1").trainable = True
    plan = mbv2.train_plan()
    for s in _specs("mobilenet_v2"):
        keep = h.PLAN_DGRAD | h.PLAN_RESGRAD | (h.PLAN_WGRAD if s["name"] == "Conv1" else 0)
        assert plan[s["name"]] == _applicable(s) & keep, s["name"]
        assert s["name"] == "Conv1" or plan[s["name"]] & h.PLAN_DGRAD


def test_plan_everything_frozen_skips_everything(vgg):
    import ssd_hip as h
    vgg.set_trainable("*", False)
    assert set(vgg.train_plan().values()) == {h.PLAN_SKIP}
    # the label and the box conv of a head level freeze independently; pools below the first trainable layer stay out
    vgg.get_layer("1_conv_boxes_output").trainable = True
    plan = vgg.train_plan()
    assert plan["1_conv_heads"] == h.PLAN_WGRAD2
    assert [n for n, f in plan.items() if f != h.PLAN_SKIP] == ["1_conv_heads"]
    vgg.get_layer("l2_normalization").trainable = True
    plan = vgg.train_plan()
    assert plan["l2_normalization"] == h.PLAN_WGRAD and plan["1_conv_heads"] == h.PLAN_WGRAD2 | h.PLAN_DGRAD
    assert plan["conv4_3"] == h.PLAN_SKIP and plan["pool4"] == h.PLAN_SKIP


def test_clone_carries_the_flags(mbv2):
    # (clone() copies the weights: host-side construction only works up to there without a device, so the flags are
    # checked on the pieces clone() uses)
    frozen = mbv2.freeze_backbone()
    from models._net import SSDModel
    m = SSDModel("mobilenet_v2", helpers.hyper_params("mobilenet_v2"))
    m.set_trainable(mbv2.non_trainable_layer_names(), False)
    assert m.non_trainable_layer_names() == frozen and m.train_plan() == mbv2.train_plan()
