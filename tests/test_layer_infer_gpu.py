"""The INFERENCE graphs (csrc/ssd_net.hip: the layer launcher plus whatever the shipped table of the batch size names)
against the float64 LAYER oracle (oracle/layer_grad_oracle.py: layer_forward / check_forward_graph), layer by layer.

One device forward ``m(x)`` at the shipped table of its key (asserted: source "shipped", nothing timed), then every layer
that ran is recomputed in float64 from the device's OWN input tensor of that layer -- ``fetch_activation`` sliced to at most
two images, the first and the last of the batch -- and compared element by element in E = |got - ref64| / (2^-24 A).  Every
BatchNorm is the folded inference form (``frozen=`` all of them).  The training forward (tests/test_layer_forward_gpu.py) does
not stand in for this path: it picks tiles by timing, never reads a table and has none of the plane machinery (three-way bf16
planes, the two-plane fp16 pair, plane-only tensors, the plane-writing epilogues, the dmah -> dma3 fallback).

The bars (their proof from reference formulas alone: tests/test_layer_infer_cpu.py):
  max   E <= 16 (lg.E_BAR) on every compared tensor; pools bit for bit;
  RMS   dense convs and heads: rms E <= RMS_BARS[family] x rms(r32), r32 the fp32 restatement of the same layer on the same
        input, with RMS_BARS[family] x rms(r32) <= rms(r16) / 4 asserted on every layer's reference (r16: both operands
        rounded to 16 significand bits), so that a split that lost a plane can never pass;
  VALU  layers (depthwise, L2 norm) and pools: max E only.
A tensor the net keeps as the two-plane fp16 pair ONLY (``fetch_planes`` reports 2 and the fetched activation is the joined
pair) has A + 4 |ref| + 2^-9: the representation bound 2^-22 |x| + 2^-33 of csrc/ssd_bf16x3.h.
bf16 mode: ``round_ops=lg.bf16_rne`` with the two admitted forms of check_forward_graph, run under option ``plane_only`` 0 so
that a producer's fp32 output is what is fetched and not its bf16 storage; on the smallest bf16 case of each net
``plane_only`` 1 must give bitwise the same deltas and probabilities.

Which batch sizes: every shipped table of the net / size / precision is parsed, the (layer, family) pairs it will run are formed
(family as in conv_geometry_cases.PREFIX; ``_ks2`` and split-K > 1 count as distinct; a ``dmah_*`` line whose tensor may not
take the fp16 pair counts as its ``dma3_*`` twin, the rule of finalize_resolve_f16x2) and the smallest batch sizes that cover
the set are taken in ascending order; a later case compares only the layers whose pair no smaller case reached.  The last
test asserts the coverage from the config strings of ``m.layers(B)``.

Measured on an MI355X at the shipped tables (27 cases, 389 compared tensors; the kernels are bitwise repeatable, r32 / r16 are
torch-CPU figures and move by a few percent with the host's BLAS).  Per family: compared tensors, largest max E with its
layer and K, largest rms E / rms(r32) with its layer, the smallest cap rms(r16) / (4 rms(r32)) over the family's layers, and
the family's RMS bar (>= 1.5 x the largest ratio, and <= the cap of EVERY layer that ran the family: asserted per layer).

    family          tensors  max E  (layer, K)                              rms ratio (layer)                          cap    bar
    direct              2     4.48  vgg16 conv1_1, 27                       1.25  vgg16 conv1_1                        32.9   2.0
    mfma               25     5.80  mbv2 block_1_project, 96                1.11  mbv2 expanded_conv_project            9.6   2.0
    mfma/split         36     1.07  vgg16 conv8_2, 2304                     1.62  mbv2 B=1 6_conv_heads probs           4.4   2.5
    skinny             42     1.77  mbv2 block_12_project, 576              1.13  mbv2 B=64 4_conv_heads probs          8.3   2.0
    mfma3               2     6.39  vgg16 conv1_2, 576                      2.90  vgg16 conv1_2                        22.2   4.5
    mfma3/split        11     1.31  mbv2 B=128 extra1_2, 2304               1.84  mbv2 B=128 extra1_2                   7.7   3.0
    dma3               21     7.14  vgg16 B=3 conv3_2, 2304                 5.85  vgg16 B=32 conv5_3 (K = 4608)        10.6   9.0
    dma3/split         28     3.22  vgg16 B=1 conv3_1, 1152                 2.42  vgg16 B=1 conv3_2                     7.9   4.0
    dmah                3     3.21  mbv2 B=232 extra1_1, 1280               4.45  mbv2 B=128 1_conv_heads deltas (5184) 8.2   7.0
    dmah/split         13     1.10  mbv2-512 B=16 1_conv_heads, 5184        2.06  mbv2-512 B=16 1_conv_heads deltas     6.5   3.5
    dmah_ks2            1     3.39  mbv2 B=128 extra1_1, 1280               2.20  mbv2 B=128 extra1_1                  10.1   3.5
    dmah_ks2/split     12     1.32  mbv2-512 B=16 extra1_1, 1280            1.50  mbv2-512 B=1 1_conv_heads deltas      6.6   2.5
    bf16 mode: bf16    10     3.12  mbv2 expanded_conv_project, 32          0.98  mbv2 expanded_conv_project           18.1   2.0
               bf16/split 20  0.47  mbv2 B=4 5_conv_heads probs, 2304       1.21  mbv2 5_conv_heads probs              11.0   2.0
               dmab    25     2.53  vgg16 B=32 conv5_3, 4608                3.90  vgg16 B=32 conv5_3                   17.0   6.0
               dmab/split 45  1.02  mbv2-512 B=16 extra1_1, 1280            2.00  vgg16 B=8 conv6                       4.4   3.2
               mfma 13 / skinny 32 / direct 2:  max E 5.07 / 2.01 / 4.42,   ratio 1.00 / 1.15 / 1.25 (the fp32 families' bars)
    VALU and pools: depthwise 34 tensors, max E 4.26 fp32 / 4.44 bf16 net (expanded_conv_depthwise / block_2_depthwise);
    L2 norm 3.63 / 3.94; 10 pools 0 (bit for bit).

No tensor exceeds max E = 7.2, so no family needs a max bar of its own.  What the RMS statistic shows and the max does not:
with split-K 1 the LDS-DMA tiles accumulate all of K in one fp32 chain per accumulator, and their rms ratio grows with the
square root of the chain -- conv4_3 on the SAME tile dma3_2x4_6x2: split-K 8 (B = 1) 1.90, split-K 1 (B = 8) 5.65; head 1 of
MobileNetV2 on dmah: split-K 12 1.22, split-K 1 (B = 128) 4.45; dmab likewise 3.90 at K = 4608.  That is the random walk of a
correct fp32 sum (torch's blocked CPU sum, the yardstick r32, is short-chained at every K), not a lost plane: a lost plane
sits at >= 37 x rms(r32) whatever the split (tests/test_layer_infer_cpu.py).  These three families therefore carry the
largest bars, 9 / 7 / 6, each still under the cap of every one of their layers (10.6 / 8.2 / 17.0); a single bar for all
families would have to be 9 and would not fit under the smallest cap of the file, 4.4 (the 84 probabilities of head 6 on its
1 x 1 map), so the bar is per family.  Found and left: nothing else; no layer failed, no kernel was changed.
ReLU6 maps of the oracle (gain-8 images): fewest sixes 1.87 %, fewest zeros 42.9 % over the 35 maps of the layer-by-layer
graph; Conv_1 at the shipped tables 10.6 % / 50.1 %.  ``plane_only`` 1 reproduces ``plane_only`` 0 bit for bit on both bf16
nets (MobileNetV2 B = 4, VGG16 B = 8).  Conv_1's output is a plane-only two-plane fp16 tensor at the shipped tables of
B = 2 and 5 and of the 512 x 512 graph (its readers extra1_1 and head 2 run dmah tiles; at B = 1 Conv_1 runs a skinny tile, which
writes no planes): it is held with the allowance above and sits at max E 2.7, rms ratio 1.00.
Sensitivity on the device: the table reader does not admit a ``bf16_*`` / ``dmab_*`` line in an fp32 net (the layer is timed
instead: test_an_fp32_net_refuses_a_bf16_tile), so the proof that the bars refuse a subtly wrong layer is the CPU file's.
"""
import os
import re

import numpy as np
import pytest
import torch

import helpers
from conv_geometry_cases import PREFIX
from oracle import layer_grad_oracle as lg
from test_layer_forward_gpu import MIN_SIXES, MIN_ZEROS
from test_layer_infer_cpu import RMS_BAR_MAX, RMS_KEYS

pytestmark = pytest.mark.gpu

MBV2_TAIL = ["Conv_1"] + ["extra%d_%d" % (i, j) for i in range(1, 5) for j in (1, 2)] + ["%d_conv_heads" % i for i in range(1, 7)]
FMAPS_512 = [32, 16, 8, 4, 2, 1]
# family -> RMS bar: at least 1.5 x the largest measured rms E / rms(r32) of the family (the docstring's table)
RMS_BARS = {"direct": 2.0, "mfma": 2.0, "mfma/split": 2.5, "skinny": 2.0, "mfma3": 4.5, "mfma3/split": 3.0, "dma3": 9.0,
            "dma3/split": 4.0, "dmah": 7.0, "dmah/split": 3.5, "dmah_ks2": 3.5, "dmah_ks2/split": 2.5,
            "bf16": 2.0, "bf16/split": 2.0, "dmab": 6.0, "dmab/split": 3.2}
assert max(RMS_BARS.values()) <= RMS_BAR_MAX        # the bar every mutant of the CPU file fails at
FULL_F64_LAYERS = 20        # a case that compares more layers than this evaluates ONE image in float64 (VGG16: 35 layers)


def _hp(backbone, S):
    hp = helpers.hyper_params(backbone)
    if S == 512:
        hp["img_size"], hp["feature_map_shapes"] = 512, list(FMAPS_512)
    return hp


# ------------------------------------------------------------------ the shipped tables -> the cases
def family_of(config):
    """"dmah_2x2_2x2_ks2/s20" -> "dmah_ks2/split"."""
    tile, _, split = config.partition("/s")
    fam = [f for p, f in PREFIX.items() if tile.startswith(p)]
    assert len(fam) == 1, config
    return fam[0] + ("_ks2" if tile.endswith("_ks2") else "") + ("/split" if split and int(split) > 1 else "")


def shipped_tables(backbone, S, precision):
    """{B: {conv layer: "config[/sN]"}} of every shipped table of the net, size and precision."""
    import tuning
    hp = _hp(backbone, S)
    out = {}
    for f in sorted(os.listdir(tuning.SHIPPED_DIR)):
        mt = re.match(r"^%s_%d_.*_b(\d+)(_bf16)?\.tune$" % (backbone, S), f)
        if not mt or bool(mt.group(2)) != (precision == "bf16"):
            continue
        B = int(mt.group(1))
        key = tuning.table_key(backbone, S, hp["total_labels"], hp["aspect_ratios"], B) + ("_bf16" if precision == "bf16" else "")
        text = tuning.load_shipped(key)
        if text is None or key + ".tune" != f:
            continue
        lines = {}
        for l in tuning.body(text).splitlines():
            p = l.split(" ")
            if len(p) == 3 and p[1] != "image" and not p[0].startswith("__"):
                lines[p[0]] = p[1] + ("/s%s" % p[2] if int(p[2]) > 1 else "")
        out[B] = lines
    return out


def expected_run(lines, specs):
    """What ``m.layers(B)`` reports for the conv lines of a table: a ``dmah_*`` line runs only where EVERY LDS-DMA reader of
    its input tensor chose ``dmah_*`` and the tensor is a ReLU6 output (finalize_apply_preset, finalize_resolve_f16x2);
    elsewhere its ``dma3_*`` twin runs, the same tile and split-K."""
    relu6_out = {s["tout"] for s in specs if s.get("act") == "relu6"}
    readers = {}
    for s in specs:
        if s["kind"] in ("conv", "head") and lines.get(s["name"], "").startswith(("dma3_", "dmab_", "dmah_")):
            readers.setdefault(s["tin"], []).append(s["name"])
    run = dict(lines)
    for tensor, names in readers.items():
        if tensor in relu6_out and all(lines[n].startswith("dmah_") for n in names):
            continue
        for n in names:
            if lines[n].startswith("dmah_"):
                run[n] = "dma3_" + lines[n][len("dmah_"):].replace("_ks2", "")
    return run


def plan(backbone, S, precision, scope):
    """[(B, layers to compare or None = the whole scope)] in ascending B, and the (layer, family) set they cover."""
    specs = lg.layers(backbone, _hp(backbone, S))
    covered, cases = set(), []
    for B, lines in sorted(shipped_tables(backbone, S, precision).items()):
        pairs = {(n, family_of(c)) for n, c in expected_run(lines, specs).items() if n in scope}
        new = pairs - covered
        if new:
            cases.append((B, None if not cases else sorted({n for n, _ in new})))
            covered |= pairs
    return cases, covered


VGG_ALL = [s["name"] for s in lg.layers("vgg16", _hp("vgg16", 300))]
NETS = [("mobilenet_v2", 300, "fp32", MBV2_TAIL), ("mobilenet_v2", 512, "fp32", MBV2_TAIL), ("vgg16", 300, "fp32", VGG_ALL),
        ("mobilenet_v2", 300, "bf16", MBV2_TAIL), ("mobilenet_v2", 512, "bf16", MBV2_TAIL), ("vgg16", 300, "bf16", VGG_ALL)]
PLANNED = {}                # (backbone, S, precision) -> the (layer, family) set of its shipped tables


def _cases():
    c = []
    # all 66 layers of MobileNetV2-300, layer kernels only: the inference stem, the depthwise kernel, the BatchNorm epilogues.
    # (bf16: the smallest shipped bf16 table is B = 4; two images run on it)
    for precision, max_batch in (("fp32", 2), ("bf16", 4)):
        c.append(pytest.param(dict(backbone="mobilenet_v2", S=300, precision=precision, B=2, max_batch=max_batch, scope=None,
                                   layers=None, options=(("fuse_blocks", 0),), planned=False, twin=False),
                              id="mobilenet_v2-300-%s-all66-b2" % precision))
    for backbone, S, precision, scope in NETS:
        cases, PLANNED[(backbone, S, precision)] = plan(backbone, S, precision, scope)
        for i, (B, layers) in enumerate(cases):
            c.append(pytest.param(dict(backbone=backbone, S=S, precision=precision, B=B, max_batch=B, scope=scope, layers=layers,
                                       options=(), planned=True, twin=precision == "bf16" and S == 300 and i == 0),
                                  id="%s-%d-%s-b%d" % (backbone, S, precision, B)))
    return c


CASES = _cases()
SEEN = {}                   # (backbone, S, precision) -> {(layer, family)} collected from m.layers(B) of the compared layers
RAN = set()                 # ids of the cases that ran
RECORDS = []                # one per compared tensor: what the measured table is made of


# ------------------------------------------------------------------ one case
def _np(t):
    return t.detach().cpu().numpy()


def _forward(m, x, B):
    d, p = m(x)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(p).all())
    return _np(d).copy(), _np(p).copy()


def run_case(case):
    backbone, S, precision, B = case["backbone"], case["S"], case["precision"], case["B"]
    get_model = __import__("models.ssd_%s" % backbone, fromlist=["get_model"]).get_model
    torch.set_num_threads(min(16, torch.get_num_threads()))
    hp = _hp(backbone, S)
    w = helpers.synthetic_weights(backbone, hp)
    # MobileNetV2: the gain-8 images fire both clamps of every ReLU6 of the folded graph (asserted below on the oracle's maps)
    x = helpers.block_test_images(B, S, gain=8.0 if backbone == "mobilenet_v2" else 1.0)
    m = get_model(hp, max_batch=case["max_batch"], precision=precision)
    m.set_weights(w)
    for name, value in case["options"]:
        m.set_option(name, value)
    if precision == "bf16":
        m.set_option("plane_only", 0)
    deltas, probs = _forward(m, x, B)
    info = m.tuning_info
    assert info["source"] == "shipped" and info["choices_timed_on_device"] == 0 and info["reproducible"], info
    ran = {r["name"]: r for r in m.layers(B) if r["bytes"] > 0}
    specs = lg.layers(backbone, hp)
    scope = set(case["scope"] if case["scope"] is not None else [s["name"] for s in specs])
    wanted = scope if case["layers"] is None else set(case["layers"])
    only = {s["name"] for s in specs if s["name"] in wanted and s["name"] in ran}
    assert only == wanted, ("layers of the case that did not run", sorted(wanted - only))
    imgs = [0] if B == 1 else ([B - 1] if len(only) > FULL_F64_LAYERS and backbone == "vgg16" else [0, B - 1])
    shapes = lg.tensor_shapes(specs, w, S)
    N = deltas.shape[1]
    cache = {}

    def fetch(name):
        if name not in cache:
            if name == "input":
                a = x
            elif name in ("probs", "deltas"):
                a = probs if name == "probs" else deltas
            else:
                a = m.fetch_activation(name).reshape((B,) + shapes[name])
            cache[name] = np.ascontiguousarray(a[imgs])
        return cache[name]
    # output tensors kept as the two-plane fp16 pair only: fetch_planes reports 2 and the fetch IS the joined pair
    planes = {}
    for s in specs:
        if s["name"] in only and s.get("act") == "relu6" and s["kind"] == "conv":
            joined, npl = m.fetch_planes(s["tout"])
            if joined is not None and npl == 2 and np.array_equal(joined.view(np.uint32), m.fetch_activation(s["tout"]).view(np.uint32)):
                planes[s["tout"]] = 2
    report, yard = lg.Report(), {}
    frozen = {s["name"] for s in specs if s.get("bn")}
    res = lg.check_forward_graph(specs, fetch, w, hp, len(imgs), report, only=only, frozen=frozen, yardstick=yard, planes=planes,
                                 round_ops=lg.bf16_rne if precision == "bf16" else None)
    assert res["layers"] == len(only)
    tag = "%s-%d %s B=%d" % (backbone, S, precision, B)
    fails = ["%s: %s" % (tag, f) for f in report.fails]
    key = (backbone, S, precision)
    for s in specs:
        if s["name"] not in only:
            continue
        cfg = ran[s["name"]]["config"]
        fam = family_of(cfg) if cfg else ("dw" if s["kind"] == "dw" else s["kind"])
        if cfg and case["planned"]:
            SEEN.setdefault(key, set()).add((s["name"], fam))
        K = s["k"] ** 2 * shapes[s["tin"]][2] if s["kind"] in ("conv", "head") else 0
        for k in (("deltas", "probs") if s["kind"] == "head" else ("out",)):
            what = k + ":" + (s["tout"] or s["name"])
            E, rms = report.stats[(s["name"], what)]
            rec = dict(net=tag, layer=s["name"], key=k, config=cfg, family=fam, K=K, E=E, rms=rms, planes=planes.get(s["tout"], 0))
            line = "%-24s %-26s %-6s %-22s K %-5d max E %6.2f rms %.3f" % (tag, s["name"], k, cfg or fam, K, E, rms)
            if s["name"] in yard and k in RMS_KEYS:
                (m32, r32), (m16, r16) = yard[s["name"]][k]["r32"], yard[s["name"]][k]["r16"]
                bar = RMS_BARS.get(fam)
                rec.update(ratio=rms / r32, cap=r16 / (4.0 * r32), r16max=m16)
                line += "   ratio %.2f (bar %s)   r32 max %.2f rms %.3f   r16 max %.1f rms %.2f   cap %.1f" % (
                    rec["ratio"], bar, m32, r32, m16, r16, rec["cap"])
                if bar is None:
                    fails.append("%s %s %s [%s]: family %s has no RMS bar: measure it and add it to RMS_BARS" % (tag, s["name"], k, cfg, fam))
                    bar = min(RMS_BARS.values())
                if not bar * r32 <= r16 / 4.0:
                    fails.append("%s %s %s [%s]: the reference's cap rms(r16) / (4 rms(r32)) = %.2f is below the family's RMS bar %g" % (
                        tag, s["name"], k, cfg, rec["cap"], bar))
                if not rms <= bar * r32:
                    fails.append("%s %s %s [%s]: rms E = %.3f > RMS bar %g x rms(r32) %.3f (ratio %.2f); max E = %.2f (bar %g)" % (
                        tag, s["name"], k, cfg, rms, bar, r32, rec["ratio"], E, lg.E_BAR))
            if not E <= lg.E_BAR:
                fails.append("%s %s %s [%s]: max E = %.3g > %g; rms E = %.3g" % (tag, s["name"], k, cfg or fam, E, lg.E_BAR, rms))
            print(line + ("   two-plane output" if rec["planes"] == 2 else ""))
            RECORDS.append(rec)
    for name, (sixes, zeros) in res["clamps"].items():
        if sixes < MIN_SIXES or zeros < MIN_ZEROS:
            fails.append("%s %s: the oracle's ReLU6 map holds %.2f %% sixes and %.2f %% zeros" % (tag, name, 100 * sixes, 100 * zeros))
    if res["clamps"]:
        c = res["clamps"]
        print("%s ReLU6 maps: fewest sixes %.2f %%, fewest zeros %.2f %% over %d maps" % (
            tag, 100 * min(v[0] for v in c.values()), 100 * min(v[1] for v in c.values()), len(c)))
    if case["twin"]:
        # the same net with plane-only tensors (bf16 storage of every activation whose readers all take its planes)
        m.set_option("plane_only", 1)
        d1, p1 = _forward(m, x, B)
        assert m.tuning_info["choices_timed_on_device"] == 0
        if not (np.array_equal(d1.view(np.uint32), deltas.view(np.uint32)) and np.array_equal(p1.view(np.uint32), probs.view(np.uint32))):
            fails.append("%s: plane_only 1 differs from plane_only 0: deltas max |d| %.3g, probs %.3g" % (
                tag, np.abs(d1 - deltas).max(), np.abs(p1 - probs).max()))
    return report, res, fails


@pytest.mark.parametrize("case", CASES)
def test_inference_layers_vs_float64_layer_oracle(case, request):
    report, res, fails = run_case(case)
    RAN.add(request.node.callspec.id)
    if case["scope"] is None:
        assert res["layers"] == 66 and report.compared == 52 + 8 + 6 * 2 and len(res["clamps"]) == 35
    elif case["layers"] is None and case["backbone"] == "vgg16":
        assert res["layers"] == 35 and report.compared == 23 + 5 + 1 + 12
    elif case["layers"] is None:
        assert res["layers"] == 15 and report.compared == 9 + 12 and set(res["clamps"]) == {"Conv_1"}
    assert not fails, "\n".join(fails[:20])


def test_an_fp32_net_refuses_a_bf16_tile():
    """Sensitivity on the device, without a wrong kernel, would be one fp32 layer pinned onto a ``bf16_*`` / ``dmab_*`` tile.
    The table reader does not admit it (conv_config_allowed: fp32 nets never take the one-product tiles): such a line is
    dropped and the layer is timed on the device instead.  Asserted here for one MobileNetV2 head; the proof that the bars
    refuse the bf16 form in fp32 mode is mutant (c) of tests/test_layer_infer_cpu.py."""
    from models.ssd_mobilenet_v2 import get_model
    from test_plane_only_gpu import forced_table
    hp = _hp("mobilenet_v2", 300)
    for tile in ("bf16_2x2_2x2", "dmab_2x2_2x2"):
        m = get_model(hp, max_batch=2)
        m.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
        m.set_tuning(forced_table("mobilenet_v2", hp, 2, {"3_conv_heads": tile}))
        _forward(m, helpers.block_test_images(2, 300), 2)
        cfg = {r["name"]: r["config"] for r in m.layers(2)}["3_conv_heads"]
        assert m.tuning_info["choices_timed_on_device"] == 1 and not cfg.startswith(("bf16_", "dmab_")), (m.tuning_info, cfg)


def test_every_layer_family_pair_of_the_shipped_tables_was_reached():
    """The config strings collected through ``m.layers(B)`` hold every (layer, family) pair of every shipped table; the
    per-family summary the docstring's table is made of is printed.  Runs after the cases; needs the whole file."""
    if len(RAN) != len(CASES):
        pytest.skip("only %d of %d cases ran in this session" % (len(RAN), len(CASES)))
    for key, want in sorted(PLANNED.items()):
        assert want and want <= SEEN.get(key, set()), (key, sorted(want - SEEN.get(key, set())))
        print("%s-%d %s: %d (layer, family) pairs reached" % (key + (len(want),)))
    fams = {}
    for r in RECORDS:
        fams.setdefault(("bf16 " if " bf16 " in r["net"] else "") + r["family"], []).append(r)
    for f, rs in sorted(fams.items()):
        top = max(rs, key=lambda r: r["E"])
        with_ratio = [r for r in rs if "ratio" in r]
        line = "family %-18s tensors %3d   max E %5.2f (%s %s %s, K = %d)" % (f, len(rs), top["E"], top["net"], top["layer"], top["key"], top["K"])
        if with_ratio:
            tr = max(with_ratio, key=lambda r: r["ratio"])
            line += "   rms ratio %.2f (%s %s %s)   smallest cap %.1f" % (tr["ratio"], tr["net"], tr["layer"], tr["key"],
                                                                         min(r["cap"] for r in with_ratio))
        print(line)
