"""Protocol scoring on the device: ``ssd_eval_match_protocol`` / ``utils.eval_utils.match_detections_protocol``,
``DetectionEvaluator.update``, ``DecoderModel.evaluate(protocol=...)`` and ``predictor.main(eval_protocol=...)`` against the
serial oracle of tests/eval_protocol_cases.py.  Everything is exact: records, counts, states, zero tails, and the AP
floats -- no tolerance anywhere."""
import functools
import importlib

import numpy as np
import pytest
import torch

import eval_protocol_cases as pc
import helpers

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3


def _np(t):
    return t.detach().cpu().numpy()


# (B, T, G, NT), class count L (background included)
SHAPES = [((1, 1, 1, 1), 2), ((2, 0, 1, 1), 2), ((3, 257, 5, 1), 6), ((3, 40, 65, 10), 8), ((8, 200, 16, 10), 21),
          ((2, 1024, 256, 10), 8)]
IDS = ["x".join(map(str, s)) for s, _ in SHAPES]


def _thresholds(NT):
    return np.array([0.5], np.float32) if NT == 1 else pc.COCO_THRESHOLDS[:NT]


@functools.lru_cache(maxsize=None)
def _case(shape, L):
    """Inputs and both rules' oracle records of one shape, computed once and left unchanged."""
    B, T, G, NT = shape
    inputs = pc.planted(B, T, G, L)
    ref = {rule: pc.oracle_records(*inputs[:6], rule, _thresholds(NT)) for rule in ("voc", "coco")}
    pc.assert_not_vacuous(inputs[6], ref["voc"][5], ref["coco"][5], _thresholds(NT))
    return inputs, ref


def _raw_call(inputs, gi, rule_id, thresholds, B, T, G):
    """The C entry point on poisoned output buffers; returns the return code and the five buffers."""
    import ctypes
    import ssd_hip as h
    dev = h.device()
    pb, pl, ps, gt, gl = inputs[:5]
    d = [h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32),
         None if gi is None else h.to_dev(gi, dtype=torch.uint8)]
    NT = len(thresholds)
    thr = np.ascontiguousarray(thresholds, np.float32)
    rows = pb.shape[1]
    oc, od = [torch.full((max(B, 1), rows), -7, dtype=torch.int32, device=dev) for _ in range(2)]
    osc = torch.full((max(B, 1), rows), float("nan"), dtype=torch.float32, device=dev)
    ost = torch.full((max(B, 1), max(NT, 1), rows), -7, dtype=torch.int8, device=dev)
    on = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
    code = h.lib().ssd_eval_match_protocol(*[h.ptr(t) for t in d], B, T, G, rule_id,
                                           thr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), NT, h.ptr(oc), h.ptr(osc),
                                           h.ptr(od), h.ptr(ost), h.ptr(on), h.stream())
    torch.cuda.synchronize()
    return code, [_np(t) for t in (oc, osc, od, ost, on)]


@pytest.mark.parametrize("rule", ["voc", "coco"])
@pytest.mark.parametrize("shape,L", SHAPES, ids=IDS)
def test_records_vs_oracle(shape, L, rule):
    """Kernel records against the oracle's: class, score bits, the detection behind each record, count, the [B,NT,T]
    states and the zero tails.  Then the C entry point on poisoned buffers: fully overwritten, and the bytes of the
    first run (two runs, same bits)."""
    from utils import eval_utils as eu
    import ssd_hip as h
    B, T, G, NT = shape
    inputs, ref = _case(shape, L)
    pb, pl, ps, gt, gl, gi, names = inputs
    rc, rs, rd, rst, rn, events = ref[rule]
    print("oracle events:", events)
    if shape == (8, 200, 16, 10):
        assert sorted(names) == sorted(pc.CASES)
    thr = _thresholds(NT)
    gc, gs, gst, gn, gd = [_np(t) for t in eu.match_detections_protocol(pb, pl, ps, gt, gl, gi, rule, thr, return_indices=True)]
    assert gst.dtype == np.int8 and gst.shape == (B, NT, T)
    np.testing.assert_array_equal(gn, rn)
    np.testing.assert_array_equal(gd, rd)
    np.testing.assert_array_equal(gc, rc)
    np.testing.assert_array_equal(gs.view(np.uint32), rs.view(np.uint32))
    np.testing.assert_array_equal(gst, rst)
    tail = np.arange(T)[None] >= gn[:, None]
    assert not gc[tail].any() and not gd[tail].any() and not gs.view(np.uint32)[tail].any()
    assert not np.moveaxis(gst, 1, 0)[:, tail].any()
    code, raw = _raw_call(inputs, gi, {"voc": h.EVAL_RULE_VOC, "coco": h.EVAL_RULE_COCO}[rule], thr, B, T, G)
    assert code == 0
    for got, first in zip(raw, (gc, gs, gd, gst, gn)):
        assert got.tobytes() == first.tobytes()
    # without the index output: the same records
    again = [_np(t) for t in eu.match_detections_protocol(pb, pl, ps, gt, gl, gi, rule, thr)]
    for a, b in zip(again, (gc, gs, gst, gn)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("rule", ["voc", "coco"])
def test_null_ignore_equals_zero_flags(rule):
    """``gt_ignore=NULL`` == an all-zero flag array, and differs from the flagged run (the flags are read)."""
    from utils import eval_utils as eu
    shape, L = SHAPES[3]
    inputs, ref = _case(shape, L)
    pb, pl, ps, gt, gl, gi, _ = inputs
    thr = _thresholds(shape[3])
    none = [_np(t) for t in eu.match_detections_protocol(pb, pl, ps, gt, gl, None, rule, thr)]
    zero = [_np(t) for t in eu.match_detections_protocol(pb, pl, ps, gt, gl, np.zeros_like(gi), rule, thr)]
    want = pc.oracle_records(pb, pl, ps, gt, gl, None, rule, thr)
    for a, z in zip(none, zero):
        assert a.tobytes() == z.tobytes()
    np.testing.assert_array_equal(none[2], want[3])
    assert (want[3] != ref[rule][3]).any()


def test_b0_and_unsupported_sizes():
    """B == 0 returns 0 and writes nothing; T = 1025, G = 0, G = 257, NT = 0 and NT = 11 return SSD_E_UNSUPPORTED with
    an error text and no launch (the poison stays); ``DetectionEvaluator.update`` then takes the host walk."""
    import ssd_hip as h
    from utils import eval_utils as eu
    B, T, G, L = 2, 1025, 4, 6
    inputs = pc.planted(B, T, G, L)
    thr11 = np.float32(np.linspace(.4, .9, 11))
    code, out = _raw_call(inputs, inputs[5], 0, thr11[:1], 0, 40, G)
    assert code == 0 and all((o == -7).all() for o in (out[0], out[2], out[3], out[4])) and np.isnan(out[1]).all()
    for t_arg, g_arg, thr in ((T, G, thr11[:1]), (40, 0, thr11[:1]), (40, 257, thr11[:1]), (40, G, thr11[:0]), (40, G, thr11)):
        for rule_id in (h.EVAL_RULE_VOC, h.EVAL_RULE_COCO):
            code, out = _raw_call(inputs, inputs[5], rule_id, thr, B, t_arg, g_arg)
            assert code == UNSUPPORTED and b"ssd_eval_match_protocol" in h.lib().ssd_last_error(), (t_arg, g_arg, len(thr))
            assert all((o == -7).all() for o in (out[0], out[2], out[3], out[4])) and np.isnan(out[1]).all()
    pb, pl, ps, gt, gl, gi, _ = inputs
    with pytest.raises(h.SsdHipUnsupported):
        eu.match_detections_protocol(pb, pl, ps, gt, gl, gi)
    labels = pc.labels_for(L)
    ev = eu.DetectionEvaluator(labels, "voc07")
    assert ev.update(pb, pl, ps, gt, gl, gi) is None
    pc.assert_results_equal(ev.result(), pc.oracle_result([inputs[:6]], labels, "voc07")[0])


@pytest.mark.parametrize("protocol", ["voc07", "voc10", "coco"])
def test_evaluator_update_two_batches_vs_oracle(protocol):
    """``DetectionEvaluator.update`` over two batches of different widths (NumPy inputs, then device tensors) == the
    oracle's result dict: float64 equality for every AP, curve and the mAP."""
    import ssd_hip as h
    from utils import eval_utils as eu
    L = 8
    labels = pc.labels_for(L)
    batches = [pc.planted(5, 40, 9, L, seed=23)[:6], pc.planted(3, 25, 7, L, seed=24)[:6]]
    ref, events = pc.oracle_result(batches, labels, protocol)
    assert events["ignored_match"] >= 1 and 0 < ref["mAP"] < 1
    ev = eu.DetectionEvaluator(labels, protocol)
    ev.update(*batches[0])
    pb, pl, ps, gt, gl, gi = batches[1]
    ev.update(h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32),
              h.to_dev(gi, dtype=torch.uint8))
    pc.assert_results_equal(ev.result(), ref)


def _split_from_detections(b, l, s, batch):
    """Ground truth made from the model's own detections, so that a synthetic-weight model scores TPs: per image a copy
    of its best detection (a TP), a copy of its second marked difficult (ignored), and one far box of another class (a
    miss); everything else the model detects is an FP."""
    n = b.shape[0]
    gt = np.zeros((n, 4, 4), np.float32); gl = np.full((n, 4), -1, np.int32); gi = np.zeros((n, 4), np.uint8)
    for i in range(n):
        assert int((l[i] > 0).sum()) >= 3
        gt[i, 0], gl[i, 0] = b[i, 0], int(l[i, 0])
        gt[i, 1], gl[i, 1], gi[i, 1] = b[i, 1], int(l[i, 1]), 1
        gt[i, 2], gl[i, 2] = (0.0, 0.0, 0.05, 0.05), 1 + int(l[i, 0]) % 20
    return [(gt[k:k + batch], gl[k:k + batch], gi[k:k + batch]) for k in range(0, n, batch)]


@pytest.mark.parametrize("lanes", [1, 2])
def test_decoder_evaluate_protocols(lanes):
    """``DecoderModel.evaluate(protocol=p)`` for the three protocols (MobileNetV2, synthetic weights, batch 4, two
    batches, score threshold 0.01) == ``predict`` followed by the host oracle on the same detections; 3-tuple batches
    mean "nothing ignored"; ``protocol=None`` returns what it did before."""
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    from utils import bbox_utils
    from utils import eval_utils as eu
    hp = helpers.hyper_params("mobilenet_v2")
    model = get_model(hp, max_batch=4)
    model.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    images = [helpers.images(4, 300, seed=k) for k in (0, 1)]
    labels = pc.labels_for(21)
    dm = get_decoder_model(model, priors, hp, lanes=lanes, score_threshold=0.01)
    try:
        assert dm.decoder.score_threshold == 0.01 and dm.decoder.max_total_size == 200
        b, l, s = dm.predict(images)
        truth = _split_from_detections(b, l, s, 4)
        data4 = [(x,) + t for x, t in zip(images, truth)]
        data3 = [d[:3] for d in data4]
        for data, flagged in ((data4, True), (data3, False)):
            parts = [(b[k:k + 4], l[k:k + 4], s[k:k + 4]) + (t if flagged else t[:2] + (None,)) for k, t in zip((0, 4), truth)]
            for protocol in ("voc07", "voc10", "coco"):
                ref, events = pc.oracle_result(parts, labels, protocol)
                result, mean_ap = dm.evaluate(data, labels, protocol=protocol)
                pc.assert_results_equal(result, ref)
                assert mean_ap == result["mAP"] and 0 < mean_ap <= 1
                rule, thr = pc.PROTOCOLS[protocol]
                states = np.concatenate([pc.oracle_records(*p, rule, thr)[3][:, 0].ravel() for p in parts])
                assert (states == pc.TP).any() and (states == pc.FP).any()
                assert (states == pc.IGNORED).any() == flagged
        # steps: the first batch only
        first, _ = dm.evaluate(data4, labels, steps=1, protocol="voc07")
        pc.assert_results_equal(first, pc.oracle_result([(b[:4], l[:4], s[:4]) + truth[0]], labels, "voc07")[0])
        # protocol=None: the reference's scoring, as before
        stats, mean_ap = dm.evaluate(data3, labels)
        ref = eu.init_stats(labels)
        for k, (gt, gl, _) in zip((0, 4), truth):
            eu.update_stats(b[k:k + 4], l[k:k + 4], s[k:k + 4], gt, gl, ref)
        ref, ref_map = eu.calculate_mAP(ref)
        assert float(mean_ap) == float(ref_map)
        for cid in ref:
            assert stats[cid]["tp"] == ref[cid]["tp"] and stats[cid]["total"] == ref[cid]["total"]
        with pytest.raises(ValueError):
            dm.evaluate(data4, labels, protocol="voc12")
    finally:
        dm.close()


def test_predictor_main_eval_protocol(tmp_path, monkeypatch, capsys):
    """``predictor.main(evaluate=True, eval_protocol="voc07")`` on 8 synthetic items: the split keeps its difficult
    objects, the printed mAP and the returned result are the oracle's over the returned detections."""
    from utils import data_utils, train_utils
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "8")
    monkeypatch.delenv("SSD_VOC_DIR", raising=False)
    predictor = importlib.import_module("predictor")
    b, l, s, result = predictor.main(["--backbone", "mobilenet_v2"], evaluate=True, eval_protocol="voc07",
                                     eval_score_threshold=0.01, batch_size=4)
    out = capsys.readouterr().out
    assert b.shape[0] == 8 and int((l > 0).sum()) > 0
    labels = ["bg"] + data_utils.get_labels()
    size = train_utils.get_hyper_params("mobilenet_v2")["img_size"]
    raw = list(data_utils.synthetic_voc_items(8, len(labels)))
    items = (data_utils.preprocessing(x, size, size, evaluate=True, keep_difficult=True) for x in raw)
    parts = []
    for i, (_, gt, gl, gd) in enumerate(data_utils.padded_batch(items, 4, data_utils.get_padding_values())):
        parts.append((b[i * 4:(i + 1) * 4], l[i * 4:(i + 1) * 4], s[i * 4:(i + 1) * 4], gt, gl, gd))
    assert sum(int(p[5].sum()) for p in parts) == sum(int(np.sum(x["objects"]["is_difficult"])) for x in raw) > 0
    ref, _ = pc.oracle_result(parts, labels, "voc07")
    pc.assert_results_equal(result, ref)
    assert ("mAP (voc07): %s" % float(ref["mAP"])) in out
    with pytest.raises(ValueError):
        predictor.main(["--backbone", "mobilenet_v2"], evaluate=True, eval_protocol="devkit", batch_size=4)
