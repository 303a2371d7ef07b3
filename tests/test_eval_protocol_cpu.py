"""Protocol scoring on the host: the oracle of tests/eval_protocol_cases.py against states worked out by hand, the AP
definitions against hand values, ``utils.eval_utils``' host walk and ``DetectionEvaluator`` against the oracle, and the
``keep_difficult`` data path.  No device is involved."""
import numpy as np
import pytest
import torch

import eval_protocol_cases as pc

THR2 = np.array([0.5, 0.75], np.float32)


@pytest.mark.parametrize("rule", ["voc", "coco"])
def test_oracle_scene_against_hand_states(rule):
    """Every planted case, one record at a time: the scene's states at the thresholds 0.5 and 0.75 are the ones its
    comments derive from the text of the two rules; the rules disagree on r1, r2, r4 and r7."""
    pb, pl, ps, gt, gl, gi = pc.scene()
    rc, rs, rd, rst, rn, ev = pc.oracle_records(pb, pl, ps, gt, gl, gi, rule, THR2)
    assert rn.tolist() == [10]
    assert rd[0, :10].tolist() == pc.SCENE_DETS and rd[0, 10] == 0
    assert rc[0].tolist() == [1, 1, 1, 2, 2, 2, 2, 2, 3, 1, 0]
    np.testing.assert_array_equal(rs[0, :10], ps[0, pc.SCENE_DETS])
    assert rst[0, :, :10].tolist() == pc.SCENE_STATES[rule]
    assert not rst[0, :, 10].any()
    assert all(ev[k] >= 1 for k in pc.CASES if not k.startswith("all_")), ev
    differ = [r for r in range(10) if pc.SCENE_STATES["voc"][0][r] != pc.SCENE_STATES["coco"][0][r]]
    assert differ == [1, 2, 4, 7]


def test_oracle_scene_cases_one_by_one():
    """The single decisions behind the scene, by hand: IoU exactly 0.5 passes ``>=``; the first maximum wins under VOC,
    the later tie under COCO; NaN never matches; a class without a box is an FP."""
    pb, pl, ps, gt, gl, gi = pc.scene()
    iou = pc.iou_map(pb, gt)[0]
    assert iou[0, 0] == np.float32(0.5) and iou[0, 1] == np.float32(0.5)           # r0: A u B against A and against B
    assert iou[4, 2] == np.float32(1) and iou[4, 3] == np.float32(2) / np.float32(3)
    assert np.isnan(iou[10, 5]) and iou[10, 0] == 0
    ev = dict.fromkeys(pc.CASES, 0)
    # the tie alone, boxes A and B free: VOC takes A (state TP either way; the NEXT detection on A shows which)
    rows = iou[[0, 2]]                                                              # r0, then A exactly
    assert pc._walk_voc(rows, [0, 1, 5], gi[0], np.float32(0.5), ev) == [pc.TP, pc.FP]
    assert pc._walk_coco(rows, [0, 1, 5], gi[0], np.float32(0.5), ev) == [pc.TP, pc.TP]
    # just above the threshold nothing matches; at it, it does
    above = np.nextafter(np.float32(0.5), np.float32(1))
    assert pc._walk_voc(iou[[0]], [0, 1, 5], gi[0], above, ev) == [pc.FP]
    assert pc._walk_coco(iou[[0]], [0, 1, 5], gi[0], above, ev) == [pc.FP]
    # the ignored box: VOC answers "ignored" every time, COCO lets it absorb one detection
    assert pc._walk_voc(iou[[7, 8]], [2, 3, 4], gi[0], np.float32(0.5), ev) == [pc.IGNORED, pc.IGNORED]
    assert pc._walk_coco(iou[[7, 8]], [2, 3, 4], gi[0], np.float32(0.5), ev) == [pc.IGNORED, pc.FP]
    # NaN alone, no box at all
    assert pc._walk_voc(iou[[10]], [5], gi[0], np.float32(0.5), ev) == [pc.FP]
    assert pc._walk_coco(iou[[10]], [5], gi[0], np.float32(0.5), ev) == [pc.FP]
    assert pc._walk_voc(iou[[9]], [], gi[0], np.float32(0.5), ev) == [pc.FP]
    assert pc._walk_coco(iou[[9]], [], gi[0], np.float32(0.5), ev) == [pc.FP]


def _evaluator_for(states, scores, npos_labels, protocol, labels=("bg", "a", "b")):
    """A DetectionEvaluator fed one image of class-1 records with the given states at every threshold."""
    from utils import eval_utils as eu
    ev = eu.DetectionEvaluator(list(labels), protocol)
    NT = len(ev.iou_thresholds)
    n = len(states)
    rec_class = np.ones((1, n), np.int32)
    rec_state = np.repeat(np.array(states, np.int8)[None, None], NT, 1)
    ev.update_from_records(rec_class, np.array([scores], np.float32), rec_state, np.array([n], np.int32),
                           np.array([npos_labels], np.int32))
    return ev.result()


HAND_AP = {"voc07": 28.0 / 33.0, "voc10": 5.0 / 6.0, "coco": (51 + 50 * 2.0 / 3.0) / 101}


@pytest.mark.parametrize("protocol", ["voc07", "voc10", "coco"])
def test_ap_hand_values(protocol):
    """States [TP, FP, TP] with two boxes: recall [.5, .5, 1], precision [1, .5, 2/3].  voc07: six recall points see
    precision 1, five see 2/3 -> 28/33; voc10: .5 * 1 + .5 * 2/3 = 5/6; coco: 51 points at 1, 50 at 2/3.  An ignored
    record between them changes nothing; a class without boxes (class 2: AP NaN) stays out of the mean."""
    from utils import eval_utils as eu
    assert abs(HAND_AP["voc07"] - 0.848485) < 1e-6 and abs(HAND_AP["coco"] - 0.834983) < 1e-6
    res = _evaluator_for([1, 0, 1], [.9, .8, .7], [1, 1, -1], protocol)
    assert abs(res["classes"][1]["AP"] - HAND_AP[protocol]) <= 1e-12
    assert res["classes"][1]["npos"] == 2 and res["classes"][2]["npos"] == 0
    assert np.isnan(res["classes"][2]["AP"])
    assert res["mAP"] == res["classes"][1]["AP"]
    curve = (res["classes"][1]["recall"], res["classes"][1]["precision"])
    if protocol == "coco":
        assert len(curve[0]) == 10 and res["AP50"] == res["AP75"] == res["mAP"] and len(res["AP_per_threshold"]) == 10
        curve = (curve[0][0], curve[1][0])
    np.testing.assert_array_equal(curve[0], [.5, .5, 1.0])
    np.testing.assert_array_equal(curve[1], [1.0, .5, 2.0 / 3.0])
    assert curve[0].dtype == np.float64 and curve[1].dtype == np.float64
    with_ignored = _evaluator_for([1, -1, 0, -1, 1], [.9, .85, .8, .75, .7], [1, 1, -1], protocol)
    assert with_ignored["classes"][1]["AP"] == res["classes"][1]["AP"] and with_ignored["mAP"] == res["mAP"]
    # the oracle's own definitions give the same numbers
    assert abs(pc.AP_FUNCTIONS[protocol](np.array([.5, .5, 1.0]), np.array([1.0, .5, 2.0 / 3.0])) - HAND_AP[protocol]) <= 1e-12
    # no record at all for a class with boxes: AP 0; ignored boxes are not counted
    from_nothing = eu.DetectionEvaluator(["bg", "a"], protocol)
    NT = len(from_nothing.iou_thresholds)
    from_nothing.update_from_records(np.zeros((1, 0), np.int32), np.zeros((1, 0), np.float32), np.zeros((1, NT, 0), np.int8),
                                     np.zeros((1,), np.int32), np.array([[1, 1, 1]]), np.array([[0, 1, 0]], np.uint8))
    out = from_nothing.result()
    assert out["classes"][1]["npos"] == 2 and out["classes"][1]["AP"] == 0.0 and out["mAP"] == 0.0
    assert np.isnan(eu.DetectionEvaluator(["bg", "a"], protocol).result()["mAP"])


def test_tied_scores_keep_image_record_order():
    """Equal scores: the stable sort keeps (image, record) order, so [TP, FP] and [FP, TP] give different curves."""
    first = _evaluator_for([1, 0], [.5, .5], [1], "voc10")
    second = _evaluator_for([0, 1], [.5, .5], [1], "voc10")
    np.testing.assert_array_equal(first["classes"][1]["precision"], [1.0, .5])
    np.testing.assert_array_equal(second["classes"][1]["precision"], [0.0, .5])


SHAPES = [(1, 11, 6, 4), (5, 40, 9, 6), (3, 70, 16, 21), (4, 0, 3, 5), (3, 1, 1, 2)]


@pytest.mark.parametrize("rule,thresholds", [("voc", (0.5,)), ("coco", (0.5,)), ("coco", pc.COCO_THRESHOLDS), ("voc", THR2)],
                         ids=["voc", "coco1", "coco10", "voc2"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_host_walk_equals_oracle(shape, rule, thresholds):
    """``match_detections_protocol_host`` (the fallback for sizes the kernel refuses) == the oracle, bit for bit, and
    its own fp32 IoU is the oracle's."""
    from utils import eval_utils as eu
    B, T, G, L = shape
    pb, pl, ps, gt, gl, gi, names = pc.planted(B, T, G, L)
    ref = pc.oracle_records(pb, pl, ps, gt, gl, gi, rule, thresholds)
    other = pc.oracle_records(pb, pl, ps, gt, gl, gi, "coco" if rule == "voc" else "voc", thresholds)
    pc.assert_not_vacuous(names, *((ref[5], other[5]) if rule == "voc" else (other[5], ref[5])), thresholds)
    if shape == (5, 40, 9, 6):
        assert sorted(names) == sorted(pc.CASES)
    got = eu.match_detections_protocol_host(pb, pl, ps, gt, gl, gi, rule, thresholds, return_indices=True)
    for g, r in zip(got, (ref[0], ref[1].view(np.uint32), ref[3], ref[4], ref[2])):
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, r)
    assert got[2].dtype == np.int8 and got[2].shape == (B, len(thresholds), T)
    for b in range(B):
        np.testing.assert_array_equal(eu._iou_fp32(pb[b], gt[b]).view(np.uint32), pc.iou_map(pb, gt)[b].view(np.uint32))
    # no flags == all-zero flags
    none = eu.match_detections_protocol_host(pb, pl, ps, gt, gl, None, rule, thresholds)
    zero = eu.match_detections_protocol_host(pb, pl, ps, gt, gl, np.zeros_like(gi), rule, thresholds)
    for a, z in zip(none, zero):
        np.testing.assert_array_equal(a, z)


@pytest.mark.parametrize("protocol", ["voc07", "voc10", "coco"])
def test_evaluator_from_host_records_equals_oracle(protocol):
    """Two batches of different widths through the host walk and ``update_from_records``: the oracle's result dict,
    float64 for float64."""
    from utils import eval_utils as eu
    L = 6
    labels = pc.labels_for(L)
    batches = [pc.planted(5, 40, 9, L, seed=23)[:6], pc.planted(3, 25, 7, L, seed=24)[:6]]
    ref, events = pc.oracle_result(batches, labels, protocol)
    assert events["ignored_match"] >= 1 and 0 < ref["mAP"] < 1
    ev = eu.DetectionEvaluator(labels, protocol)
    rule, thr = pc.PROTOCOLS[protocol]
    assert ev.rule == rule
    np.testing.assert_array_equal(ev.iou_thresholds, thr)
    for pb, pl, ps, gt, gl, gi in batches:
        ev.update_from_records(*eu.match_detections_protocol_host(pb, pl, ps, gt, gl, gi, rule, thr), gl, gi)
    pc.assert_results_equal(ev.result(), ref)


def test_unknown_names_raise():
    from utils import eval_utils as eu
    pb, pl, ps, gt, gl, gi = pc.scene()
    with pytest.raises(ValueError):
        eu.DetectionEvaluator(["bg", "a"], "voc12")
    with pytest.raises(ValueError):
        eu.protocol_spec(None)
    with pytest.raises(ValueError):
        eu.match_detections_protocol_host(pb, pl, ps, gt, gl, gi, rule="devkit")
    with pytest.raises(ValueError):
        eu.match_detections_protocol(pb, pl, ps, gt, gl, gi, rule="devkit")        # refused before any device call
    with pytest.raises(ValueError):
        eu.average_precision([1.0], [1.0], "voc2012")
    with pytest.raises(KeyError):
        eu.DetectionEvaluator(["bg", "a"], "voc07").update_from_records(
            np.array([[2]], np.int32), np.array([[.5]], np.float32), np.zeros((1, 1, 1), np.int8), np.array([1]), np.array([[1]]))


def test_get_decoder_model_defaults_unchanged():
    """Without the new keywords the decoder keeps the reference's 0.5 / 200."""
    from models.decoder import SSDDecoder, get_decoder_model

    class Base(object):
        pass
    dm = get_decoder_model(Base(), np.zeros((4, 4), np.float32), {"variances": [0.1, 0.1, 0.2, 0.2]}, lanes=1)
    ref = SSDDecoder(np.zeros((4, 4), np.float32), [0.1, 0.1, 0.2, 0.2])
    assert (dm.decoder.score_threshold, dm.decoder.max_total_size) == (ref.score_threshold, ref.max_total_size) == (0.5, 200)
    dm = get_decoder_model(Base(), np.zeros((4, 4), np.float32), {"variances": [0.1, 0.1, 0.2, 0.2]}, lanes=1,
                           score_threshold=0.01, max_total_size=100)
    assert (dm.decoder.score_threshold, dm.decoder.max_total_size) == (0.01, 100)


# ------------------------------------------------------------------------------------------------ the data path
def _items(n=5, L=6):
    from utils import data_utils
    return list(data_utils.synthetic_voc_items(n, L, seed=4))


def _host_preprocessing(monkeypatch):
    """``preprocessing`` without a device: the resize call answers 0 and leaves its (host) output tensor as it is."""
    import ssd_hip

    class Lib(object):
        @staticmethod
        def ssd_preprocess(*args):
            return 0
    monkeypatch.setattr(ssd_hip, "_lib", Lib())
    monkeypatch.setattr(ssd_hip, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(ssd_hip, "stream", lambda: None)


def test_preprocessing_keep_difficult(monkeypatch):
    """4-tuples with ``keep_difficult``: every object stays, whatever ``evaluate`` says, and flag i belongs to box i;
    3-tuples otherwise, ``evaluate=True`` still drops the difficult objects."""
    from utils import data_utils
    _host_preprocessing(monkeypatch)
    items = _items()
    assert any(np.asarray(it["objects"]["is_difficult"]).any() for it in items)
    for it in items:
        diff = np.asarray(it["objects"]["is_difficult"], bool)
        for evaluate in (False, True):
            out = data_utils.preprocessing(it, 8, 8, evaluate=evaluate, keep_difficult=True)
            assert len(out) == 4 and out[3].dtype == np.uint8
            np.testing.assert_array_equal(out[1], np.asarray(it["objects"]["bbox"], np.float32))
            np.testing.assert_array_equal(out[2], np.asarray(it["objects"]["label"]) + 1)
            np.testing.assert_array_equal(out[3], diff.astype(np.uint8))
        dropped = data_utils.preprocessing(it, 8, 8, evaluate=True)
        assert len(dropped) == 3 and len(dropped[1]) == int((~diff).sum())
        np.testing.assert_array_equal(dropped[1], np.asarray(it["objects"]["bbox"], np.float32)[~diff])
        assert len(data_utils.preprocessing(it, 8, 8)) == 3


def test_padded_batch_and_voc_batches_flags(monkeypatch):
    """``padded_batch`` and ``voc_batches`` yield the flags as uint8 [B,G], 0 where the labels are padding, aligned with
    the boxes; without ``keep_difficult`` both yield 3-tuples as before."""
    from utils import data_utils
    _host_preprocessing(monkeypatch)
    monkeypatch.setattr(data_utils, "preprocess_ragged_batch", lambda images, h, w: torch.zeros((len(images), h, w, 3)))
    items = _items()
    kept = list(data_utils.padded_batch((data_utils.preprocessing(it, 8, 8, evaluate=True, keep_difficult=True) for it in items), 3))
    plain = list(data_utils.padded_batch((data_utils.preprocessing(it, 8, 8, evaluate=True) for it in items), 3))
    streamed = list(data_utils.voc_batches(items, 3, 8, 8, evaluate=True, keep_difficult=True, workers=1))
    streamed_plain = list(data_utils.voc_batches(items, 3, 8, 8, evaluate=True, workers=1))
    assert [len(b) for b in kept] == [4, 4] and [len(b) for b in plain] == [3, 3]
    assert [len(b) for b in streamed] == [4, 4] and [len(b) for b in streamed_plain] == [3, 3]
    for batches in (kept, streamed):
        i = 0
        for _, gt, gl, gd in batches:
            assert gd.dtype == np.uint8 and gd.shape == gl.shape and gt.shape == gl.shape + (4,)
            assert not gd[gl == -1].any()
            for row in range(gl.shape[0]):
                obj = items[i]["objects"]
                n = len(obj["label"])
                np.testing.assert_array_equal(gd[row, :n], np.asarray(obj["is_difficult"], bool).astype(np.uint8))
                np.testing.assert_array_equal(gt[row, :n], np.asarray(obj["bbox"], np.float32))
                np.testing.assert_array_equal(gl[row, :n], np.asarray(obj["label"]) + 1)
                assert (gl[row, n:] == -1).all()
                i += 1
        assert i == len(items)
    for (_, gt, gl), (_, gt2, gl2) in zip(plain, streamed_plain):
        np.testing.assert_array_equal(gt, gt2)
        np.testing.assert_array_equal(gl, gl2)
        assert gl.shape[1] <= max(b[2].shape[1] for b in kept)
