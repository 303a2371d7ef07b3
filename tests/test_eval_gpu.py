"""N2 on the device: ``ssd_eval_match`` / ``utils.eval_utils.match_detections``,
``update_stats_device``, ``DecoderModel.evaluate`` and ``predictor.main(evaluate=True)`` against
``oracle.eval_oracle.update_stats`` and the host ``update_stats``.  Everything is exact: records, counts, visit order,
stats lists and the mAP float -- no tolerance anywhere."""
import copy
import ctypes
import importlib

import numpy as np
import pytest
import torch

import eval_cases as ec
import helpers
from oracle import eval_oracle as eo

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


# (shape, least TPs, least FPs asserted on the oracle's records).  20 / 20 where the shape allows; G = 1 holds at
# most one TP per image (5 images of the 8 have a real box), T = 1 at most 8 records in all.
SHAPES = [((12, 40, 8, 6), 20, 20), ((64, 200, 16, 21), 20, 20), ((8, 40, 1, 6), 3, 20), ((8, 1, 8, 6), 1, 1)]


@pytest.mark.parametrize("shape,min_tp,min_fp", SHAPES, ids=["12x40x8", "64x200x16", "G1", "T1"])
def test_eval_match_records_vs_oracle(shape, min_tp, min_fp):
    """Kernel records against the records read off the oracle's own walk: class, score, TP flag, the detection
    behind each record (= visit order), counts, zero tails.  Inputs hold duplicates (tied IoU), an IoU of exactly
    0.5, NaN rows, an all-label-0 image and an all-padding image (tests/eval_cases.py)."""
    from utils import eval_utils as eu
    B, T, G, L = shape
    pb, pl, ps, gt, gl, where = ec.case(B, T, G, L)
    rc, rs, rt, rd, rn = ec.oracle_records(pb, pl, ps, gt, gl)
    n_tp, n_fp, taken, ties = ec.assert_not_vacuous(pb, pl, gt, gl, rt, rd, rn, min_tp, min_fp, want_tie=T > 1,
                                                    want_taken=T > 1)
    print("oracle: %d TPs, %d FPs, %d eligible-but-taken, %d ties" % (n_tp, n_fp, taken, ties))
    gc, gs, gtp, gn, gd = [_np(t) for t in eu.match_detections(pb, pl, ps, gt, gl, return_indices=True)]
    np.testing.assert_array_equal(gn, rn)
    np.testing.assert_array_equal(gd, rd)
    np.testing.assert_array_equal(gc, rc)
    np.testing.assert_array_equal(gtp, rt)
    np.testing.assert_array_equal(gs.view(np.uint32), rs.view(np.uint32))
    tail = np.arange(T)[None] >= gn[:, None]
    assert not gc[tail].any() and not gtp[tail].any() and not gd[tail].any() and not gs.view(np.uint32)[tail].any()
    # without the index output: the same records
    again = [_np(t) for t in eu.match_detections(pb, pl, ps, gt, gl)]
    for a, b in zip(again, (gc, gs, gtp, gn)):
        np.testing.assert_array_equal(a, b)
    # the IoU the kernel decided on is ssd_iou_map's: the host path on the same inputs gives the same stats
    labels = ec.labels_for(L)
    ref = eo.update_stats(pb, pl, ps, gt, gl, eo.init_stats(labels))
    ec.assert_stats_equal(eu.stats_from_records(gc, gs, gtp, gn, gl, eu.init_stats(labels)), ref)


def test_eval_match_outputs_fully_overwritten_and_b0():
    """Poisoned output buffers come back fully written; B == 0 is a no-op that returns 0."""
    import ssd_hip as h
    B, T, G, L = 12, 40, 8, 6
    pb, pl, ps, gt, gl, _ = ec.case(B, T, G, L)
    rc, rs, rt, rd, rn = ec.oracle_records(pb, pl, ps, gt, gl)
    dev = h.device()
    d = [h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32)]
    oc, ot, od = [torch.full((B, T), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    osc = torch.full((B, T), float("nan"), dtype=torch.float32, device=dev)
    on = torch.full((B,), -7, dtype=torch.int32, device=dev)
    lib = h.lib()
    rcode = lib.ssd_eval_match(*[h.ptr(t) for t in d], B, T, G, 0.5, h.ptr(oc), h.ptr(osc), h.ptr(ot), h.ptr(od), h.ptr(on),
                               h.stream())
    assert rcode == 0
    for got, ref in ((oc, rc), (ot, rt), (od, rd), (on, rn), (osc, rs)):
        np.testing.assert_array_equal(_np(got), ref)
    assert lib.ssd_eval_match(*[h.ptr(t) for t in d], 0, T, G, 0.5, h.ptr(oc), h.ptr(osc), h.ptr(ot), h.ptr(od), h.ptr(on),
                              h.stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(on), rn)


@pytest.mark.parametrize("shape", [(12, 40, 8, 6), (64, 200, 16, 21)], ids=["12x40x8", "64x200x16"])
def test_update_stats_device_vs_host_and_oracle(shape):
    """``update_stats_device`` == ``update_stats`` == the oracle, lists and mAP, from NumPy inputs and from device
    tensors; two calls accumulate like the host path."""
    import ssd_hip as h
    from utils import eval_utils as eu
    B, T, G, L = shape
    pb, pl, ps, gt, gl, _ = ec.case(B, T, G, L)
    labels = ec.labels_for(L)
    ref = eo.update_stats(pb, pl, ps, gt, gl, eo.init_stats(labels))
    host = eu.update_stats(pb, pl, ps, gt, gl, eu.init_stats(labels))
    ec.assert_stats_equal(host, ref)
    from_numpy = eu.update_stats_device(pb, pl, ps, gt, gl, eu.init_stats(labels))
    ec.assert_stats_equal(from_numpy, ref)
    dev = [h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32)]
    from_device = eu.update_stats_device(*dev, eu.init_stats(labels))
    ec.assert_stats_equal(from_device, ref)
    halves = eu.init_stats(labels)
    k = B // 2
    eu.update_stats_device(pb[:k], pl[:k], ps[:k], gt[:k], gl[:k], halves)
    eu.update_stats_device(*[t[k:] for t in dev], halves)
    ec.assert_stats_equal(halves, ref)
    ref, rm = eo.calculate_mAP(ref)
    for got in (host, from_numpy, from_device, halves):
        got, gm = eu.calculate_mAP(got)
        assert float(gm) == float(rm)
        for cid in ref:
            assert got[cid]["AP"] == ref[cid]["AP"]
    assert float(rm) > 0


def test_eval_match_unsupported_sizes_fall_back():
    """Argument validation only: T beyond the header's limit (1024) or G outside 1..256 gets SSD_E_UNSUPPORTED and
    an error text before any launch (the output buffers keep their poison); ``update_stats_device`` then takes the
    host path and still returns the oracle's stats."""
    import ssd_hip as h
    from utils import eval_utils as eu
    B, T, G, L = 5, 1025, 4, 6
    pb, pl, ps, gt, gl, _ = ec.case(B, T, G, L)
    dev = h.device()
    d = [h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32)]
    out = [torch.full((B, T), -7, dtype=torch.int32, device=dev) for _ in range(4)]
    on = torch.full((B,), -7, dtype=torch.int32, device=dev)
    lib = h.lib()
    for t_arg, g_arg in ((T, G), (40, 257), (40, 0)):
        rcode = lib.ssd_eval_match(*[h.ptr(t) for t in d], B, t_arg, g_arg, 0.5, h.ptr(out[0]), h.ptr(out[1].view(torch.float32)),
                                   h.ptr(out[2]), h.ptr(out[3]), h.ptr(on), h.stream())
        assert rcode == -3 and b"ssd_eval_match" in lib.ssd_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out + [on])
    with pytest.raises(h.SsdHipUnsupported):
        eu.match_detections(pb, pl, ps, gt, gl)
    labels = ec.labels_for(L)
    ref = eo.update_stats(pb, pl, ps, gt, gl, eo.init_stats(labels))
    ec.assert_stats_equal(eu.update_stats_device(pb, pl, ps, gt, gl, eu.init_stats(labels)), ref)
    # the largest supported sizes run
    B, T, G, L = 5, 1024, 256, 6
    pb, pl, ps, gt, gl, _ = ec.case(B, T, G, L)
    rc, rs, rt, rd, rn = ec.oracle_records(pb, pl, ps, gt, gl)
    gc, gs, gtp, gn, gd = [_np(t) for t in eu.match_detections(pb, pl, ps, gt, gl, return_indices=True)]
    for got, ref in ((gc, rc), (gs, rs), (gtp, rt), (gn, rn), (gd, rd)):
        np.testing.assert_array_equal(got, ref)


def _compare_final_stats(got, ref):
    ec.assert_stats_equal(got, ref)
    for cid in ref:
        assert float(got[cid]["AP"]) == float(ref[cid]["AP"]), cid
        np.testing.assert_array_equal(np.asarray(got[cid]["recall"]), np.asarray(ref[cid]["recall"]))
        np.testing.assert_array_equal(np.asarray(got[cid]["precision"]), np.asarray(ref[cid]["precision"]))


@pytest.mark.parametrize("lanes", [1, 2])
def test_evaluate_equals_predict_then_evaluate_predictions(lanes, capsys):
    """``DecoderModel.evaluate`` (matching on the lane's stream, records copied out once) == ``predict`` +
    ``evaluate_predictions`` on the host path of the same model: stats list for list, mAP float for float.  The
    batches' ground truth is unrelated to the image seeds, so the mAP may be near 0: the equality is the check."""
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    from utils import bbox_utils, data_utils
    from utils import eval_utils as eu
    hp = helpers.hyper_params("mobilenet_v2")
    model = get_model(hp, max_batch=8)
    model.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    data = list(data_utils.synthetic_dataset(40, 8))
    assert len(data) == 5
    labels = ["bg"] + data_utils.get_labels()
    dm = get_decoder_model(model, priors, hp, lanes=lanes)
    try:
        stats, mean_ap = dm.evaluate(data, labels)
        b, l, s = dm.predict(data)
        assert int((l > 0).sum()) > 0
        # the parent's host path: update_stats over the same batches
        ref = eu.init_stats(labels)
        for i, (_, gt, gl) in enumerate(data):
            eu.update_stats(b[i * 8:(i + 1) * 8], l[i * 8:(i + 1) * 8], s[i * 8:(i + 1) * 8], gt, gl, ref)
        assert sum(len(r["tp"]) for r in ref.values()) == int((l > 0).sum())
        ref, ref_map = eu.calculate_mAP(ref)
        _compare_final_stats(stats, ref)
        assert float(mean_ap) == float(ref_map)
        # ... and evaluate_predictions as shipped (device matching from host arrays)
        capsys.readouterr()
        shipped = eu.evaluate_predictions(data, b, l, s, labels, 8)
        assert ("mAP: %s" % float(ref_map)) in capsys.readouterr().out
        _compare_final_stats(shipped, ref)
        # steps: the first three batches only
        part, _ = dm.evaluate(data, labels, steps=3)
        ref3 = eu.init_stats(labels)
        for i, (_, gt, gl) in enumerate(data[:3]):
            eu.update_stats(b[i * 8:(i + 1) * 8], l[i * 8:(i + 1) * 8], s[i * 8:(i + 1) * 8], gt, gl, ref3)
        _compare_final_stats(part, eu.calculate_mAP(ref3)[0])
    finally:
        dm.close()


def test_predictor_evaluate_equals_host_update_stats(tmp_path, monkeypatch, capsys):
    """``predictor.main(evaluate=True)`` returns the stats the host ``update_stats`` gives over its own returned
    boxes and the same data."""
    from utils import data_utils, train_utils
    from utils import eval_utils as eu
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "14")
    predictor = importlib.import_module("predictor")
    b, l, s, stats = predictor.main(["--backbone", "mobilenet_v2"], evaluate=True, batch_size=4)
    out = capsys.readouterr().out
    assert b.shape[0] == 14 and int((l > 0).sum()) > 0
    labels = ["bg"] + data_utils.get_labels()
    size = train_utils.get_hyper_params("mobilenet_v2")["img_size"]
    items = (data_utils.preprocessing(x, size, size, evaluate=True) for x in data_utils.synthetic_voc_items(14, len(labels)))
    ref = eu.init_stats(labels)
    for i, (_, gt, gl) in enumerate(data_utils.padded_batch(items, 4, data_utils.get_padding_values())):
        eu.update_stats(b[i * 4:(i + 1) * 4], l[i * 4:(i + 1) * 4], s[i * 4:(i + 1) * 4], gt, gl, ref)
    ref, ref_map = eu.calculate_mAP(ref)
    _compare_final_stats(stats, ref)
    assert ("mAP: %s" % float(ref_map)) in out
