"""Soft-NMS / class-agnostic suppression on the GPU against the float64 oracle of tests/soft_nms_cases.py (its docstring
states the bars), and the net's predict path with a config: one net, alternating configs, graphs, lanes."""
import numpy as np
import pytest
import torch

import helpers
import soft_nms_cases as sc
from test_bbox_gpu import TOL

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _config(case):
    import ssd_hip
    return ssd_hip.nms_config(case.method, case.agnostic, case.max_per_class, case.max_total, case.iou_threshold,
                              case.score_threshold, case.sigma, case.clip)


def run_raw(case, cfg=None):
    """``ssd_combined_nms_cfg`` with the kept indices (``bbox_utils.non_max_suppression`` does not return them)."""
    import ssd_hip as h
    lib = h.lib()
    cfg = cfg or _config(case)
    B, N, C = case.scores.shape
    T = case.max_total
    bd, sd = h.to_dev(case.boxes), h.to_dev(case.scores)
    dev = h.device()
    ob = torch.full((B, T, 4), 7.0, device=dev)
    osc, oc = torch.full((B, T), 7.0, device=dev), torch.full((B, T), 7.0, device=dev)
    v = torch.full((B,), 77, dtype=torch.int32, device=dev)
    ki = torch.full((B, T), 77, dtype=torch.int32, device=dev)
    ws = h.workspace(lib.ssd_decode_nms_cfg_workspace_bytes(B, N, C, cfg))
    h.check(lib.ssd_combined_nms_cfg(h.ptr(bd), h.ptr(sd), B, N, C, cfg, h.ptr(ob), h.ptr(osc), h.ptr(oc), h.ptr(v), h.ptr(ki),
                                     h.ptr(ws), ws.numel(), h.stream()), "ssd_combined_nms_cfg")
    return _np(ob), _np(osc), _np(oc), _np(v), _np(ki)


RAW = [n for n in sc.names() if not n.startswith("decoder")]


@pytest.mark.parametrize("name", RAW)
def test_raw_form_against_the_oracle(name):
    case = sc.by_name(name)
    ob, osc, oc, v, ki = run_raw(case)
    sc.check(case, ob, osc, oc, v, ki)


def test_through_non_max_suppression():
    from utils import bbox_utils
    case = sc.by_name("agnostic_gaussian")
    ob, osc, oc, v = bbox_utils.non_max_suppression(
        case.boxes[:, :, None, :], case.scores, max_output_size_per_class=case.max_per_class, max_total_size=case.max_total,
        iou_threshold=case.iou_threshold, score_threshold=case.score_threshold, nms_method="gaussian",
        soft_nms_sigma=case.sigma, class_agnostic=True)
    sc.check(case, _np(ob), _np(osc), _np(oc), _np(v))
    for method, iou_thr, sigma, want in sc.known_answers():
        ob, osc, oc, v = bbox_utils.non_max_suppression(
            sc.KNOWN_BOXES[:, :, None, :], sc.KNOWN_SCORES, max_output_size_per_class=3, max_total_size=3, iou_threshold=iou_thr,
            score_threshold=0.1, clip_boxes=False, nms_method=method, soft_nms_sigma=sigma)
        assert _np(v).tolist() == [len(want)]
        np.testing.assert_allclose(_np(osc)[0, :len(want)], [s for _, s in want], rtol=5e-7)
        np.testing.assert_array_equal(_np(ob)[0, :len(want)], sc.KNOWN_BOXES[0, [a for a, _ in want]])


def test_planted_ties_come_out_as_stated():
    for m, copy in (("linear", 0.0), ("gaussian", 0.9 * np.exp(-1.0))):        # sigma 0.5: exp(-0.5 / 0.5 * 1^2)
        case = sc.by_name("planted_%s" % m)
        ob, osc, oc, v, ki = run_raw(case)
        assert v.tolist() == [6]
        order = ki[0].tolist()
        assert order[0] == 0 and order[1:4] == [2, 3, 4]                        # equal scores on disjoint boxes: lower index first
        np.testing.assert_allclose(osc[0, order.index(1)], copy, rtol=5e-7, atol=0)
        assert osc[0, 0] == np.float32(0.9) and (osc[0, 1:4] == np.float32(0.6)).all()


def test_empty_batch_and_no_anchors():
    import ssd_hip as h
    from utils import bbox_utils
    for B, N in ((0, 10), (2, 0)):
        ob, osc, oc, v = bbox_utils.non_max_suppression(np.zeros((B, N, 1, 4), np.float32), np.zeros((B, N, 3), np.float32),
                                                        max_output_size_per_class=4, max_total_size=5, nms_method="gaussian",
                                                        class_agnostic=bool(N))
        assert ob.shape == (B, 5, 4) and not _np(osc).any() and not _np(v).any()
    with pytest.raises(h.SsdHipUnsupported):               # the hard kernel's LDS limit on max_per_class, kept
        bbox_utils.non_max_suppression(np.zeros((1, 20000, 1, 4), np.float32), np.zeros((1, 20000, 1), np.float32),
                                       max_output_size_per_class=20000, max_total_size=5, nms_method="linear")


def _decoder(case, **kw):
    from models.decoder import SSDDecoder
    return SSDDecoder(case.priors, case.var, max_total_size=case.max_total, score_threshold=case.score_threshold,
                      iou_threshold=case.iou_threshold, nms_method=case.method, soft_nms_sigma=case.sigma,
                      class_agnostic=case.agnostic, **kw)


@pytest.mark.parametrize("name", ["decoder_gaussian_050", "decoder_gaussian_001", "decoder_agnostic_hard"])
def test_decoder_form_against_the_oracle(name):
    case = sc.by_name(name)
    dec = _decoder(case)
    b, l, s = dec([case.deltas, case.scores], return_indices=True)
    sc.check(case, _np(b), _np(s), _np(l), _np(dec.last_valid_detections), _np(dec.last_kept_indices), box_tol=TOL)
    b2, l2, s2 = dec([case.deltas, case.scores])                                # without the indices: the same rows
    for x, y in ((b, b2), (l, l2), (s, s2)):
        np.testing.assert_array_equal(_np(x), _np(y))


def test_hard_per_class_through_cfg_is_the_old_entry_point():
    import ssd_hip as h
    from models.decoder import SSDDecoder
    from utils import bbox_utils
    lib = h.lib()
    raw = sc.by_name("raw_gaussian_0")._replace(method="hard")
    want = bbox_utils.non_max_suppression(raw.boxes[:, :, None, :], raw.scores, max_output_size_per_class=raw.max_per_class,
                                          max_total_size=raw.max_total, score_threshold=raw.score_threshold)
    ob, osc, oc, v, _ = run_raw(raw)
    for x, y in zip((ob, osc, oc, v), want):
        np.testing.assert_array_equal(x, _np(y))
    case = sc.by_name("decoder_gaussian_050")
    dec = SSDDecoder(case.priors, case.var)
    wb, wl, wsc = dec([case.deltas, case.scores], return_indices=True)
    B, N, L = case.scores.shape
    T = 200
    cfg = h.nms_config("hard", False, T, T, 0.5, 0.5)
    dd, pd, pri = h.to_dev(case.deltas), h.to_dev(case.scores), h.to_dev(case.priors)
    dev = h.device()
    b, l, s = torch.empty((B, T, 4), device=dev), torch.empty((B, T), device=dev), torch.empty((B, T), device=dev)
    v = torch.empty((B,), dtype=torch.int32, device=dev)
    ki = torch.empty((B, T), dtype=torch.int32, device=dev)
    var_p, _keep = h.host4(case.var)
    ws = h.workspace(lib.ssd_decode_nms_cfg_workspace_bytes(B, N, L, cfg))
    h.check(lib.ssd_decode_nms_cfg(h.ptr(dd), h.ptr(pd), h.ptr(pri), var_p, B, N, L, cfg, h.ptr(b), h.ptr(l), h.ptr(s), h.ptr(v),
                                   h.ptr(ki), h.ptr(ws), ws.numel(), h.stream()), "ssd_decode_nms_cfg")
    for x, y in ((b, wb), (l, wl), (s, wsc), (v, dec.last_valid_detections), (ki, dec.last_kept_indices)):
        np.testing.assert_array_equal(_np(x), _np(y))


# ------------------------------------------------------------------------------------------------ the net's predict path
CONFIGS = (("default", {}), ("gaussian", {"nms_method": "gaussian", "score_threshold": 0.3}),
           ("agnostic", {"class_agnostic": True, "max_total_size": 50}), ("linear", {"nms_method": "linear", "iou_threshold": 0.3}))


@pytest.fixture(scope="module")
def net_setup():
    from models.ssd_mobilenet_v2 import get_model
    from utils import bbox_utils
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    x = helpers.images(2, 300, seed=5)

    def fresh():
        m = get_model(hp, max_batch=2)
        m.set_weights(w)
        return m
    return hp, priors, x, fresh


def _predict(m, dec, x):
    return [_np(t) for t in m.predict_on_device(x, dec.prior_boxes, dec.variances, **dec.predict_kwargs())]


def test_net_predict_with_a_config(net_setup):
    from models.decoder import SSDDecoder, get_decoder_model
    hp, priors, x, fresh = net_setup
    decs = {k: SSDDecoder(priors, hp["variances"], **kw) for k, kw in CONFIGS}
    m = fresh()
    deltas, probs = m(x)
    # every config on a fresh net == SSDDecoder.call on the forward's outputs (the fused softmax leaves the same bits)
    want = {}
    for k, dec in decs.items():
        want[k] = _predict(fresh() if k != "default" else m, dec, x)
        b, l, s = dec([deltas, probs])
        for got, ref in zip(want[k], (b, l, s, dec.last_valid_detections)):
            np.testing.assert_array_equal(got, _np(ref), err_msg=k)
        assert want[k][3].min() > 0, k
    assert not np.array_equal(want["gaussian"][2], want["default"][2])
    # one net, the configs alternating (the counters every call leaves, the re-carve at another max_total, the graph key);
    # then the same on graphs over the one-stream step: every config twice, so that each replays its own graph
    order = ("default", "gaussian", "agnostic", "default", "linear", "agnostic", "gaussian", "default")
    for options in ((), (("overlap_heads", 0), ("use_graph", 1))):
        for name, value in options:
            m.set_option(name, value)
        for k in order:
            for got, ref in zip(_predict(m, decs[k], x), want[k]):
                np.testing.assert_array_equal(got, ref, err_msg="%s after %s" % (k, options))
    # two lanes give the one-lane answer
    one = get_decoder_model(fresh(), priors, hp, lanes=1, nms_method="gaussian", score_threshold=0.3)
    two = get_decoder_model(fresh(), priors, hp, lanes=2, nms_method="gaussian", score_threshold=0.3)
    batches = [helpers.images(2, 300, seed=60 + i) for i in range(4)]
    ref = [tuple(_np(t) for t in one(b)) for b in batches]
    outs = [two.submit(b) for b in batches]
    two.wait()
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        for a, b in zip(o, r):
            np.testing.assert_array_equal(_np(a), b)
