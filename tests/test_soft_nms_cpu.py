"""Soft-NMS / class-agnostic suppression: what holds without a GPU -- the oracle against the hard-NMS oracle, against TF's
lazy priority-queue formulation and against known answers, the cases' own promises, and the Python surface."""
import ctypes

import numpy as np
import pytest

import soft_nms_cases as sc
from oracle import bbox_oracle as bo


@pytest.mark.parametrize("name", sc.names())
def test_cases_keep_away_from_near_ties(name):
    case = sc.by_name(name)
    fig = sc.restatement_figures(case)
    print("%s (seed %s): %s" % (name, case.seed, fig))
    assert fig["order_agrees"], "the float32 restatement selects other rows than the oracle"
    if case.method != "hard":
        assert fig["tie_gap"] >= 16.0 * fig["deviation"]
    assert sc.oracle(case).valid.sum() > 0
    if not name.startswith(("planted", "edge")):
        assert sc.score_bar(case) <= 1e-5               # the bars stay what fp32 costs: a few 1e-7 .. 1e-6


def test_the_shapes_reach_the_paths_they_are_meant_for():
    per_list = lambda c: (sc.candidate_inputs(c, np.float64)[1] > np.float32(c.score_threshold)).sum(1).max()
    assert per_list(sc.by_name("wide_gaussian")) == 700 > 2 * 256
    assert per_list(sc.by_name("hbm_linear")) == sc.LDS_CANDIDATES + 37
    assert per_list(sc.by_name("hbm_linear_below")) == sc.LDS_CANDIDATES - 1
    assert per_list(sc.by_name("decoder_gaussian_001")) > 256
    raw1 = sc.by_name("raw_gaussian_1")                 # nothing pruned, the limit truncates
    assert per_list(raw1) == 500 and sc.oracle(raw1).valid.tolist() == [40, 40, 40]
    hole = sc.by_name("edge_hole_gaussian")
    assert not (hole.scores[:, :, 1] > 0.2).any() and hole.max_per_class > hole.scores.shape[1]


def test_class_agnostic_differs_from_per_class_on_its_case():
    for m in sc.METHODS:
        case = sc.by_name("agnostic_%s" % m)
        per_class = sc.run(case._replace(agnostic=False))
        pooled = sc.oracle(case)
        assert not (np.array_equal(per_class.idx, pooled.idx) and np.array_equal(per_class.classes, pooled.classes))
        # one anchor, one class: an anchor comes out at most once under hard suppression (IoU with itself is 1)
        if m == "hard":
            for b in range(pooled.idx.shape[0]):
                kept = pooled.idx[b, :pooled.valid[b]]
                assert len(set(kept.tolist())) == kept.size


def test_hard_per_class_is_the_combined_nms_oracle():
    """The inputs of tests/test_bbox_gpu.py::test_combined_nms_raw."""
    rng = np.random.default_rng(51)
    B, N, C = 3, 500, 5
    c = rng.uniform(0.0, 1.0, (B, N, 2)); sz = rng.uniform(-0.1, 0.4, (B, N, 2))
    boxes = np.concatenate([c - sz / 2, c + sz / 2], -1).astype(np.float32)
    boxes[:, ::17, 2:] = boxes[:, ::17, :2]
    scores = rng.uniform(0, 1, (B, N, C)).astype(np.float32)
    for thr, mpc, mt in ((0.5, 200, 200), (-1.0, 30, 40), (0.9, 5, 200)):
        case = sc.make_case("hard", "raw", "hard", boxes=boxes, scores=scores, score_threshold=thr, max_per_class=mpc, max_total=mt)
        got = sc.run(case)
        rb, rs, rc, rv, ri = bo.combined_non_max_suppression(boxes, scores, mpc, mt, 0.5, thr, return_indices=True)
        np.testing.assert_array_equal(got.valid, rv)
        np.testing.assert_array_equal(got.idx, ri)
        np.testing.assert_array_equal(got.classes, rc.astype(np.int64))
        np.testing.assert_array_equal(got.scores.astype(np.float32), rs)
        np.testing.assert_array_equal(got.boxes.astype(np.float32), rb)


@pytest.mark.parametrize("name", ["raw_gaussian_0", "raw_gaussian_2", "wide_gaussian", "agnostic_gaussian"])
def test_eager_selection_is_tfs_lazy_priority_queue(name):
    case = sc.by_name(name)
    boxes, scores = sc.candidate_inputs(case, np.float64)
    thr32 = np.float32(case.score_threshold)
    scale = sc.scale_of(case.sigma)
    worst = 0.0
    for b in range(scores.shape[0]):
        lists = []
        if case.agnostic:
            a, c = np.nonzero(scores[b] > thr32)
            lists.append((a, c, min(case.max_per_class, case.max_total, a.size)))
        else:
            for c in range(scores.shape[2]):
                a = np.nonzero(scores[b, :, c] > thr32)[0]
                lists.append((a, np.full(a.shape, c), min(case.max_per_class, scores.shape[1])))
        for a, c, limit in lists:
            if not a.size:
                continue
            args = (boxes[b], a, c, scores[b][a, c], float(np.float32(case.iou_threshold)), float(thr32), scale, limit)
            eager = sc.select_list(args[0], a, c, args[3], "gaussian", *args[4:])
            lazy = sc.lazy_gaussian_list(*args)
            assert [(e[0], e[1]) for e in eager] == [(l[0], l[1]) for l in lazy]
            worst = max([worst] + [abs(e[2] - l[2]) / e[2] for e, l in zip(eager, lazy)])
    print("%s: eager against lazy, worst relative score difference %.3g" % (name, worst))
    assert worst <= 1e-14           # the same products in the same order; float64 leaves ~1e-16 per step


def test_known_answer_on_the_oracle():
    for method, iou_thr, sigma, want in sc.known_answers():
        case = sc.make_case("known", "raw", method, boxes=sc.KNOWN_BOXES, scores=sc.KNOWN_SCORES, iou_threshold=iou_thr,
                            score_threshold=0.1, sigma=sigma, max_per_class=3, max_total=3, clip=False)
        for dtype, tol in ((np.float64, 1e-7), (np.float32, 5e-7)):     # 0.9 / 0.8 / 0.7 are their fp32 roundings
            got = sc.run(case, dtype)
            assert got.valid.tolist() == [len(want)]
            assert got.idx[0, :len(want)].tolist() == [a for a, _ in want]
            np.testing.assert_allclose(got.scores[0, :len(want)], [s for _, s in want], rtol=tol)


def test_arguments_are_validated():
    from models.decoder import SSDDecoder, get_decoder_model
    from utils import bbox_utils
    priors = np.zeros((4, 4), np.float32)
    var = [0.1, 0.1, 0.2, 0.2]
    bad = [dict(nms_method="soft"), dict(nms_method=None), dict(nms_method="gaussian", soft_nms_sigma=0.0),
           dict(nms_method="gaussian", soft_nms_sigma=-1.0), dict(nms_method="gaussian", soft_nms_sigma=float("nan")),
           dict(nms_method="gaussian", soft_nms_sigma=float("inf")), dict(iou_threshold=1.5), dict(iou_threshold=-0.1),
           dict(iou_threshold=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            SSDDecoder(priors, var, **kw)
        if kw.get("nms_method", "x") is not None:
            with pytest.raises(ValueError):
                get_decoder_model(object(), priors, {"variances": var}, lanes=1, **kw)
        with pytest.raises(ValueError):
            bbox_utils.non_max_suppression(np.zeros((1, 4, 1, 4), np.float32), np.zeros((1, 4, 2), np.float32),
                                           max_output_size_per_class=2, max_total_size=2, **kw)
    SSDDecoder(priors, var, nms_method="linear", soft_nms_sigma=float("nan"))       # sigma belongs to "gaussian" alone
    SSDDecoder(priors, var, nms_method="hard", iou_threshold=0.0, class_agnostic=True)
    d = get_decoder_model(object(), priors, {"variances": var}, lanes=1, nms_method="linear", iou_threshold=0.3,
                          class_agnostic=True, soft_nms_sigma=0.25).decoder
    assert (d.nms_method, d.iou_threshold, d.class_agnostic, d.soft_nms_sigma) == ("linear", 0.3, True, 0.25)


def test_get_config_round_trip():
    from models.decoder import SSDDecoder
    priors = np.arange(8, dtype=np.float32).reshape(2, 4)
    d = SSDDecoder(priors, [0.1, 0.1, 0.2, 0.2], max_total_size=50, score_threshold=0.01, iou_threshold=0.45,
                   nms_method="gaussian", soft_nms_sigma=0.3, class_agnostic=True, name="dec")
    cfg = d.get_config()
    assert {"iou_threshold", "nms_method", "soft_nms_sigma", "class_agnostic"} <= set(cfg)
    again = SSDDecoder(**cfg).get_config()
    assert np.array_equal(again.pop("prior_boxes"), cfg.pop("prior_boxes")) and again == cfg
    plain = SSDDecoder(priors, [0.1, 0.1, 0.2, 0.2])
    assert plain.nms_config() is None and "nms_config" not in plain.predict_kwargs()        # the reference's path, as ever
    c = d.nms_config()
    assert (c.method, c.class_agnostic, c.max_per_class, c.max_total) == (1, 1, 50, 50)
    assert (c.iou_threshold, c.score_threshold, c.sigma) == tuple(float(np.float32(v)) for v in (0.45, 0.01, 0.3))


def test_nms_config_mirrors_the_struct():
    import ssd_hip
    lib = ssd_hip.lib()
    assert ctypes.sizeof(ssd_hip.NmsConfig) == lib.ssd_nms_config_bytes() == 32
    assert (ssd_hip.NMS_HARD, ssd_hip.NMS_GAUSSIAN, ssd_hip.NMS_LINEAR) == (0, 1, 2)
    assert 256 < lib.ssd_nms_lds_candidates() and lib.ssd_nms_lds_candidates() * 24 <= 160 * 1024
    cfg = ssd_hip.nms_config("linear", True, 7, 9, 0.25, 0.125, 0.5, False)
    assert lib.ssd_decode_nms_cfg_workspace_bytes(2, 100, 5, cfg) == lib.ssd_decode_nms_workspace_bytes(2, 100, 5, 7)


def test_the_library_rejects_what_the_header_says():
    """SSD_E_INVALID -> ValueError before anything is launched (no device is touched: B = 0 pointers are never read)."""
    import ssd_hip
    lib = ssd_hip.lib()
    z = ssd_hip.vp(0)

    def call(cfg):
        ssd_hip.check(lib.ssd_combined_nms_cfg(z, z, 0, 10, 3, cfg, z, z, z, z, z, z, 0, z), "ssd_combined_nms_cfg")

    call(ssd_hip.NmsConfig(0, 0, 5, 5, 1, 0.5, 0.5, 0.5))
    for cfg in (ssd_hip.NmsConfig(3, 0, 5, 5, 1, 0.5, 0.5, 0.5), ssd_hip.NmsConfig(-1, 0, 5, 5, 1, 0.5, 0.5, 0.5),
                ssd_hip.NmsConfig(1, 0, 5, 5, 1, 0.5, 0.5, 0.0), ssd_hip.NmsConfig(1, 0, 5, 5, 1, 0.5, 0.5, float("nan")),
                ssd_hip.NmsConfig(1, 0, 5, 5, 1, 0.5, 0.5, float("inf")), ssd_hip.NmsConfig(2, 1, 5, 5, 1, 1.5, 0.5, 0.5),
                ssd_hip.NmsConfig(2, 1, 5, 5, 1, float("nan"), 0.5, 0.5), ssd_hip.NmsConfig(2, 1, 0, 5, 1, 0.5, 0.5, 0.5),
                ssd_hip.NmsConfig(1, 1, 5, 0, 1, 0.5, 0.5, 0.5)):
        with pytest.raises(ValueError):
            call(cfg)


def test_predictor_knobs_exist():
    """Read, not imported: importing predictor.py chooses the process's serving setup."""
    import ast
    import os
    import ssd_hip
    src = open(os.path.join(os.path.dirname(os.path.abspath(ssd_hip.__file__)), "predictor.py")).read()
    assigned = {t.id for n in ast.parse(src).body if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)}
    assert {"nms_method", "nms_sigma", "nms_iou_threshold", "nms_class_agnostic"} <= assigned
    for k in ("nms_method", "nms_sigma", "nms_iou_threshold", "nms_class_agnostic"):
        assert 'knobs.get("%s", %s)' % (k, k) in src
