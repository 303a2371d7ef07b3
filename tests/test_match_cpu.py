"""Target assignment strategies: what holds without a GPU -- the oracle of tests/match_cases.py against the reference's
oracle and against hand-worked answers, the promises of the generated cases, and the Python surface."""
import ctypes

import numpy as np
import pytest

import helpers
import match_cases as mc
from oracle import bbox_oracle as bo

F32 = np.float32


def _case(strategy, priors, gt, gl, **kw):
    return mc.Case("hand/%s/%s/%d" % (strategy, kw.get("topk", 0), len(priors)), None, strategy, np.asarray(priors, F32), np.asarray(gt, F32),
                   np.asarray(gl, np.int32), kw.get("thr", 0.5), kw.get("topk", 0), kw.get("level_start"))


@pytest.mark.parametrize("backbone,seed", [("mobilenet_v2", 3), ("vgg16", 61)])
def test_oracle_under_max_iou_is_the_reference_oracle(backbone, seed):
    p = mc.priors_of(backbone)
    gt, gl = helpers.gt_inputs(3, seed=seed)
    got = mc.oracle(mc.Case("ref/%s" % backbone, seed, "max_iou", p, gt, gl, 0.5, 0, None))
    d, oh, lab, am = bo.calculate_actual_outputs(p, gt, gl, helpers.hyper_params(backbone), return_indices=True)
    np.testing.assert_array_equal(got.label_idx, lab)
    np.testing.assert_array_equal(got.match_idx, am)
    np.testing.assert_array_equal(got.onehot, oh)
    np.testing.assert_array_equal(got.deltas, d)


def test_known_answer_two_boxes_one_best_prior():
    """Priors P0 = [0, 0, .4, .4], P1 = [0, .2, .4, .6], P2 far away.  Box A = P0 (IoU 1 with P0, 1/3 with P1); box B = P0 moved
    right by .05 (IoU .14 / .18 = .78 with P0, .1 / .22 = .45 with P1).  Both prefer P0; A's IoU is the larger, so A takes P0 and
    B its runner-up P1 -- which the threshold rule alone leaves negative (.45 < .5).  P2 overlaps nothing: background, first
    arg-max 0."""
    priors = [[0, 0, .4, .4], [0, .2, .4, .6], [.6, .6, 1, 1]]
    gt = [[[0, 0, .4, .4], [0, .05, .4, .45]]]
    gl = [[7, 9]]
    plain = mc.oracle(_case("max_iou", priors, gt, gl))
    assert plain.label_idx.tolist() == [[7, 0, 0]] and plain.match_idx.tolist() == [[0, 1, 0]]
    forced = mc.oracle(_case("bipartite", priors, gt, gl))
    assert forced.forced == [{0: 0, 1: 1}]
    assert forced.label_idx.tolist() == [[7, 9, 0]] and forced.match_idx.tolist() == [[0, 1, 0]]
    want = bo.get_deltas_from_bboxes(np.asarray(priors, F32), np.asarray([gt[0][0], gt[0][1], [0, 0, 0, 0]], F32)) / np.asarray(helpers.VARIANCES, F32)
    np.testing.assert_array_equal(forced.deltas[0], want.astype(F32))
    assert forced.onehot[0].argmax(-1).tolist() == [7, 9, 0]


def test_known_answer_atss_five_candidates():
    """One level of five priors inside the box [0, 0, 1, 1] (so IoU = the prior's area), top-k 5: IoUs 1, .98, .04, .01, .25.
    mean .456; squared deviations .2959 + .2746 + .1731 + .1989 + .0424 = .9849, / 4 = .2462, root .4962: threshold .952.
    P0 and P1 pass and their centres lie inside; the other three are background with match_idx -1."""
    priors = [[0, 0, 1, 1], [0, 0, 1, .98], [.4, .4, .6, .6], [.1, .1, .2, .2], [.25, .25, .75, .75]]
    res = mc.oracle(_case("atss", priors, [[[0, 0, 1, 1]]], [[5]], topk=5, level_start=[0, 5]))
    assert res.label_idx.tolist() == [[5, 5, 0, 0, 0]]
    assert res.match_idx.tolist() == [[0, 0, -1, -1, -1]]
    # the same priors behind top-k 2: the two nearest centres ((d2, i) order: P0, P2 -- P4 ties with them and has the larger
    # index) have IoUs 1 and .04: mean .52, deviation .6788, threshold 1.199 -- nothing passes
    res = mc.oracle(_case("atss", priors, [[[0, 0, 1, 1]]], [[5]], topk=2, level_start=[0, 5]))
    assert res.label_idx.tolist() == [[0, 0, 0, 0, 0]] and res.match_idx.tolist() == [[-1] * 5]


@pytest.mark.parametrize("name", mc.names("bipartite"))
def test_bipartite_properties(name):
    case, res = mc.by_name(name), mc.oracle(mc.by_name(name))
    for b, forced in enumerate(res.forced):
        boxes = list(forced.values())
        assert len(set(boxes)) == len(boxes), "a box is forced twice"          # priors are distinct: they are dict keys
        assert all(case.gl[b, g] > 0 for g in boxes)
        iou = bo.generate_iou_map(case.priors, case.gt[b:b + 1])[0]
        for g in np.nonzero(case.gl[b] > 0)[0]:
            overlapping = set(np.nonzero(iou[:, g] > 0)[0].tolist())
            if overlapping - set(forced):                                       # some overlapping prior is still free
                assert boxes.count(g) == 1, "box %d has a free overlapping prior and is not forced" % g
        for i, g in forced.items():
            assert res.match_idx[b, i] == g and res.label_idx[b, i] == case.gl[b, g]


def test_cases_reach_what_they_are_meant_for():
    iou = lambda c: bo.generate_iou_map(c.priors, c.gt[0:1])[0]
    c = mc.by_name("shared_best_n300")
    assert c.priors.shape[0] == 300 and c.gl[0].tolist() == [3, -1, 5, -1, 7]
    assert len(set(iou(c)[:, [0, 2, 4]].argmax(0).tolist())) == 1               # three boxes, one best prior
    c = mc.by_name("nested_chain")
    assert len(set(iou(c).argmax(0).tolist())) <= 3 and len(mc.oracle(c).forced[0]) == 8
    c = mc.by_name("identical_boxes")
    f = {g: i for i, g in mc.oracle(c).forced[0].items()}
    assert iou(c)[f[0], 0] > iou(c)[f[1], 1] and f[0] == iou(c)[:, 0].argmax()
    c = mc.by_name("zero_area_box")
    assert not (iou(c)[:, 0] > 0).any() and list(mc.oracle(c).forced[0].values()) == [1]
    c = mc.by_name("three_priors_five_boxes")
    assert (iou(c) > 0).all() and len(mc.oracle(c).forced[0]) == 3
    for name in ("real_mobilenet_v2", "real_vgg16"):
        assert mc.rescued_boxes(mc.by_name(name))
    ls = mc.level_starts("mobilenet_v2")
    assert ls == [0, 1444, 2044, 2194, 2248, 2264, 2268] and mc.level_starts("vgg16")[-1] == 8732
    c = mc.by_name("atss_shared_prior")
    own = mc.oracle(c).positives[0]
    assert set(own.values()) >= {0, 2} and 1 not in own.values()                # the identical pair: every tie to the smaller g
    c = mc.by_name("atss_one_iou")
    assert mc.oracle(c).label_idx.tolist() == [[11] * 4]
    c = mc.by_name("atss_single_candidate")
    assert (mc.oracle(c).label_idx > 0).sum() == 1
    c = mc.by_name("atss_cell_centre")                                           # the four priors of the cell are at distance 0
    pcy, pcx = mc.centres(c.priors)
    gcy, gcx = mc.centres(c.gt[0])
    assert ((pcy == gcy[0]) & (pcx == gcx[0]))[:1444].sum() == 4


def test_match_config_surface():
    import ssd_hip
    assert ctypes.sizeof(ssd_hip.MatchConfig) == 16 + 4 * 9
    cfg = ssd_hip.match_config("atss", topk=9, level_start=[0, 4, 10])
    assert (cfg.strategy, cfg.topk, cfg.n_levels, list(cfg.level_start)[:3]) == (ssd_hip.MATCH_ATSS, 9, 2, [0, 4, 10])
    assert ssd_hip.match_config("bipartite", 0.4).strategy == ssd_hip.MATCH_BIPARTITE
    assert ssd_hip.match_config().strategy == ssd_hip.MATCH_MAX_IOU
    for kw in (dict(strategy="hungarian"), dict(strategy="atss", topk=0, level_start=[0, 4]),
               dict(strategy="atss", topk=65, level_start=[0, 4]), dict(strategy="atss"), dict(strategy="atss", level_start=[0]),
               dict(strategy="atss", level_start=[1, 4]), dict(strategy="atss", level_start=[0, 5, 4]),
               dict(strategy="atss", level_start=list(range(10)))):
        with pytest.raises(ValueError):
            ssd_hip.match_config(**kw)


def test_library_refuses_what_the_builder_refuses():
    """SSD_E_INVALID before anything is launched (no device is touched: with B = 0 no pointer is read)."""
    import ssd_hip
    lib = ssd_hip.lib()
    var_p, _keep = ssd_hip.host4(helpers.VARIANCES)

    def call(cfg, N=10):
        return lib.ssd_match_encode_cfg(None, None, None, var_p, cfg, 0, N, 3, 21, None, None, None, None, None, 0, None)
    good = ssd_hip.match_config("atss", topk=9, level_start=[0, 4, 10])
    assert call(good) == 0 and call(ssd_hip.match_config("bipartite")) == 0 and call(ssd_hip.match_config()) == 0
    assert call(None) == -1 and b"NULL" in lib.ssd_last_error()
    assert call(good, N=11) == -1 and b"level_start" in lib.ssd_last_error()
    for field, value in (("strategy", 3), ("topk", 0), ("topk", 65), ("n_levels", 0), ("n_levels", 9)):
        bad = ssd_hip.match_config("atss", topk=9, level_start=[0, 4, 10])
        setattr(bad, field, value)
        assert call(bad) == -1 and lib.ssd_last_error(), (field, value)
    bad = ssd_hip.match_config("atss", topk=9, level_start=[0, 4, 10])
    bad.level_start[1] = 11
    assert call(bad) == -1
    ws = lib.ssd_match_encode_cfg_workspace_bytes
    assert ws(2, 300, 5, ssd_hip.match_config()) == 0 and ws(2, 300, 5, None) == 0
    assert ws(2, 300, 5, ssd_hip.match_config("bipartite")) == 2 * 300 * 4 + 2 * 5 * 8
    assert ws(2, 300, 5, ssd_hip.match_config("atss", level_start=[0, 300])) == 2 * 300 * 8


def test_hyper_params_gain_no_key_and_levels_are_checked():
    from utils import train_utils
    for backbone in ("mobilenet_v2", "vgg16"):
        hp = train_utils.get_hyper_params(backbone)
        assert not [k for k in hp if k.startswith("match")]
        assert not [k for k in train_utils.SSD[backbone] if k.startswith("match")]
    hp = helpers.hyper_params("mobilenet_v2")
    assert train_utils.match_config_from(hp, 2268) is None                      # absent keys: ssd_match_encode as before
    cfg = train_utils.match_config_from(dict(hp, match_strategy="atss"), 2268)
    assert (cfg.strategy, cfg.topk, cfg.n_levels) == (2, 9, 6) and list(cfg.level_start)[:7] == mc.level_starts("mobilenet_v2")
    assert train_utils.match_config_from(dict(hp, match_strategy="atss", match_topk=4), 2268).topk == 4
    assert train_utils.match_config_from(dict(hp, match_strategy="bipartite"), 17).strategy == 1
    with pytest.raises(ValueError, match="2268"):
        train_utils.match_config_from(dict(hp, match_strategy="atss"), 2264)
    with pytest.raises(ValueError):
        train_utils.match_config_from(dict(hp, match_strategy="nearest"), 2268)
    with pytest.raises(ValueError):
        train_utils.match_config_from(dict(hp, match_strategy="atss", match_topk=0), 2268)


def test_match_from_env(monkeypatch):
    import importlib
    from utils import train_utils
    trainer = importlib.import_module("trainer")
    hp = train_utils.get_hyper_params("mobilenet_v2")
    before = dict(hp)
    for k in ("SSD_TRAINER_MATCH", "SSD_TRAINER_MATCH_TOPK"):
        monkeypatch.delenv(k, raising=False)
    assert trainer.match_from_env(hp) is hp
    monkeypatch.setenv("SSD_TRAINER_MATCH", "max_iou")
    assert trainer.match_from_env(hp) is hp
    monkeypatch.setenv("SSD_TRAINER_MATCH", "Bipartite")
    got = trainer.match_from_env(hp)
    assert got["match_strategy"] == "bipartite" and "match_topk" not in got and got is not hp
    monkeypatch.setenv("SSD_TRAINER_MATCH_TOPK", "5")
    with pytest.raises(ValueError, match="SSD_TRAINER_MATCH_TOPK"):
        trainer.match_from_env(hp)                                              # a top-k beside a strategy that ignores it
    monkeypatch.setenv("SSD_TRAINER_MATCH", "atss")
    got = trainer.match_from_env(hp)
    assert (got["match_strategy"], got["match_topk"]) == ("atss", 5)
    monkeypatch.delenv("SSD_TRAINER_MATCH_TOPK")
    assert trainer.match_from_env(hp)["match_topk"] == 9
    for bad in ("0", "65", "nine", "2.5"):
        monkeypatch.setenv("SSD_TRAINER_MATCH_TOPK", bad)
        with pytest.raises(ValueError, match="SSD_TRAINER_MATCH_TOPK"):
            trainer.match_from_env(hp)
    monkeypatch.delenv("SSD_TRAINER_MATCH_TOPK")
    monkeypatch.setenv("SSD_TRAINER_MATCH", "hungarian")
    with pytest.raises(ValueError, match="SSD_TRAINER_MATCH"):
        trainer.match_from_env(hp)
    monkeypatch.delenv("SSD_TRAINER_MATCH")
    monkeypatch.setenv("SSD_TRAINER_MATCH_TOPK", "9")
    with pytest.raises(ValueError):
        trainer.match_from_env(hp)                                              # ... and beside the default
    assert hp == before, "the module-level table gained or lost a key"
