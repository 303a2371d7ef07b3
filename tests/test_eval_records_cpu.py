"""N2: ``utils.eval_utils.stats_from_records`` -- the host half of the device scoring path -- against
``oracle.eval_oracle.update_stats``.  The records are read off the oracle itself (tests/eval_cases.py), in the layout
``ssd_eval_match`` writes them; no device is involved."""
import copy

import numpy as np
import pytest

import eval_cases as ec
from oracle import eval_oracle as eo

B, T, G, L = 12, 40, 8, 6


def _eu():
    from utils import eval_utils
    return eval_utils


@pytest.fixture(scope="module")
def batch():
    pb, pl, ps, gt, gl = ec.detections(B, T, G, L)          # the generator of test_eval_update_stats_vs_oracle
    rec = ec.oracle_records(pb, pl, ps, gt, gl)
    ref = eo.update_stats(pb, pl, ps, gt, gl, eo.init_stats(ec.labels_for(L)))
    return (pb, pl, ps, gt, gl), rec, ref


def test_generator_is_the_existing_one():
    """Same draws as tests/test_bbox_gpu.py::test_eval_update_stats_vs_oracle: its asserted property holds here too."""
    pb, pl, ps, gt, gl = ec.detections(B, T, G, L)
    ref = eo.update_stats(pb, pl, ps, gt, gl, eo.init_stats(ec.labels_for(L)))
    assert sum(sum(r["tp"]) for r in ref.values()) > 20 and sum(sum(r["fp"]) for r in ref.values()) > 20
    _, m = eo.calculate_mAP(ref)
    assert 0.05 < float(m) < 1.0


def test_stats_from_records_equal_the_oracle(batch):
    (pb, pl, ps, gt, gl), (rc, rs, rt, rd, rn), ref = batch
    eu = _eu()
    ec.assert_not_vacuous(pb, pl, gt, gl, rt, rd, rn, 20, 20)
    got = eu.stats_from_records(rc, rs, rt, rn, gl, eu.init_stats(ec.labels_for(L)))
    ec.assert_stats_equal(got, ref)
    got, gm = eu.calculate_mAP(got)
    ref, rm = eo.calculate_mAP(copy.deepcopy(ref))
    assert float(gm) == float(rm)
    for cid in ref:
        assert got[cid]["AP"] == ref[cid]["AP"]


def test_rows_after_the_count_are_ignored(batch):
    (pb, pl, ps, gt, gl), (rc, rs, rt, rd, rn), ref = batch
    eu = _eu()
    live = np.arange(T)[None] < rn[:, None]
    junk_c = np.where(live, rc, 77).astype(np.int32)        # class 77 does not exist: it must never be looked up
    junk_t = np.where(live, rt, 1).astype(np.int32)
    got = eu.stats_from_records(junk_c, rs, junk_t, rn, gl, eu.init_stats(ec.labels_for(L)))
    ec.assert_stats_equal(got, ref)


def test_two_halves_equal_one_call(batch):
    (pb, pl, ps, gt, gl), (rc, rs, rt, rd, rn), ref = batch
    eu = _eu()
    h = B // 2
    got = eu.init_stats(ec.labels_for(L))
    eu.stats_from_records(rc[:h], rs[:h], rt[:h], rn[:h], gl[:h], got)
    eu.stats_from_records(rc[h:], rs[h:], rt[h:], rn[h:], gl[h:], got)
    ec.assert_stats_equal(got, ref)
    # ground truth as a list of arrays of different widths (padded batches differ in G)
    wide = np.concatenate([gl[h:], -np.ones((B - h, 3), np.int32)], 1)
    one = eu.stats_from_records(rc, rs, rt, rn, [gl[:h], wide], eu.init_stats(ec.labels_for(L)))
    ec.assert_stats_equal(one, ref)
    assert float(eu.calculate_mAP(got)[1]) == float(eu.calculate_mAP(one)[1]) == float(eo.calculate_mAP(copy.deepcopy(ref))[1])


def test_unknown_class_raises_keyerror(batch):
    (pb, pl, ps, gt, gl), (rc, rs, rt, rd, rn), ref = batch
    eu = _eu()
    assert rn[0] > 0
    bad = rc.copy()
    bad[0, 0] = L + 3
    stats = eu.init_stats(ec.labels_for(L))
    with pytest.raises(KeyError):
        eu.stats_from_records(bad, rs, rt, rn, gl, stats)
    assert all(r["total"] == 0 and r["tp"] == [] for r in stats.values())      # nothing appended
    with pytest.raises(KeyError):                                               # ... a ground-truth class too
        eu.stats_from_records(rc, rs, rt, rn, np.where(gl == gl.max(), L + 1, gl), eu.init_stats(ec.labels_for(L)))
    with pytest.raises(KeyError):                                               # ... as the host path does (class 0)
        eu.stats_from_records(np.zeros_like(rc), rs, rt, rn, gl, eu.init_stats(ec.labels_for(L)))


def test_edge_case_inputs_on_the_oracle():
    """The constructed cases the GPU test relies on, re-checked on the CPU: where they sit and what the oracle makes
    of them (4 x 200 x 16 x 21 gave 54 TPs / 620 FPs when this was written)."""
    for shape, min_tp, min_fp in (((12, 40, 8, 6), 20, 20), ((64, 200, 16, 21), 20, 20), ((8, 40, 1, 6), 3, 20),
                                  ((8, 1, 8, 6), 1, 1)):
        pb, pl, ps, gt, gl, where = ec.case(*shape)
        rc, rs, rt, rd, rn = ec.oracle_records(pb, pl, ps, gt, gl)
        Tn = shape[1]
        ec.assert_not_vacuous(pb, pl, gt, gl, rt, rd, rn, min_tp, min_fp, want_tie=Tn > 1, want_taken=Tn > 1)
        iou, best, arg = ec.best_and_arg(pb, gt)

        def record_of(b, t):
            k = np.nonzero(rd[b, :rn[b]] == t)[0]
            assert len(k) == 1
            return int(k[0])
        b, t = where["half"]
        assert best[b, t] == np.float32(0.5) and rt[b, record_of(b, t)] == 1 and record_of(b, t) == 0
        if "half_taken" in where:
            b, t = where["half_taken"]
            assert best[b, t] == np.float32(0.5) and rt[b, record_of(b, t)] == 0 and record_of(b, t) == 1
        if "duplicate" in where:
            b, t0, t1 = where["duplicate"]
            assert best[b, t0] == best[b, t1] and record_of(b, t1) == record_of(b, t0) + 1
        b, t = where["degenerate_padded"]
        assert np.isnan(iou[b, t]).any() and (gl[b] == -1).any() and rt[b, record_of(b, t)] == 0
        assert rn[3] == 0
        b, t = where["degenerate_all_padding"]
        assert (gl[b] == -1).all() and best[b, t] == -np.inf and record_of(b, t) == rn[b] - 1 and rt[b].sum() == 0
