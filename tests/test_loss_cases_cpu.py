"""The hard-negative mining cases of tests/loss_cases.py, on the CPU alone: every case does what it says on the oracle
(``assert_not_vacuous``), three wrong tie rules each change the mask of every tie case (so the bit equality
tests/test_loss_edges_gpu.py asks of the device would notice them), and the NumPy restatement of the kernel's own
algorithm -- radix select, then the ordered count over chunks, waves and lanes -- equals
``oracle.loss_oracle.hard_negative_mask`` on all cases and on 300 random images whose losses take 8 distinct values.
If the GPU test fails while this file passes, the algorithm is right and its implementation is not."""
import numpy as np
import pytest

import loss_cases as lc
from oracle import loss_oracle as lo


def _oracle_neg(masked, K):
    return lo.hard_negative_mask(masked[None], np.ones((1, masked.size), np.float32), [K])[0]


def _masked(case):
    return (case.ce_cpu * case.yl[:, 0]).astype(np.float32)


@pytest.mark.parametrize("name", list(lc.batches()))
def test_cases_are_not_vacuous(name):
    batch = lc.batches()[name]
    masks = batch.oracle_masks()
    for case, mask in zip(batch.cases, masks):
        lc.assert_not_vacuous(case, mask)
        assert case.purpose
        # images do not depend on their batch
        alone = lo.conf_loss_fn(case.yl[None], case.pp[None], case.ratio, return_parts=True)[2][0]
        np.testing.assert_array_equal(alone, mask)


def test_case_list_is_what_the_suite_relies_on():
    cases = {c.name: c for c in lc.all_cases()}
    assert len(cases) == len(lc.all_cases())
    ks = {c.K for c in cases.values() if c.name.startswith("ties_K")}
    assert ks == {1, 64, 65, 1024, 1025}                       # on and just past a wave and a chunk boundary
    assert {c.N for c in cases.values()} >= {50, 2500, 8732}
    assert cases["all"].K >= cases["all"].N and cases["none"].K == 0 and cases["none"].P == 2
    assert cases["saturated_floor"].ce_cpu[cases["saturated_floor"].level == lc.SATURATED].max() == lc.SATURATED_LOSS
    tie = [c for c in cases.values() if c.tie]
    assert len(tie) >= 14 and all(c.kind in ("cut_inside", "zero") for c in tie)
    # a level is one bit pattern, and the levels are far apart
    for c in cases.values():
        for i in range(len(c.palette)):
            assert np.unique(c.ce_cpu[c.level == i].view(np.uint32)).size == 1, c
    w = cases["wide_group"]
    assert w.ce_cpu[w.level == 0][0] - w.ce_cpu[w.level == 1][0] > 1.0


def test_fp32_product_pair():
    """(P, ratio) whose fp32 product truncates to another integer than the double product; the search finds one far
    below P = 2000."""
    P, ratio, k32, k64 = lc.find_fp32_truncation_pair()
    assert P < 2000 and ratio != int(ratio)
    assert k32 == int(np.float32(P) * np.float32(ratio)) and k64 == int(P * ratio) and k32 != k64
    c = lc.batches()["fp32_product"].cases[0]
    assert (c.P, c.ratio, c.K) == (P, ratio, k32)


@pytest.mark.parametrize("rule", lc.TIE_RULES_WRONG)
def test_wrong_tie_rules_change_every_tie_case(rule):
    seen = 0
    for case in lc.all_cases():
        masked = _masked(case)
        right = _oracle_neg(masked, case.K)
        wrong = lc.radix_select_restatement(masked, case.K, rule)
        if case.tie:
            seen += 1
            assert not np.array_equal(wrong, right), (case, rule)
        if rule == "gt" and case.kind == "cut_at_end":
            assert not np.array_equal(wrong, right), (case, rule)
    assert seen >= 14


def test_dropping_the_carry_across_chunks_changes_every_multi_chunk_tie_case():
    seen = 0
    for case in lc.all_cases():
        if case.tie and len(case.expect["chunks"]) > 1:
            seen += 1
            masked = _masked(case)
            assert not np.array_equal(lc.radix_select_restatement(masked, case.K, "no_running"),
                                      _oracle_neg(masked, case.K)), case
    assert seen >= 12


def test_restatement_equals_oracle_on_all_cases():
    for case in lc.all_cases():
        masked = _masked(case)
        np.testing.assert_array_equal(lc.radix_select_restatement(masked, case.K), _oracle_neg(masked, case.K),
                                      err_msg=case.name)


def test_restatement_equals_oracle_on_quantised_random_images():
    rng = np.random.default_rng(2024)
    tied = 0
    for i in range(300):
        masked, K = lc.quantised_random_image(rng)
        want = _oracle_neg(masked, K)
        np.testing.assert_array_equal(lc.radix_select_restatement(masked, K), want, err_msg="image %d" % i)
        if 0 < K < masked.size:
            T = np.sort(np.where(masked == 0, np.float32(0), masked))[::-1][K - 1]
            g = masked == T
            tied += int(0 < (g & (want == 1)).sum() < g.sum())
    assert tied >= 150                      # most images cut inside a group
    # -0.0 ranks as 0.0, by index
    m = np.array([-0.0, 0.5, 0.0, -0.0, 0.0], np.float32)
    np.testing.assert_array_equal(lc.radix_select_restatement(m, 3), [1, 1, 1, 0, 0])
    np.testing.assert_array_equal(_oracle_neg(m, 3), [1, 1, 1, 0, 0])


def test_gradient_oracle_takes_a_mask():
    """``torch_loss_and_grads(final_mask=...)`` differentiates with the given selection: its own mask reproduces the
    default, another mask moves the gradient rows with it."""
    b = lc.batches()["partial_wave"]
    own = b.oracle_masks(lo.cross_entropy(b.yl, lo.keras_softmax(__import__("torch").from_numpy(b.z)).numpy()))
    base = lo.torch_loss_and_grads(b.yd, b.yl, b.pd, b.z, b.ratio)
    same = lo.torch_loss_and_grads(b.yd, b.yl, b.pd, b.z, b.ratio, final_mask=own)
    for x, y in zip(base, same):
        np.testing.assert_array_equal(x, y)
    other = own[:, ::-1].copy()
    gz = lo.torch_loss_and_grads(b.yd, b.yl, b.pd, b.z, b.ratio, final_mask=other)[4]
    assert not gz[other == 0].any() and (np.abs(gz[other != 0]).max(-1) > 0).all()


def test_edge_batches_are_what_they_say():
    yd, yl, pd, z, pp, notes = lc.localisation_edge_batch()
    pos = np.any(yd != 0, -1)
    b, n = notes["denormal"]
    assert pos[b, n] and np.abs(yd[b, n]).max() < 1.2e-38
    b, n = notes["negative_zero"]
    assert not pos[b, n] and np.signbit(yd[b, n]).all()
    b = notes["zero_delta_positives"]
    assert not pos[b].any() and (yl[b, :, 1:] != 0).any(-1).sum() == 3
    assert not pos[notes["empty"]].any() and not (yl[notes["empty"], :, 1:] != 0).any()
    loc = lo.loc_loss_fn(yd, pd)
    assert loc[2] == 0 and loc[3] == 0 and loc[0] > 0 and loc[1] > 0
    conf = lo.conf_loss_fn(yl, pp)
    assert conf[2] > 0 and conf[3] == 0
    batch, below, above = lc.clip_edge_batch()
    c = batch.cases[0]
    assert below.sum() == 8 and above.sum() == 8 and (c.pos[below | above]).all() and c.P > 16
    np.testing.assert_allclose(c.ce_cpu[below], -np.log(np.float32(1e-7)), rtol=1e-6)
    assert (c.ce_cpu[above] == lc.SATURATED_LOSS).all()
    _, _, _, _, gz = lo.torch_loss_and_grads(batch.yd, batch.yl, batch.pd, batch.z, 3.0)
    assert not gz[0][below | above].any() and (np.abs(gz[0][c.pos & ~below & ~above]).max(-1) > 0).all()
