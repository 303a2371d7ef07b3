"""The loss kernel (csrc/ssd_loss.hip) at the edges of its decisions, against oracle/loss_oracle.py: hard-negative mining
when the K-th loss sits inside a group of bit-identical losses (the ordered ballot/popcount count over lanes, waves and
1024-anchor chunks decides), the `all`, `none` and T = 0 paths, the clip edges of the gradient, unnormalised
probabilities, the localisation term's edges, output hygiene through the C ABI, and one whole training step whose label
head is zero, so that every anchor of the batch ties.  The cases are tests/loss_cases.py (shown not to be vacuous, and to
catch three wrong tie rules, in tests/test_loss_cases_cpu.py).

Bars, all from tests/test_loss.py: final_mask bit-exact given the device's own per-anchor losses; per-anchor CE within
2e-6 * max(1, max CE); loss values within 1e-5 relative; gradients within 1e-6 absolute of torch autograd evaluated with
the device's mask; plus bit equalities (a level is one bit pattern, unselected rows are exactly zero, mask-2 rows are
exactly twice the rows the same anchor gets with mask 1).

Measured on an MI355X (gfx950), worst over the batch; "tie-break" = anchors equal to T taken / in the group:
  batch (images x anchors)      |ce - oracle| (bound)     |grad_logits| / |grad_deltas| - autograd   tie-break per image
  ratio3       (6 x 2500)       9.5e-07 (2.2e-05)         9.3e-09 / 1.9e-09       67/900, 60/64, 120/2460, 15/15, 800/2100, 300/700
  all          (1 x 2500)       2.4e-07 (8.0e-06)         1.5e-08 / 4.7e-09       -
  none         (1 x 2500)       4.8e-07 (8.3e-06)         6.0e-08 / 3.0e-08       -
  cuts         (5 x 2500)       9.5e-07 (2.5e-05)         3.0e-08 / 2.3e-10       1/2499, 64/2436, 65/2435, 1024/1476, 1025/1475
  nine_chunks  (2 x 8732)       9.5e-07 (2.3e-05)         1.2e-09 / 4.7e-10       199/4000, 3998/4200
  partial_wave (2 x 50)         4.8e-07 (1.1e-05)         7.5e-09 / 7.5e-09       7/20, 18/44
  fp32_product (1 x 2500)       9.5e-07 (2.1e-05)         5.6e-09 / 3.5e-09       29/2475 (the double product would give 28)
  clip_edges   (1 x 300)        1.9e-06 (3.2e-05)         inside 1e-6
  localisation edges (5 x 130)  -                         1.5e-08 / 5.6e-09
  training step, zero label head (2 x 2268): probabilities one bit pattern, 1.5e-09 / 9.3e-10
(the gradient bound is 1e-6 absolute throughout; the largest gradient entry of a batch lies between 5e-3 and 0.5).
"""
import numpy as np
import pytest

import helpers
import loss_cases as lc
from oracle import loss_oracle as lo

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(batch):
    """One batch through CustomLoss.conf_loss_fn and loss_and_grads, and the autograd oracle with the device's mask:
    computed once, shared by the tests, left unchanged."""
    if batch.name not in _RUNS:
        from ssd_loss import CustomLoss
        cl = CustomLoss(batch.ratio, 1.0)
        conf = cl.conf_loss_fn(batch.yl, batch.pp).cpu().numpy()
        r = dict(conf=conf, ce=cl.last_cross_entropy.cpu().numpy(), fm=cl.last_final_mask.cpu().numpy())
        loc, conf2, gd, gz = cl.loss_and_grads(batch.yd, batch.yl, batch.pd, batch.pp)
        r.update(loc=loc.cpu().numpy(), conf2=conf2.cpu().numpy(), gd=gd.cpu().numpy(), gz=gz.cpu().numpy())
        r["ref"] = lo.torch_loss_and_grads(batch.yd, batch.yl, batch.pd, batch.z, batch.ratio, 1.0, final_mask=r["fm"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[batch.name] = r
    return _RUNS[batch.name]


def _check_forward(batch, r, pp=None):
    """The forward bars of tests/test_loss.py -> (worst |ce - oracle|, its bound)."""
    pp = batch.pp if pp is None else pp
    rce = lo.cross_entropy(batch.yl, pp)
    ce_err, ce_bound = float(np.abs(r["ce"] - rce).max()), 2e-6 * max(1.0, float(rce.max()))
    print("%s: worst |ce - oracle| %.3e (bound %.3e)" % (batch.name, ce_err, ce_bound))
    rconf, _, rfm = lo.conf_loss_fn(batch.yl, pp, batch.ratio, return_parts=True, ce=r["ce"])
    np.testing.assert_array_equal(r["fm"], rfm)
    assert ce_err <= ce_bound
    np.testing.assert_allclose(r["conf"], rconf, rtol=1e-5, atol=1e-7)
    return rfm


@pytest.mark.parametrize("name", list(lc.batches()))
def test_mining_under_ties_matches_oracle(name):
    batch = lc.batches()[name]
    r = _run(batch)
    for b, case in enumerate(batch.cases):
        for i in range(len(case.palette)):                       # the device's loss within a level is one bit pattern
            assert np.unique(r["ce"][b][case.level == i].view(np.uint32)).size == 1, case
        if (case.level == lc.SATURATED).any():
            assert np.unique(r["ce"][b][case.level == lc.SATURATED].view(np.uint32)).size == 1, case
    rfm = _check_forward(batch, r)
    for b, case in enumerate(batch.cases):
        lc.assert_not_vacuous(case, rfm[b], ce=r["ce"][b])        # ... on the device's losses too: the tie-break decided
        if case.expect:
            print("  %-22s K %4d  tie-break %d / %d" % (case.name, case.K, case.expect["taken"], case.expect["group"]))
    np.testing.assert_array_equal(r["conf2"], r["conf"])          # the same kernel with the localisation term beside it


@pytest.mark.parametrize("name", list(lc.batches()))
def test_gradients_under_ties_match_autograd(name):
    from ssd_loss import CustomLoss
    batch = lc.batches()[name]
    r = _run(batch)
    rloc, rconf, _, rgd, rgz = r["ref"]
    gd_err, gz_err = float(np.abs(r["gd"] - rgd).max()), float(np.abs(r["gz"] - rgz).max())
    print("%s: worst |grad_deltas - autograd| %.3e, |grad_logits - autograd| %.3e (bound 1e-6; largest |g| %.3e)" % (
        batch.name, gd_err, gz_err, float(np.abs(rgz).max())))
    np.testing.assert_allclose(r["loc"], rloc, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r["conf2"], rconf, rtol=1e-5, atol=1e-7)
    assert gd_err <= 1e-6 and gz_err <= 1e-6
    assert np.abs(rgz).max() > 1e-5
    fm = r["fm"]
    assert not r["gz"][fm == 0].any()                              # rows of unselected anchors: exactly zero
    p_true = (batch.pp * batch.yl).sum(-1)                          # (a selected anchor outside the clip range has none)
    inside = (p_true >= np.float32(1e-7)) & (p_true <= np.float32(1) - np.float32(1e-7))
    assert (np.abs(r["gz"][(fm != 0) & inside]).max(-1) > 0).all()
    assert not r["gz"][~inside].any()
    assert not r["gd"][~np.any(batch.yd != 0, -1)].any()
    # mask 2 = twice the gradient, exactly: the same anchors with ratio 0 (mask = positives only)
    _, _, _, gz1 = CustomLoss(0.0, 1.0).loss_and_grads(batch.yd, batch.yl, batch.pd, batch.pp)
    gz1 = gz1.cpu().numpy()
    pos = np.stack([c.pos for c in batch.cases])
    np.testing.assert_array_equal(r["gz"][fm == 2], 2 * gz1[fm == 2])
    np.testing.assert_array_equal(r["gz"][pos & (fm == 1)], gz1[pos & (fm == 1)])
    assert not gz1[~pos].any()
    if name in ("all", "ratio3"):
        assert (fm == 2).any()


def test_gradient_clip_edges():
    """A positive whose true-class probability is below 1e-7 is selected, loses -log(1e-7) and has an all-zero gradient
    row; so has one whose probability saturates above 1 - 1e-7."""
    batch, below, above = lc.clip_edge_batch()
    r = _run(batch)
    _check_forward(batch, r)
    _, _, _, rgd, rgz = r["ref"]
    assert np.abs(r["gz"] - rgz).max() <= 1e-6 and np.abs(r["gd"] - rgd).max() <= 1e-6
    fm, ce, gz = r["fm"][0], r["ce"][0], r["gz"][0]
    assert (fm[below | above] == 1).all()
    assert np.unique(ce[below].view(np.uint32)).size == 1 and np.unique(ce[above].view(np.uint32)).size == 1
    assert ce[below][0] > 16 and ce[above][0] < 2e-7                # -log(1e-7) and -log(1 - 1e-7)
    assert not gz[below | above].any() and not rgz[0][below | above].any()
    others = batch.cases[0].pos & ~below & ~above
    assert (np.abs(gz[others]).max(-1) > 0).all()


def test_unnormalised_probabilities_forward():
    """Rows scaled by 0.5 ... 2 (one factor per level, so the ties stay): the kernel renormalises as Keras does."""
    from ssd_loss import CustomLoss
    batch = lc.batches()["ratio3"]
    rng = np.random.default_rng(3)
    scale = (0.5 + 1.5 * rng.random((batch.B, batch.N))).astype(np.float32)
    for b, case in enumerate(batch.cases):
        for lv in list(range(len(case.palette))) + [lc.SATURATED]:
            scale[b][case.level == lv] = np.float32(0.5 + 1.5 * rng.random())
    pp = batch.pp * scale[..., None]
    assert np.abs(pp.sum(-1) - 1).max() > 0.4
    cl = CustomLoss(batch.ratio, 1.0)
    conf = cl.conf_loss_fn(batch.yl, pp).cpu().numpy()
    r = dict(conf=conf, ce=cl.last_cross_entropy.cpu().numpy(), fm=cl.last_final_mask.cpu().numpy())
    rfm = _check_forward(batch, r, pp)
    np.testing.assert_allclose(conf, lo.conf_loss_fn(batch.yl, pp, batch.ratio), rtol=1e-4, atol=1e-6)
    for b, case in enumerate(batch.cases):
        if case.kind == "cut_inside":                              # still a cut inside a group of one bit pattern
            masked = r["ce"][b] * batch.yl[b, :, 0]
            T = np.sort(masked)[::-1][case.K - 1]
            g = masked == T
            assert 0 < ((rfm[b] - case.pos == 1) & g).sum() < g.sum(), case


def test_localisation_edges():
    from ssd_loss import CustomLoss
    yd, yl, pd, z, pp, notes = lc.localisation_edge_batch()
    cl = CustomLoss(3.0, 1.0)
    loc_only = cl.loc_loss_fn(yd, pd).cpu().numpy()
    loc, conf, gd, gz = (t.cpu().numpy() for t in cl.loss_and_grads(yd, yl, pd, pp))
    cl.conf_loss_fn(yl, pp)
    fm = cl.last_final_mask.cpu().numpy()
    rloc, rconf, _, rgd, rgz = lo.torch_loss_and_grads(yd, yl, pd, z, 3.0, 1.0, final_mask=fm)
    np.testing.assert_array_equal(loc_only, loc)
    np.testing.assert_allclose(loc, lo.loc_loss_fn(yd, pd), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(loc, rloc, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(conf, rconf, rtol=1e-5, atol=1e-7)
    print("localisation edges: worst |grad_deltas - autograd| %.3e, |grad_logits - autograd| %.3e" % (
        np.abs(gd - rgd).max(), np.abs(gz - rgz).max()))
    assert np.abs(gd - rgd).max() <= 1e-6 and np.abs(gz - rgz).max() <= 1e-6
    # errors of exactly 0, +-1, +-3: gradient 0, +-g, +-g with g = 1 / (B * positives)
    b, idx = notes["knee"]
    err = pd[b, idx] - yd[b, idx]
    got = gd[b, idx]
    assert not got[err == 0].any()
    g = got[err == 1][0]                                             # one bit pattern on and beyond the knee, either sign
    assert g > 0 and (got[err >= 1] == g).all() and (got[err <= -1] == -g).all()
    assert (got[err == 0.5] == g * np.float32(0.5)).all() and (got[err == -0.5] == -g * np.float32(0.5)).all()
    # the denormal target is a positive (the reference's `!= 0`); -0.0 is none
    b, n = notes["denormal"]
    pos_loc = np.any(yd != 0, -1)
    assert pos_loc[b].sum() == 2
    assert np.abs(gd[b, n]).max() > 0, "a target of 1e-40 was not counted as a positive"
    assert np.abs(rgd[b, n]).max() > 0
    b0, n0 = notes["negative_zero"]
    assert not gd[b0, n0].any()
    assert not gd[~pos_loc].any()
    # label positives with all-zero deltas: pos_loc = 0 (divide by 1), pos_conf = 3
    b = notes["zero_delta_positives"]
    assert loc[b] == 0 and not gd[b].any() and conf[b] > 0 and fm[b].sum() == 3 + 9 and np.abs(gz[b]).max() > 0
    # no positives at all
    b = notes["empty"]
    assert loc[b] == 0 and conf[b] == 0 and not gd[b].any() and not gz[b].any() and not fm[b].any()


GUARD = 64                        # floats on either side of an output (256 bytes: the ABI's 16-byte alignment holds)
GUARD_BITS = 0x7FC0BEEF           # a NaN too: whoever reads a guard sees it


def _poisoned(shape, dev):
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    bits = buf.view(torch.int32)
    bits[:GUARD] = GUARD_BITS
    bits[GUARD + n:] = GUARD_BITS
    return buf, buf[GUARD:GUARD + n].view(shape)


def _written_and_guarded(buf, view, what):
    import torch
    n = view.numel()
    bits = buf.view(torch.int32)
    assert bool((bits[:GUARD] == GUARD_BITS).all()) and bool((bits[GUARD + n:] == GUARD_BITS).all()), \
        "%s: written outside the tensor" % what
    assert not bool(torch.isnan(view).any()), "%s: not fully written" % what
    return view.cpu().numpy().view(np.uint32)


def test_c_abi_outputs_fully_written_inside_their_bounds():
    """Every output starts NaN-poisoned inside a guarded buffer; the workspace is exactly ssd_loss_workspace_bytes with
    poison behind it; localisation pair alone, confidence pair alone; two calls give the same bits."""
    import torch
    import ssd_hip as h
    batch = lc.batches()["partial_wave"]
    big = lc.batches()["ratio3"]
    lib = h.lib()
    for bt in (batch, big):
        B, N, L = bt.B, bt.N, bt.L
        yd, pd, yl, pl = (h.to_dev(getattr(bt, f)) for f in ("yd", "pd", "yl", "pp"))
        dev = yd.device
        nbytes = lib.ssd_loss_workspace_bytes(B, N)
        assert nbytes >= B * N * 9

        def call(loc_term, conf_term):
            shapes = {}
            if loc_term:
                shapes.update(loc=(B,), gd=(B, N, 4))
            if conf_term:
                shapes.update(conf=(B,), ce=(B, N), mask=(B, N), gz=(B, N, L))
            o = {k: _poisoned(s, dev) for k, s in shapes.items()}
            ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
            p = lambda k: h.ptr(o[k][1]) if k in o else h.ptr(None)
            h.check(lib.ssd_loss(h.ptr(yd if loc_term else None), h.ptr(pd if loc_term else None),
                                 h.ptr(yl if conf_term else None), h.ptr(pl if conf_term else None), B, N,
                                 L if conf_term else 1, bt.ratio, 1.0, p("loc"), p("conf"), p("ce"), p("mask"), p("gd"), p("gz"),
                                 1.0 / B, h.ptr(ws), nbytes, h.stream()), "ssd_loss")
            torch.cuda.synchronize()
            assert bool((ws[nbytes:] == 0xA5).all()), "written behind the workspace"
            return {k: _written_and_guarded(buf, view, k) for k, (buf, view) in o.items()}

        full, again = call(True, True), call(True, True)
        assert set(full) == {"loc", "gd", "conf", "ce", "mask", "gz"}
        for k in full:
            np.testing.assert_array_equal(full[k], again[k], err_msg=k)        # same inputs, same bits
        loc_only, conf_only = call(True, False), call(False, True)
        assert set(loc_only) == {"loc", "gd"} and set(conf_only) == {"conf", "ce", "mask", "gz"}
        for part in (loc_only, conf_only):
            for k in part:
                np.testing.assert_array_equal(part[k], full[k], err_msg=k)
        r = _run(bt)
        np.testing.assert_array_equal(full["mask"].view(np.float32), r["fm"])
        np.testing.assert_array_equal(full["gz"].view(np.float32), r["gz"])
    # a workspace one byte short is refused before anything is launched
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loc = torch.empty(B, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        h.check(lib.ssd_loss(h.ptr(yd), h.ptr(pd), None, None, B, N, 1, 3.0, 1.0, h.ptr(loc), None, None, None, None, None,
                             1.0, h.ptr(ws), nbytes - 1, h.stream()), "ssd_loss")


def test_training_step_under_total_ties():
    """MobileNetV2, B = 2, every *_conv_label_output kernel and bias zero: every anchor's probabilities are the one row
    1 / L, every background loss ties, and the step must learn from the positives plus, per image, the FIRST K background
    anchors by index."""
    from models.ssd_mobilenet_v2 import get_model
    from oracle import bbox_oracle as bo
    from ssd_loss import CustomLoss
    hp = helpers.hyper_params("mobilenet_v2")
    L = hp["total_labels"]
    w = {k: v.copy() for k, v in helpers.synthetic_weights("mobilenet_v2", hp).items()}
    for i in range(1, 7):
        w["%d_conv_label_output/kernel" % i][...] = 0
        w["%d_conv_label_output/bias" % i][...] = 0
    B = 2
    x = helpers.images(B, 300, seed=21)
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=L, seed=3)
    yd, yl = bo.calculate_actual_outputs(priors, gt, gl, hp)
    m = get_model(hp)
    m.set_weights(w)
    cl = CustomLoss(hp["neg_pos_ratio"], hp["loc_loss_alpha"])
    m.compile(loss=[cl.loc_loss_fn, cl.conf_loss_fn])
    loc, conf, _ = m.forward_backward(x, yd, yl)
    probs = m.train_fetch("probs", B).reshape(B, -1, L)
    deltas = m.train_fetch("deltas", B).reshape(B, -1, 4)
    gz = m.train_fetch("grad_logits", B).reshape(B, -1, L)
    gd = m.train_fetch("grad_deltas", B).reshape(B, -1, 4)
    N = probs.shape[1]
    assert np.unique(probs.view(np.uint32)).size == 1 and abs(float(probs.flat[0]) - 1.0 / L) < 1e-7
    pos = (yl[..., 1:] != 0).any(-1)
    want = pos.astype(np.float32)
    for b in range(B):
        K = lc.total_neg(int(pos[b].sum()), hp["neg_pos_ratio"])
        assert 0 < K < (~pos[b]).sum()
        want[b, np.nonzero(~pos[b])[0][:K]] += 1
    np.testing.assert_array_equal(np.abs(gz).max(-1) > 0, want > 0)
    # ... which is what the oracle selects on the device's probabilities
    np.testing.assert_array_equal(lo.conf_loss_fn(yl, probs, hp["neg_pos_ratio"], return_parts=True)[2], want)
    rloc, rconf, rprobs, rgd, rgz = lo.torch_loss_and_grads(yd, yl, deltas, np.zeros((B, N, L), np.float32),
                                                            hp["neg_pos_ratio"], hp["loc_loss_alpha"], final_mask=want)
    assert np.abs(rprobs - probs).max() <= 1e-7
    print("total ties: worst |grad_logits - oracle| %.3e, |grad_deltas - oracle| %.3e" % (
        np.abs(gz - rgz).max(), np.abs(gd - rgd).max()))
    assert np.abs(gz - rgz).max() <= 1e-6 and np.abs(gd - rgd).max() <= 1e-6
    np.testing.assert_allclose(conf.cpu().numpy(), rconf, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(loc.cpu().numpy(), rloc, rtol=1e-5, atol=1e-7)
