"""TEST INFRASTRUCTURE ONLY -- images for the loss kernel's hard-negative mining (csrc/ssd_loss.hip phases B and C) built
so that the tie-break at the threshold T has work to do, shared by tests/test_loss_cases_cpu.py (no GPU) and
tests/test_loss_edges_gpu.py.

An image is built from a PALETTE of logit rows, not from random rows: a background anchor of a level gets the row
``(log(p0 / (1 - p0) * (L - 1)), 0, ..., 0)``, so every anchor of a level is bit-identical, its loss is bit-identical on
any implementation, and levels as far apart as p0 = 0.1 and 0.3 cannot change order between libm and the device's logf.
"Saturated" backgrounds are ``(40, 0, ..., 0)``: fp32 softmax gives p0 == 1.0 exactly, the clip maps it to 1 - 1e-7 and
every such anchor to the loss 1.192093e-07.  The remaining backgrounds ("filler") are distinct confident random rows
(standard normal, z0 += 6).  Positives sit at the first P indices of a seeded permutation and the levels at the following
ones, so tied anchors are scattered over all 1024-anchor chunks of the kernel's ordered prefix count.

Every case states what it is for (``kind``, ``expect``); ``assert_not_vacuous`` checks that statement on the ORACLE's
mask -- a condition on the inputs, not on the kernel.  The expected figures were worked out once on the CPU with
oracle/loss_oracle.py and are written down in ``_build_cases`` so that a change of the construction cannot quietly turn
a "cut inside the group" into something easier.

``radix_select_restatement`` is the kernel's own algorithm in NumPy (four 8-bit histogram passes over the fp32 bit
patterns, then the ordered ballot/popcount count over chunks, waves and lanes); with ``rule`` other than "index" it
applies one of three WRONG tie rules, which the CPU tests show to change the mask of every tie case.
"""
import numpy as np

from oracle import loss_oracle as lo

F32 = np.float32
CHUNK = 1024            # csrc/ssd_loss.hip kLossThreads: anchors per pass of the ordered count
WAVE = 64
SATURATED_LOSS = F32(-np.log(F32(1) - F32(1e-7)))          # 1.192093e-07

POSITIVE, FILLER, SATURATED = -1, -2, -3                   # ``Case.level`` codes; >= 0: index into the palette
TIE_RULES_WRONG = ("reverse", "ge", "gt")                  # highest index first; every key >= T; only keys > T


def softmax32(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(F32)


def level_row(p0, L):
    z = np.zeros(L, F32)
    z[0] = F32(np.log(p0 / (1.0 - p0) * (L - 1)))
    return z


def total_neg(P, ratio):
    """tf.cast(total_pos * neg_pos_ratio, int32) in fp32 (reference ssd_loss.py:52)."""
    return int(F32(P) * F32(ratio))


def find_fp32_truncation_pair(p_max=2000):
    """Smallest P (then smallest ratio in hundredths, below 4) for which the fp32 product P * ratio truncates to another
    integer than the double product: the kernel must take the fp32 one.  None if there is no pair below ``p_max``."""
    ratios = np.array([r / 100.0 for r in range(1, 400) if r % 100], np.float64)
    for P in range(1, p_max):
        k32 = (F32(P) * ratios.astype(F32)).astype(np.int32)
        k64 = (float(P) * ratios).astype(np.int32)
        bad = np.nonzero(k32 != k64)[0]
        if bad.size:
            return P, float(ratios[bad[0]]), int(k32[bad[0]]), int(k64[bad[0]])
    return None


class Case(object):
    """One image.  ``palette``: [(p0, count), ...]; ``saturated``: count of saturated backgrounds; ``kind``: "cut_inside" |
    "cut_at_end" | "zero" (T = 0: the positives rank a second time) | "all" | "none"; ``tie``: the three wrong tie rules
    must change this image's mask; ``filler_shift``: what the filler rows add to z0 (6: a few of some thousand rows still
    lose more than the 0.3 level, which puts keys above T among the tied ones; 9: none does); ``expect``: t_level (palette
    index, SATURATED, or POSITIVE for T = 0), group (keys equal to T), taken (of them selected), chunks (the 1024-chunks
    the group touches), last_chunk (where the last one taken lies)."""

    def __init__(self, name, purpose, N, L, P, ratio, palette=(), saturated=0, kind="cut_inside", tie=True, expect=None,
                 seed=1, shared_positive_row=False, filler_shift=6.0):
        self.name, self.purpose, self.N, self.L, self.P, self.ratio = name, purpose, N, L, P, float(ratio)
        self.palette, self.kind, self.tie, self.expect = list(palette), kind, tie, dict(expect or {})
        self.K = total_neg(P, ratio)
        rng = np.random.default_rng(seed)
        perm = rng.permutation(N)
        level = np.full(N, FILLER, np.int64)
        level[perm[:P]] = POSITIVE
        at = P
        for i, (_, count) in enumerate(self.palette):
            level[perm[at:at + count]] = i
            at += count
        level[perm[at:at + saturated]] = SATURATED
        at += saturated
        assert at <= N, "%s: more anchors asked for than N" % name
        z = rng.standard_normal((N, L)).astype(F32)
        z[:, 0] += F32(filler_shift)
        for i, (p0, _) in enumerate(self.palette):
            z[level == i] = level_row(p0, L)
        sat = np.zeros(L, F32)
        sat[0] = 40
        z[level == SATURATED] = sat
        pos = np.sort(perm[:P])
        cls = rng.integers(1, L, P)
        z[pos] = (rng.standard_normal((P, L)) * 2).astype(F32)
        if shared_positive_row:                          # one row, one class: mask-2 rows are exactly twice mask-1 rows
            cls[:] = 1
            z[pos] = z[pos[0]] if P else 0
        yl = np.zeros((N, L), F32)
        yl[:, 0] = 1
        yl[pos, 0] = 0
        yl[pos, cls] = 1
        yd = np.zeros((N, 4), F32)
        yd[pos] = (rng.standard_normal((P, 4)) * 2).astype(F32)
        self.level, self.pos = level, level == POSITIVE
        self.z, self.pp, self.yl, self.yd = z, softmax32(z), yl, yd
        self.pd = (rng.standard_normal((N, 4)) * 1.5).astype(F32)
        self.ce_cpu = lo.cross_entropy(yl[None], self.pp[None])[0]

    def __repr__(self):
        return "Case(%s)" % self.name


class Batch(object):
    """Images that share N, L and the ratio, stacked: one kernel launch, which also checks that images do not leak into
    each other."""

    def __init__(self, name, cases):
        self.name, self.cases = name, list(cases)
        c0 = self.cases[0]
        assert all((c.N, c.L, c.ratio) == (c0.N, c0.L, c0.ratio) for c in self.cases)
        self.ratio, self.N, self.L, self.B = c0.ratio, c0.N, c0.L, len(self.cases)
        for f in ("yd", "yl", "pd", "z", "pp"):
            setattr(self, f, np.stack([getattr(c, f) for c in self.cases]))

    def oracle_masks(self, ce=None):
        """final_mask [B,N] of oracle/loss_oracle.py, from ``ce`` [B,N] (the device's own) or from its own losses."""
        return lo.conf_loss_fn(self.yl, self.pp, self.ratio, return_parts=True, ce=ce)[2]

    def __repr__(self):
        return "Batch(%s)" % self.name


def assert_not_vacuous(case, oracle_mask, ce=None):
    """The case does what it says, on the oracle's mask [N] (computed from ``ce`` [N]; default: the CPU losses)."""
    ce = case.ce_cpu if ce is None else np.asarray(ce, F32)
    N, K, e = case.N, case.K, case.expect
    mask = np.asarray(oracle_mask, F32)
    pos = case.pos
    neg = mask - pos.astype(F32)
    assert set(np.unique(neg)) <= {0.0, 1.0}, case
    assert int(pos.sum()) == case.P and int(neg.sum()) == min(max(K, 0), N), case
    if case.kind == "all":
        assert K >= N and case.P > 0 and (neg == 1).all() and (mask[pos] == 2).all(), case
        return
    if case.kind == "none":
        assert K == 0 and case.P > 0 and np.array_equal(mask, pos.astype(F32)), case
        return
    assert 0 < K < N, case
    masked = (ce * case.yl[:, 0]).astype(F32)
    T = np.sort(masked)[::-1][K - 1]
    group = masked == T
    taken = int((group & (neg == 1)).sum())
    assert int((masked > T).sum()) + taken == K, case
    want = pos | (masked == 0) if e["t_level"] == POSITIVE else case.level == e["t_level"]
    assert np.array_equal(group, want), "%s: the group at T is not the level it should be" % case
    assert int(group.sum()) == e["group"], (case, int(group.sum()))
    assert sorted(set((np.nonzero(group)[0] // CHUNK).tolist())) == list(e["chunks"]), case
    assert taken == e["taken"], (case, taken)
    # ... and the tie-break is what decides: the taken ones are the group's lowest indices
    assert np.array_equal(np.nonzero(group & (neg == 1))[0], np.nonzero(group)[0][:taken]), case
    if case.kind == "cut_inside":
        assert 0 < taken < e["group"], case
    elif case.kind == "cut_at_end":
        assert taken == e["group"] and int((masked < T).sum()) > 0, case
    elif case.kind == "zero":
        assert T == 0 and e["t_level"] == POSITIVE and 0 < int((mask == 2).sum()) < case.P, case
        assert int((mask == 2).sum()) == K - int((~pos).sum()), case
        if "last_chunk" in e:
            assert int(np.nonzero(mask == 2)[0][-1]) // CHUNK == e["last_chunk"], case
    else:
        raise AssertionError("unknown kind %r" % case.kind)
    if "last_chunk" in e and case.kind != "zero":
        assert int(np.nonzero(group & (neg == 1))[0][-1]) // CHUNK == e["last_chunk"], case


def radix_select_restatement(masked, K, rule="index"):
    """csrc/ssd_loss.hip phases B and C for one image in NumPy -> neg_mask [N] (float32 0 / 1).  ``rule``: "index" is the
    kernel's (and TF's) tie-break; "reverse", "ge" and "gt" are the wrong ones of TIE_RULES_WRONG; "no_running" is the
    right rule with the carry across chunks dropped."""
    m = np.asarray(masked, F32)
    keys = np.where(m == 0, F32(0), m).astype(F32).view(np.uint32).astype(np.int64)        # -0.0 ranks as 0.0
    N = keys.size
    if K >= N:
        return np.ones(N, F32)
    if K <= 0:
        return np.zeros(N, F32)
    prefix, need = 0, K
    for shift in (24, 16, 8, 0):
        himask = 0 if shift == 24 else (0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF
        sel = (keys & himask) == (prefix & himask)
        hist = np.bincount((keys[sel] >> shift) & 255, minlength=256)
        cum, b = 0, 255
        while b > 0:
            if cum + hist[b] >= need:
                break
            cum += hist[b]
            b -= 1
        prefix |= b << shift
        need -= cum
    T = prefix
    total = int((keys == T).sum())
    neg = np.zeros(N, F32)
    running = 0
    for n0 in range(0, N, CHUNK):
        k = np.zeros(CHUNK, np.int64)
        inside = np.zeros(CHUNK, bool)
        n1 = min(N, n0 + CHUNK)
        k[:n1 - n0] = keys[n0:n1]
        inside[:n1 - n0] = True
        eq = inside & (k == T)
        ballots = eq.reshape(CHUNK // WAVE, WAVE)
        pop = ballots.sum(1)                                              # shi[wv] = popcount(ballot)
        take = np.zeros((CHUNK // WAVE, WAVE), bool)
        for wv in range(CHUNK // WAVE):
            before = running + int(pop[:wv].sum()) + (np.cumsum(ballots[wv]) - ballots[wv])       # lanes below this one
            if rule == "index":
                chosen = ballots[wv] & (before < need)
            elif rule == "reverse":
                chosen = ballots[wv] & (total - 1 - before < need)
            elif rule == "ge":
                chosen = ballots[wv]
            elif rule == "gt":
                chosen = np.zeros(WAVE, bool)
            elif rule == "no_running":                   # the count forgets the chunks before this one
                chosen = ballots[wv] & (before - running < need)
            else:
                raise ValueError(rule)
            take[wv] = (k.reshape(-1, WAVE)[wv] > T) | chosen
        running += int(pop.sum())
        neg[n0:n1] = (take.reshape(-1) & inside)[:n1 - n0]
    return neg


def _ties(name, N, P, ratio, purpose, expect, kind="cut_inside", L=21, seed=1):
    """The "everything ties" image: every background at p0 = 0.3."""
    return Case(name, purpose, N, L, P, ratio, palette=[(0.3, N - P)], kind=kind, expect=expect, seed=seed)


_CACHE = {}


def batches():
    """All mining batches, built once per process: {name: Batch}."""
    if not _CACHE:
        _build_cases()
    return _CACHE


def all_cases():
    return [c for b in batches().values() for c in b.cases]


def _build_cases():
    N, L = 2500, 21                  # two full 1024-chunks and a ragged 452 (not a multiple of 64)
    c3 = [0, 1, 2]
    ratio3 = [
        Case("wide_group", "T inside a 900-anchor group that spans all three chunks", N, L, 40, 3,
             palette=[(0.1, 50), (0.3, 900)], expect=dict(t_level=1, group=900, taken=67, chunks=c3, last_chunk=0)),
        Case("narrow_group", "T inside a 64-anchor group; the last one taken lies in the ragged chunk", N, L, 40, 3,
             palette=[(0.1, 56), (0.3, 64)], expect=dict(t_level=1, group=64, taken=60, chunks=c3, last_chunk=2)),
        _ties("everything_ties", N, 40, 3, "every background ties: the first 120 by index are taken",
              dict(t_level=0, group=2460, taken=120, chunks=c3, last_chunk=0)),
        Case("cut_at_group_end", "K ends exactly at the end of the group: all 15, none beyond", N, L, 5, 3,
             palette=[(0.3, 15)], kind="cut_at_end", tie=False, filler_shift=9.0, expect=dict(t_level=0, group=15, taken=15, chunks=c3)),
        Case("saturated_floor", "T is the clip floor 1.192093e-07 shared by 2100 saturated backgrounds", N, L, 300, 3,
             palette=[(0.3, 100)], saturated=2100,
             expect=dict(t_level=SATURATED, group=2100, taken=800, chunks=c3, last_chunk=0)),
        Case("negatives_run_out", "K above the 1800 backgrounds: T = 0, 300 of the 700 positives get mask 2", N, L, 700, 3,
             palette=[(0.3, 100)], kind="zero", shared_positive_row=True,
             expect=dict(t_level=POSITIVE, group=700, taken=300, chunks=c3)),
    ]
    _CACHE["ratio3"] = Batch("ratio3", ratio3)
    _CACHE["all"] = Batch("all", [Case("all", "K >= N: every anchor selected, positives mask 2", N, L, 10, 300,
                                       kind="all", tie=False, shared_positive_row=True)])
    _CACHE["none"] = Batch("none", [Case("none", "K = 0 with positives: the mask is the positives, denominator 2",
                                         N, L, 2, 0.4, kind="none", tie=False)])
    # the cut on and just past a wave boundary (64) and a chunk boundary (1024) of the prefix count: ratio 1, P = K
    cuts = []
    for K in (1, 64, 65, 1024, 1025):
        nb = N - K
        group_chunks = c3
        cuts.append(_ties("ties_K%d" % K, N, K, 1, "everything ties, the cut after %d tied anchors" % K,
                          dict(t_level=0, group=nb, taken=K, chunks=group_chunks), seed=K))
    _CACHE["cuts"] = Batch("cuts", cuts)
    n9 = list(range(9))
    _CACHE["nine_chunks"] = Batch("nine_chunks", [
        Case("nine_chunks_wide", "N = 8732: a 4000-anchor group over nine chunks, cut in the first", 8732, L, 100, 3,
             palette=[(0.1, 100), (0.3, 4000)], expect=dict(t_level=1, group=4000, taken=199, chunks=n9, last_chunk=0)),
        Case("nine_chunks_deep", "N = 8732: `running` carried over eight chunks before the cut in the ninth", 8732, L, 1500,
             3, palette=[(0.1, 500), (0.3, 4200)], expect=dict(t_level=1, group=4200, taken=3998, chunks=n9, last_chunk=8),
             seed=2),
    ])
    _CACHE["partial_wave"] = Batch("partial_wave", [
        Case("partial_wave", "N = 50: one partial wave", 50, 3, 4, 3, palette=[(0.1, 5), (0.3, 20)],
             expect=dict(t_level=1, group=20, taken=7, chunks=[0], last_chunk=0)),
        Case("partial_wave_all_tie", "N = 50, every background ties", 50, 3, 6, 3, palette=[(0.3, 44)],
             expect=dict(t_level=0, group=44, taken=18, chunks=[0], last_chunk=0), seed=2),
    ])
    pair = find_fp32_truncation_pair()
    assert pair is not None, "no (P, ratio) below P = 2000 truncates differently in fp32 and double"
    P, ratio, k32, k64 = pair
    assert k32 != k64 and total_neg(P, ratio) == k32
    _CACHE["fp32_product"] = Batch("fp32_product", [
        _ties("fp32_product", N, P, ratio, "int(f32(P) * f32(ratio)) = %d, the double product gives %d" % (k32, k64),
              dict(t_level=0, group=N - P, taken=k32, chunks=c3))])


def clip_edge_batch():
    """Gradient clip edges (one image, ratio 3): positives whose true-class probability lies below 1e-7 (z_true = -40:
    loss -log(1e-7), selected, gradient row all zero) or saturates above 1 - 1e-7 (z_true = +40: p == 1.0), among
    ordinary positives.  Returns (Batch, below [N] bool, above [N] bool)."""
    c = Case("clip_edges", "positives outside the clip range on either side", 300, 21, 24, 3, palette=[(0.3, 100)],
             seed=5)
    pos = np.nonzero(c.pos)[0]
    below, above = np.zeros(c.N, bool), np.zeros(c.N, bool)
    below[pos[0:16:2]] = True
    above[pos[1:16:2]] = True
    cls = c.yl.argmax(-1)
    for n in np.nonzero(below)[0]:
        c.z[n, cls[n]] = -40
    for n in np.nonzero(above)[0]:
        c.z[n, cls[n]] = 40
    c.pp = softmax32(c.z)
    c.ce_cpu = lo.cross_entropy(c.yl[None], c.pp[None])[0]
    p_true = c.pp[np.arange(c.N), cls]
    assert (p_true[below] < 1e-8).all() and (p_true[below] > 0).all() and (p_true[above] == 1).all()     # off the bounds
    return Batch("clip_edges", [c]), below, above


def localisation_edge_batch():
    """Five images (N = 130, L = 4, ratio 3) for the localisation term's edges -> (yd, yl, pd, z, pp, notes).
    0: errors of exactly 0, +-1 and +-3 on positives (the Huber knee and both linear branches);
    1: one target whose only non-zero component is the denormal 1e-40 (a positive for NumPy and the reference), and one
       target of all -0.0 (not a positive);
    2: label positives whose deltas are all zero (a prior equal to its box): pos_loc = 0 while pos_conf > 0;
    3: no positives at all: both losses 0, both gradients entirely zero;
    4: an ordinary image."""
    B, N, L = 5, 130, 4
    rng = np.random.default_rng(7)
    yd = np.zeros((B, N, 4), F32)
    yl = np.zeros((B, N, L), F32)
    yl[..., 0] = 1
    pd = (rng.standard_normal((B, N, 4)) * 1.5).astype(F32)
    z = rng.standard_normal((B, N, L)).astype(F32)
    z[..., 0] += 2

    def label(b, idx):
        yl[b, idx, 0] = 0
        yl[b, idx, 1 + np.arange(len(idx)) % (L - 1)] = 1

    idx0 = np.array([3, 63, 64, 65, 127, 128, 129])
    yd[0, idx0] = np.array([0.5, -2.0, 4.0, 0.25], F32)
    errs = np.array([[0, 1, -1, 3], [-3, 0, 1, -1], [1, 1, 1, 1], [-1, -1, -1, -1], [3, -3, 3, -3], [0, 0, 0, 0],
                     [0.5, -0.5, 2, -2]], F32)
    pd[0, idx0] = yd[0, idx0] + errs
    assert np.array_equal(pd[0, idx0] - yd[0, idx0], errs)                # exactly 0, +-1, +-3
    label(0, idx0)
    yd[1, 70, 2] = F32(1e-40)
    assert yd[1, 70, 2] != 0 and yd[1, 70].view(np.uint32)[2] == 71362     # a denormal bit pattern, not zero
    yd[1, 5] = F32(-0.0)
    assert np.signbit(yd[1, 5]).all()
    yd[1, 100] = (0.5, 0.5, -1, 2)
    label(1, np.array([70, 100]))                                          # anchor 5 (-0.0) stays background
    label(2, np.array([1, 64, 129]))                                       # deltas stay zero
    idx4 = rng.choice(N, 9, replace=False)
    yd[4, idx4] = (rng.standard_normal((9, 4)) * 2).astype(F32)
    label(4, idx4)
    notes = dict(knee=(0, idx0), denormal=(1, 70), negative_zero=(1, 5), zero_delta_positives=2, empty=3)
    return yd, yl, pd, z, softmax32(z), notes


def quantised_random_image(rng, n_max=3000, levels=8):
    """A random image whose background losses take ``levels`` distinct values -> (masked [N], K): heavy ties at every
    threshold, for the restatement against the oracle."""
    N = int(rng.integers(1, n_max + 1))
    values = np.sort(rng.random(levels).astype(F32) * F32(3) + F32(1e-3))
    if rng.random() < 0.3:
        values[0] = SATURATED_LOSS
    masked = values[rng.integers(0, levels, N)]
    P = int(rng.integers(0, max(2, N // 3)))
    pos = rng.choice(N, min(P, N), replace=False)
    masked[pos] = 0
    if rng.random() < 0.2 and pos.size:
        masked[pos[: pos.size // 2]] = F32(-0.0)
    K = int(rng.integers(0, N + 3)) if rng.random() < 0.7 else total_neg(pos.size, 3)
    return masked.astype(F32), K
