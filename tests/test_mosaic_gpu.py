"""Mosaic augmentation on the device (csrc/ssd_mosaic.hip) against its NumPy restatement (tests/mosaic_cases.py, pinned
without a GPU by test_mosaic_cpu.py): plan, boxes, labels and info BIT-EQUAL, the pixels bit-equal image by image (compared
as uint32, no tolerance: the plan kernel makes the restatement's fp32 operations in its order, the tile pixels are the
geometry kernel's four taps, which test_augment_batch_gpu.py holds to ``resize_bilinear``); nothing written outside the
outputs; determinism; ``out=`` reuse; every refusal of include/ssd_hip.h with the outputs untouched; the feed."""
import ctypes

import numpy as np
import pytest

import mosaic_cases as mc

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 0x5A5A5A5A          # the pattern around (and, before a call, inside) every output
PAD = 64                    # guard elements on each side


def _guarded(shape, dtype):
    """(the whole buffer as int32, the output in its middle): both filled with GUARD."""
    import torch
    import ssd_hip as h
    n = int(np.prod(shape))
    whole = torch.full((PAD + n + PAD,), GUARD, dtype=torch.int32, device=h.device())
    return whole, whole[PAD:PAD + n].view(dtype).view(shape)


def _guards_intact(whole, inside=False):
    n = whole.numel() - 2 * PAD
    ok = bool((whole[:PAD] == GUARD).all()) and bool((whole[PAD + n:] == GUARD).all())
    return ok and (not inside or bool((whole == GUARD).all()))


def _plan_outputs(B, G_out):
    import torch
    return [_guarded(s, d) for s, d in (((B, 16), torch.int32), ((B, G_out, 4), torch.float32), ((B, G_out), torch.int32),
                                        ((B, 4), torch.int32))]


def _assert_bit_equal(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    assert bad.size == 0, "%s: %d values differ, first at %s: %r != %r" % (what, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


def _run_case(c):
    import augmentation as aug
    out = aug.mosaic_plan_device(c.boxes, c.labels, c.ids, c.H, c.W, mc.SEED, c.p, c.scale, c.max_boxes)
    return out, aug.run_mosaic_device(c.images, out[0], mc.FILL)


@pytest.mark.parametrize("name", mc.CASES)
def test_bit_equal_to_the_restatement(name):
    c, ref = mc.case(name), mc.reference(name)
    out, px = _run_case(c)
    assert tuple(out[1].shape) == (c.boxes.shape[0], mc.rows_out(c), 4)
    for n, t in zip(mc.NAMES, out):
        _assert_bit_equal(t.cpu().numpy(), ref[n], "%s %s" % (name, n))
    px = px.cpu().numpy()
    for b in range(px.shape[0]):            # image by image: a wrong source or tile names its image
        _assert_bit_equal(px[b], ref["pixels"][b], "%s pixels of image %d (plan %s)" % (name, b, ref["plan"][b].tolist()))


@pytest.mark.parametrize("name", ["SMALL", "SMALL_HALF", "CAP"])
def test_nothing_is_written_outside_the_outputs(name):
    import torch
    import ssd_hip as h
    c, ref = mc.case(name), mc.reference(name)
    B, G = c.labels.shape
    G_out = mc.rows_out(c)
    g, gl, ids, x = h.to_dev(c.boxes), h.to_dev(c.labels, torch.int32), h.to_dev(c.ids, torch.int64), h.to_dev(c.images)
    outs = _plan_outputs(B, G_out)
    h.check(h.lib().ssd_augment_mosaic_plan(h.ptr(g), h.ptr(gl), h.ptr(ids), B, G, c.H, c.W, mc.SEED, c.p, c.scale[0], c.scale[1], G_out,
                                            mc.PAD_LABEL, *[h.ptr(v) for _, v in outs], h.stream()), "ssd_augment_mosaic_plan")
    whole, px = _guarded((B, c.H, c.W, 3), torch.float32)
    fill = (ctypes.c_float * 3)(*mc.FILL)
    h.check(h.lib().ssd_augment_mosaic_pixels(h.ptr(x), B, c.H, c.W, h.ptr(outs[0][1]), fill, h.ptr(px), h.stream()),
            "ssd_augment_mosaic_pixels")
    torch.cuda.synchronize()
    assert all(_guards_intact(w) for w, _ in outs) and _guards_intact(whole)
    for n, (_, v) in zip(mc.NAMES, outs):
        _assert_bit_equal(v.cpu().numpy(), ref[n], "%s %s" % (name, n))
    _assert_bit_equal(px.cpu().numpy(), ref["pixels"], name + " pixels")
    # the inputs are read only
    assert np.array_equal(g.cpu().numpy(), c.boxes) and np.array_equal(gl.cpu().numpy(), c.labels) and np.array_equal(x.cpu().numpy(), c.images)


def test_same_call_twice_same_bits_and_batch_is_plan_plus_run():
    import torch
    import augmentation as aug
    c = mc.case("SMALL_HALF")
    (p1, b1, l1, i1), x1 = _run_case(c)
    (p2, b2, l2, i2), x2 = _run_case(c)
    for a, b in ((p1, p2), (l1, l2), (i1, i2), (b1.view(torch.int32), b2.view(torch.int32)), (x1.view(torch.int32), x2.view(torch.int32))):
        assert torch.equal(a, b)
    im, gb, gl = aug.mosaic_batch_device(c.images, c.boxes, c.labels, c.ids, seed=mc.SEED, p=c.p, scale=c.scale)
    assert im.is_cuda and gb.is_cuda and gl.is_cuda and gl.dtype == torch.int32
    assert torch.equal(im.view(torch.int32), x1.view(torch.int32)) and torch.equal(gb.view(torch.int32), b1.view(torch.int32))
    assert torch.equal(gl, l1)
    other = aug.mosaic_plan_device(c.boxes, c.labels, c.ids, c.H, c.W, mc.SEED + 1, c.p, c.scale)
    assert not torch.equal(other[0], p1)                                    # the seed matters


def test_out_reuse_allocates_nothing():
    import torch
    import augmentation as aug
    import ssd_hip as h
    c, ref = mc.case("SMALL"), mc.reference("SMALL")
    B, G = c.labels.shape
    G_out = mc.rows_out(c)
    g, gl, ids = h.to_dev(c.boxes), h.to_dev(c.labels, torch.int32), h.to_dev(c.ids, torch.int64)
    out = aug.mosaic_plan_device(g, gl, ids, c.H, c.W, mc.SEED)
    for t in out:
        t.fill_(0)
    torch.cuda.synchronize()
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]       # requests to the caching allocator, cached or not

    def requests(fn):
        before = count()
        fn()
        return count() - before
    # what passing the inputs through ``ssd_hip.to_dev`` costs by itself: nothing for device tensors of the right type in the
    # product, one guarded copy per fp32 tensor under this suite's conftest (which wraps ``to_dev``)
    inputs = requests(lambda: (h.to_dev(g), h.to_dev(gl, torch.int32), h.to_dev(ids, torch.int64)))
    fresh = requests(lambda: aug.mosaic_plan_device(g, gl, ids, c.H, c.W, mc.SEED))
    reused = [requests(lambda: aug.mosaic_plan_device(g, gl, ids, c.H, c.W, mc.SEED, out=out)) for _ in range(3)]
    print("allocation requests: inputs %d, without out= %d, with out= %r" % (inputs, fresh, reused))
    assert inputs <= 1 and fresh == inputs + 4 and reused == [inputs] * 3
    back = aug.mosaic_plan_device(g, gl, ids, c.H, c.W, mc.SEED, out=out)
    assert all(a is b for a, b in zip(back, out))
    for n, t in zip(mc.NAMES, out):
        _assert_bit_equal(t.cpu().numpy(), ref[n], "out= " + n)
    with pytest.raises(ValueError):
        aug.mosaic_plan_device(g, gl, ids, c.H, c.W, mc.SEED, out=out[:1] + (out[1][:, :G],) + out[2:])
    with pytest.raises(ValueError):
        aug.mosaic_plan_device(g, gl, ids, c.H, c.W, mc.SEED, out=out[:2] + (out[2].to(torch.int64),) + out[3:])
    with pytest.raises(ValueError):
        aug.mosaic_plan_device(g, None, ids, c.H, c.W, mc.SEED)
    # (an output that IS an input is the library's refusal: test_plan_refusals_leave_the_outputs_untouched[alias=...] at the C
    # entry -- through Python this suite's conftest hands the kernel a guarded copy of every fp32 input, never the tensor itself)
    assert G_out == 4 * G


# ---------------------------------------------------------------------------------------------------------- the refusals
UNSUPPORTED, INVALID = -3, -1
_BASE = dict(B=8, G=6, H=23, W=37, p=1.0, lo=0.5, hi=1.0, G_out=24)
_PLAN_REFUSALS = [
    (UNSUPPORTED, dict(H=1)), (UNSUPPORTED, dict(H=4097)), (UNSUPPORTED, dict(W=1)), (UNSUPPORTED, dict(W=4097)),
    (UNSUPPORTED, dict(G=0)), (UNSUPPORTED, dict(G=513, G_out=2048)), (UNSUPPORTED, dict(G_out=5)), (UNSUPPORTED, dict(G_out=2049)),
    (UNSUPPORTED, dict(B=65536)),
    (INVALID, dict(B=-1)), (INVALID, dict(p=-0.01)), (INVALID, dict(p=1.01)), (INVALID, dict(p=float("nan"))),
    (INVALID, dict(lo=0.05)), (INVALID, dict(lo=1.0, hi=0.5)), (INVALID, dict(hi=2.5)), (INVALID, dict(lo=float("nan"))),
] + [(INVALID, dict(null=i)) for i in range(7)] + [(INVALID, dict(alias=a)) for a in ("boxes", "labels", "ids", "boxes tail", "outputs")]


@pytest.mark.parametrize("code, change", _PLAN_REFUSALS, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_plan_refusals_leave_the_outputs_untouched(code, change):
    """Every condition of the header: its code, and the guard pattern still everywhere -- nothing was launched.  The tensors
    keep the base sizes whatever the call claims: a refusal comes before any launch."""
    import torch
    import ssd_hip as h
    c = mc.case("SMALL")
    a = dict(_BASE, **{k: v for k, v in change.items() if k in _BASE})
    g, gl, ids = h.to_dev(c.boxes), h.to_dev(c.labels, torch.int32), h.to_dev(c.ids, torch.int64)
    outs = _plan_outputs(_BASE["B"], _BASE["G_out"])
    ptrs = [h.ptr(g), h.ptr(gl), h.ptr(ids)] + [h.ptr(v) for _, v in outs]
    if "null" in change:
        ptrs[change["null"]] = None
    alias = change.get("alias")
    if alias == "boxes":
        ptrs[4] = ptrs[0]
    elif alias == "labels":
        ptrs[5] = ptrs[1]
    elif alias == "ids":
        ptrs[6] = ptrs[2]
    elif alias == "boxes tail":             # the output begins inside the input's last row
        ptrs[4] = h.vp(g.data_ptr() + g.numel() * 4 - 16)
    elif alias == "outputs":
        ptrs[6] = ptrs[3]
    rc = h.lib().ssd_augment_mosaic_plan(ptrs[0], ptrs[1], ptrs[2], a["B"], a["G"], a["H"], a["W"], mc.SEED, a["p"], a["lo"], a["hi"],
                                         a["G_out"], mc.PAD_LABEL, ptrs[3], ptrs[4], ptrs[5], ptrs[6], h.stream())
    assert rc == code and b"ssd_augment_mosaic_plan" in h.lib().ssd_last_error()
    torch.cuda.synchronize()
    assert all(_guards_intact(w, inside=True) for w, _ in outs)
    assert np.array_equal(g.cpu().numpy(), c.boxes) and np.array_equal(gl.cpu().numpy(), c.labels)


_PIXEL_REFUSALS = [(UNSUPPORTED, dict(H=1)), (UNSUPPORTED, dict(H=4097)), (UNSUPPORTED, dict(W=1)), (UNSUPPORTED, dict(W=4097)),
                   (UNSUPPORTED, dict(B=65536)), (INVALID, dict(B=-1))] + [(INVALID, dict(null=i)) for i in range(4)] + [
                   (INVALID, dict(alias="images")), (INVALID, dict(alias="plan"))]


@pytest.mark.parametrize("code, change", _PIXEL_REFUSALS, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_pixel_refusals_leave_the_output_untouched(code, change):
    import torch
    import ssd_hip as h
    c, ref = mc.case("SMALL"), mc.reference("SMALL")
    a = dict(_BASE, **{k: v for k, v in change.items() if k in _BASE})
    x, plan = h.to_dev(c.images), h.to_dev(ref["plan"], torch.int32)
    whole, out = _guarded(tuple(x.shape), torch.float32)
    fill = (ctypes.c_float * 3)(*mc.FILL)
    ptrs = [h.ptr(x), h.ptr(plan), fill, h.ptr(out)]
    if "null" in change:
        ptrs[change["null"]] = None
    if change.get("alias") == "images":
        ptrs[3] = h.vp(x.data_ptr() + 12)
    elif change.get("alias") == "plan":
        ptrs[3] = ptrs[1]
    rc = h.lib().ssd_augment_mosaic_pixels(ptrs[0], a["B"], a["H"], a["W"], ptrs[1], ptrs[2], ptrs[3], h.stream())
    assert rc == code and b"ssd_augment_mosaic_pixels" in h.lib().ssd_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(whole, inside=True)
    assert np.array_equal(x.cpu().numpy(), c.images) and np.array_equal(plan.cpu().numpy(), ref["plan"])


def test_empty_batch_is_a_no_op_and_python_raises_the_library_codes():
    import torch
    import augmentation as aug
    import ssd_hip as h
    outs = _plan_outputs(_BASE["B"], _BASE["G_out"])
    assert h.lib().ssd_augment_mosaic_plan(None, None, None, 0, 6, 23, 37, 0, 1.0, 0.5, 1.0, 24, -1, None, None, None, None, h.stream()) == 0
    assert h.lib().ssd_augment_mosaic_pixels(None, 0, 23, 37, None, None, None, h.stream()) == 0
    torch.cuda.synchronize()
    assert all(_guards_intact(w, inside=True) for w, _ in outs)
    c = mc.case("SMALL")
    with pytest.raises(h.SsdHipUnsupported) as e:
        aug.mosaic_plan_device(c.boxes, c.labels, c.ids, c.H, c.W, mc.SEED, max_boxes=2049)
    assert "ssd_augment_mosaic_plan" in str(e.value) and "2049" in str(e.value)
    with pytest.raises(h.SsdHipUnsupported):
        aug.mosaic_plan_device(c.boxes, c.labels, c.ids, 4097, c.W, mc.SEED)
    with pytest.raises(ValueError):
        aug.mosaic_plan_device(c.boxes, c.labels, c.ids, c.H, c.W, mc.SEED, p=1.5)
    with pytest.raises(ValueError):
        aug.mosaic_plan_device(c.boxes, c.labels, c.ids, c.H, c.W, mc.SEED, scale=(1.0, 0.5))


# ------------------------------------------------------------------------------------------------------------- the feed
def test_mosaicked_feeds_the_augmentation_and_the_target_assignment():
    """``mosaicked`` -> ``apply_batch_device`` (through ``augmented`` + ``device_draws``) -> ``calculate_actual_outputs`` on a
    B = 4 synthetic batch: finite targets of the usual shapes, and the mosaic stage alone is the restatement's."""
    import torch
    import augmentation as aug
    from utils import bbox_utils, data_utils, train_utils
    hp = train_utils.get_hyper_params("mobilenet_v2")
    hp["total_labels"] = 21
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    B, S = 4, 64
    imgs = data_utils.synthetic_images(B, S, seed=5)
    gt, gl = data_utils.synthetic_gt(B, max_boxes=6, seed=6)
    offset = 1 << 40
    (im, gb, lab), = list(aug.mosaicked([(imgs, gt, gl)], 1.0, mc.SEED, rank_offset=offset))
    ref = mc.mosaic_batch(mc.SEED, np.arange(offset, offset + B), gt, gl, S, S, 1.0, (0.5, 1.0), 24, imgs)
    assert tuple(gb.shape) == (B, 24, 4) and tuple(lab.shape) == (B, 24) and (ref["info"][:, 2] > 0).all()
    _assert_bit_equal(gb.cpu().numpy(), ref["boxes"], "feed boxes")
    _assert_bit_equal(lab.cpu().numpy(), ref["labels"], "feed labels")
    _assert_bit_equal(im.cpu().numpy(), ref["pixels"], "feed pixels")
    stream = aug.augmented(aug.mosaicked([(imgs, gt, gl)], 1.0, mc.SEED, rank_offset=offset), aug.device_draws(mc.SEED, rank_offset=offset))
    (im2, gb2, lab2), = list(stream)
    assert tuple(im2.shape) == (B, S, S, 3) and tuple(gb2.shape) == (B, 24, 4) and torch.equal(lab2, lab)
    deltas, labels = train_utils.calculate_actual_outputs(priors, gb2, lab2, hp)
    N = priors.shape[0]
    assert tuple(deltas.shape) == (B, N, 4) and tuple(labels.shape) == (B, N, 21)
    assert bool(torch.isfinite(deltas).all()) and bool(torch.isfinite(labels).all()) and bool(torch.isfinite(im2).all())
    assert bool((labels.sum(-1) == 1).all()) and bool((labels[..., 1:].sum((1, 2)) > 0).all())     # one-hot rows, positives in every image


def test_a_mosaic_without_a_row_passes_the_device_draws_and_the_target_assignment():
    """Every mosaic of ``empty_mosaic_batch`` keeps no row.  Behind ``mosaicked`` the device draws give such an image no patch
    (the host draws' sampler raises on it, which is why ``trainer.mosaic_from_env`` refuses them): finite images, all-padding
    ground truth, every prior background."""
    import torch
    import augmentation as aug
    from utils import bbox_utils, train_utils
    hp = dict(train_utils.get_hyper_params("mobilenet_v2"), total_labels=21)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    images, boxes, labels = mc.empty_mosaic_batch()
    B, S = images.shape[0], images.shape[1]
    ref = mc.mosaic_batch(mc.SEED, np.arange(B), boxes, labels, S, S, 1.0, (0.5, 1.0), 4, images)
    assert (ref["info"][:, 2] == 0).all()
    stream = aug.augmented(aug.mosaicked([(images, boxes, labels)], 1.0, mc.SEED), aug.device_draws(mc.SEED))
    (im, gb, gl), = list(stream)
    _assert_bit_equal(gl.cpu().numpy(), ref["labels"], "labels")
    assert not gb.cpu().numpy().any() and bool(torch.isfinite(im).all()) and tuple(im.shape) == (B, S, S, 3)
    plan = aug.plan_batch_device(ref["boxes"], ref["labels"], np.arange(B), S, S, mc.SEED)
    assert not plan[0][:, 9].cpu().numpy().any()                            # no valid row: no patch
    deltas, onehot = train_utils.calculate_actual_outputs(priors, gb, gl, hp)
    assert bool(torch.isfinite(deltas).all()) and bool((onehot[..., 0] == 1).all())               # every prior background


def test_trainer_refuses_mosaic_beside_the_host_draws(monkeypatch, tmp_path):
    import importlib
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_TRAINER_MOSAIC", "0.5")
    monkeypatch.delenv("SSD_TRAINER_MOSAIC_SCALE", raising=False)
    monkeypatch.delenv("SSD_TRAINER_AUGMENT", raising=False)
    trainer = importlib.import_module("trainer")
    monkeypatch.setattr(trainer, "fit", lambda *a, **k: pytest.fail("the feed was built"))
    with pytest.raises(ValueError) as e:
        trainer.main(["--backbone", "mobilenet_v2"])
    assert "SSD_TRAINER_AUGMENT=gpu" in str(e.value)


def test_pixels_of_a_plan_row_outside_the_plan_kernels_ranges_are_fill():
    """The plan is device data: a tile whose row names no image of the batch, a centre off the image or a size beyond what the
    plan kernel writes shows the fill colour -- no arithmetic on such a row, nothing read outside the batch.  One image per
    kind, all four tiles alike, so the whole image is fill; the last image keeps the reference's plan and its pixels."""
    import torch
    import ssd_hip as h
    c, ref = mc.case("SMALL"), mc.reference("SMALL")
    B = c.images.shape[0]
    big, low = 2 ** 31 - 1, -2 ** 31
    plan = ref["plan"].copy()
    kinds = [dict(src=B), dict(src=-1), dict(hs=big), dict(ws=low), dict(hs=0), dict(hs=8193), dict(yc=big)]
    for b, kind in enumerate(kinds):
        plan[b, 0] = 1
        plan[b, 1] = kind.get("yc", plan[b, 1])
        for t in range(4):
            for k, name in enumerate(("src", "hs", "ws")):
                plan[b, 4 + 3 * t + k] = kind.get(name, plan[b, 4 + 3 * t + k])
    assert len(kinds) == B - 1
    x, pd = h.to_dev(c.images), h.to_dev(plan, torch.int32)
    whole, out = _guarded(tuple(x.shape), torch.float32)
    fill = (ctypes.c_float * 3)(0.25, 0.5, 0.75)
    h.check(h.lib().ssd_augment_mosaic_pixels(h.ptr(x), B, c.H, c.W, h.ptr(pd), fill, h.ptr(out), h.stream()), "ssd_augment_mosaic_pixels")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert _guards_intact(whole)
    for b in range(B - 1):
        assert (got[b] == np.array([0.25, 0.5, 0.75], F32)).all(), (b, kinds[b])
    _assert_bit_equal(got[B - 1], mc.pixels([int(v) for v in plan[B - 1]], B - 1, c.images, (0.25, 0.5, 0.75)), "the untouched row")


def _first_batch_of_trainer(monkeypatch, tmp_path, mosaic):
    """``trainer.main`` up to ``fit``: the first batch of its training feed and the calls ``mosaicked`` got."""
    import importlib
    import augmentation as aug
    monkeypatch.chdir(tmp_path)
    for k, v in (("SSD_TRAINER_EPOCHS", "1"), ("SSD_TRAINER_STEPS", "1"), ("SSD_TRAINER_BATCH", "4"), ("SSD_TRAINER_ITEMS", "4"),
                 ("SSD_TRAINER_AUGMENT", "gpu")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("SSD_VOC_DIR", raising=False)
    monkeypatch.delenv("SSD_TRAINER_MOSAIC_SCALE", raising=False)
    if mosaic is None:
        monkeypatch.delenv("SSD_TRAINER_MOSAIC", raising=False)
    else:
        monkeypatch.setenv("SSD_TRAINER_MOSAIC", mosaic)
    trainer = importlib.import_module("trainer")
    calls, got = [], {}
    real = aug.mosaicked
    monkeypatch.setattr(aug, "mosaicked", lambda *a, **k: calls.append((a[1:], k)) or real(*a, **k))
    monkeypatch.setattr(trainer, "fit", lambda model, train_feed, *a, **k: got.update(batch=next(train_feed)))
    trainer.main(["--backbone", "mobilenet_v2"])
    return got["batch"], calls


def test_trainer_feed_without_the_knob_is_the_parents_and_with_it_a_mosaic(monkeypatch, tmp_path):
    """Knob unset: ``mosaicked`` is never called and the first training batch is, bit for bit, what the feed built by hand the
    way the trainer builds it without the knob gives.  Knob set: one ``mosaicked`` in front, the same feed otherwise."""
    import torch
    import augmentation as aug
    from utils import bbox_utils, data_utils, train_utils
    (img, (deltas, labels)), calls = _first_batch_of_trainer(monkeypatch, tmp_path, None)
    assert calls == []
    hp = train_utils.get_hyper_params("mobilenet_v2")
    total = len(["bg"] + data_utils.get_labels())
    hp = dict(hp, total_labels=total)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    data = list(data_utils.synthetic_dataset(4, 4, hp["img_size"], total, seed=0))
    want_img, (want_deltas, want_labels) = next(train_utils.generator(aug.augmented(data, aug.device_draws(4242, rank_offset=0)), priors, hp))
    assert torch.equal(img.view(torch.int32), want_img.view(torch.int32))
    assert torch.equal(deltas.view(torch.int32), want_deltas.view(torch.int32)) and torch.equal(labels, want_labels)
    (img2, (deltas2, labels2)), calls = _first_batch_of_trainer(monkeypatch, tmp_path, "1")
    assert calls == [((1.0, 4242), {"rank_offset": 0, "scale": (0.5, 1.0)})]
    mos = aug.augmented(aug.mosaicked(data, 1.0, 4242, rank_offset=0), aug.device_draws(4242, rank_offset=0))
    want_img2, (want_deltas2, want_labels2) = next(train_utils.generator(mos, priors, hp))
    assert torch.equal(img2.view(torch.int32), want_img2.view(torch.int32)) and not torch.equal(img2, img)
    assert torch.equal(deltas2.view(torch.int32), want_deltas2.view(torch.int32)) and torch.equal(labels2, want_labels2)
    assert bool(torch.isfinite(deltas2).all())
