"""``ssd_augment_plan`` (csrc/ssd_augplan.hip) on the device against its NumPy restatement (tests/augment_plan_cases.py,
pinned without a GPU by test_augment_plan_cpu.py): all six outputs BIT-EQUAL -- the kernel makes the same fp32 operations
in the same order, every one rounded on its own, and the same integer draws -- over the listed image sizes, row counts,
batch sizes and sample ids above 2^32; the sampler outcomes a wave-parallel search can get wrong (a window accepted in the
lanes' second pass, no window at all, no valid row); independence of the batch; the in-place call; the pixels of
``apply_batch_device`` against the existing ``run_plans`` on the same plan; the refusals."""
import functools

import numpy as np
import pytest

import augment_plan_cases as pc

pytestmark = pytest.mark.gpu
F32 = np.float32


def _device_plan(boxes, labels, ids, H, W, seed=pc.SEED):
    import augmentation as aug
    out = aug.plan_batch_device(boxes, labels, ids, H, W, seed)
    return {n: t.cpu().numpy() for n, t in zip(pc.NAMES, out)}


def _assert_bit_equal(got, want, what=""):
    for n in pc.NAMES:
        g, w = np.asarray(got[n]), np.asarray(want[n])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s %s: %d values differ, first at %s: %r != %r" % (what, n, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _bit_case(name):
    _, H, W, G, B, gseed = next(c for c in pc.BIT_CASES if c[0] == name)
    boxes, labels = pc.ground_truth(B, G, seed=gseed)
    ids = pc.case_ids(B, name)
    return H, W, boxes, labels, ids, pc.plan_batch(pc.SEED, ids, H, W, boxes, labels)


@pytest.mark.parametrize("name", [c[0] for c in pc.BIT_CASES])
def test_plan_bit_equal_to_the_restatement(name):
    H, W, boxes, labels, ids, ref = _bit_case(name)
    assert (labels == 0).any() or boxes.shape[1] == 1
    assert (labels == -1).any() or boxes.shape[1] == 1
    _assert_bit_equal(_device_plan(boxes, labels, ids, H, W), ref, name)
    # without labels a row is valid iff its box is not all zero: the label-0 rows over a box now count
    ref2 = pc.plan_batch(pc.SEED, ids[:3], H, W, boxes[:3], None)
    _assert_bit_equal(_device_plan(boxes[:3], None, ids[:3], H, W), ref2, name + " (no labels)")


def test_required_sampler_outcomes():
    H, W, boxes, labels, ids = pc.outcome_batch()
    ref = pc.plan_batch(pc.SEED, ids, H, W, boxes, labels)
    info = ref["info"]
    # the restatement first: the case list holds what it must
    assert ((info[:, 0] >= 64) & (info[:, 0] < 100)).any() and (info[:, 0] == 100).any() and (info[:, 0] == 64).any()
    none = len(pc.LATE_IDS)
    assert not (labels[none] > 0).any() and info[none, 0] == -1
    patched = info[:, 0] >= 0
    assert (info[patched, 2] == 1).any() and (info[patched, 2] == 0).any()
    got = _device_plan(boxes, labels, ids, H, W)
    _assert_bit_equal(got, ref, "outcomes")
    np.testing.assert_array_equal(got["boxes"][none], boxes[none])           # no valid row: copied through, no patch
    assert got["geom"][none, 9] == 0


def test_plan_does_not_depend_on_the_batch():
    """The plan of (seed, id) at B = 1, inside a batch of 7 and at another position of that batch."""
    H, W, G = 37, 53, 5
    boxes, labels = pc.ground_truth(7, G, seed=51)
    ids = np.array([(1 << 34) + 3, 9, 10, 11, (1 << 34) + 3, 12, 13], np.int64)
    boxes[4], labels[4] = boxes[0], labels[0]                   # the same image twice in the batch
    alone = _device_plan(boxes[:1], labels[:1], ids[:1], H, W)
    batch = _device_plan(boxes, labels, ids, H, W)
    perm = np.array([6, 5, 0, 3, 2, 1, 4])
    moved = _device_plan(boxes[perm], labels[perm], ids[perm], H, W)
    for n in pc.NAMES:
        np.testing.assert_array_equal(batch[n][0], alone[n][0])
        np.testing.assert_array_equal(batch[n][4], alone[n][0])
        np.testing.assert_array_equal(moved[n], batch[n][perm])
    other = _device_plan(boxes[:1], labels[:1], ids[:1], H, W, seed=pc.SEED + 1)
    assert any(not np.array_equal(other[n], alone[n]) for n in pc.NAMES)      # the seed matters


def test_in_place_call_and_preallocated_outputs():
    import torch
    import augmentation as aug
    import ssd_hip as h
    H, W, boxes, labels, ids, ref = _bit_case("300x300_G5_B70")
    B, G = boxes.shape[:2]
    dev = h.device()
    g = torch.as_tensor(boxes).to(dev)
    gl, di = torch.as_tensor(labels).to(dev), torch.as_tensor(ids).to(dev)
    out = [torch.empty(s, dtype=d, device=dev) for s, d in (((B, 10), torch.int32), ((B, 4), torch.float32), ((B,), torch.int32),
                                                            ((B,), torch.float32), ((B, 4), torch.int32))]
    h.check(h.lib().ssd_augment_plan(h.ptr(g), h.ptr(gl), h.ptr(di), B, G, H, W, pc.SEED, *[h.ptr(t) for t in out], h.ptr(g),
                                     h.stream()), "ssd_augment_plan")
    _assert_bit_equal({n: t.cpu().numpy() for n, t in zip(pc.NAMES, out + [g])}, ref, "in place")
    # out=: the tensors handed in are the ones written and returned
    out.append(torch.empty((B, G, 4), dtype=torch.float32, device=dev))
    back = aug.plan_batch_device(boxes, labels, ids, H, W, pc.SEED, out=tuple(out))
    assert all(a is b for a, b in zip(back, out))
    _assert_bit_equal({n: t.cpu().numpy() for n, t in zip(pc.NAMES, out)}, ref, "out=")
    with pytest.raises(ValueError):
        aug.plan_batch_device(boxes, labels, ids, H, W, pc.SEED, out=tuple(out[:5]) + (out[5][:, :1],))


@pytest.mark.parametrize("shape", [(3, 24, 40), (3, 300, 300)])
def test_apply_batch_device_same_pixels_as_run_plans(shape):
    """The device plan read back and handed to the existing ``run_plans`` gives the images of ``apply_batch_device`` bit
    for bit (an image with neither crop nor flip goes through the geometry kernel's copy path there, ``clone()`` here)."""
    import torch
    import augmentation as aug
    B, H, W = shape
    imgs = np.random.default_rng(H).random((B, H, W, 3), dtype=np.float32)
    boxes, labels = pc.ground_truth(B, 5, seed=61)
    # consecutive ids chosen with the restatement: between them a crop out of an expanded canvas, a flip, an image with
    # neither (the copy path) and every colour operation
    ids = np.arange(1004, 1007, dtype=np.int64) if H == 300 else np.arange((1 << 32) + 2, (1 << 32) + 5, dtype=np.int64)
    ref = pc.plan_batch(pc.SEED, ids, H, W, boxes, labels)
    q = ref["geom"]
    assert (ref["info"][:, 2] == 1).any() and (q[:, 8] == 1).any() and ((q[:, 8] == 0) & (q[:, 9] == 0)).any()
    assert np.bitwise_or.reduce(ref["flags"]) == 15
    out, gb = aug.apply_batch_device(imgs, boxes, labels, ids, seed=pc.SEED)
    assert isinstance(gb, torch.Tensor) and gb.is_cuda and tuple(out.shape) == (B, H, W, 3)
    np.testing.assert_array_equal(gb.cpu().numpy().view(np.uint32), ref["boxes"].view(np.uint32))
    plan = _device_plan(boxes, labels, ids, H, W)
    _assert_bit_equal(plan, ref, "plan")
    want = aug.run_plans(imgs, pc.host_plans(plan))
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and o.min() >= 0.0 and o.max() <= 1.0
    # device_draws: the augmentation_fn signature, consecutive ids from the offset on
    fn = aug.device_draws(pc.SEED, rank_offset=int(ids[0]))
    o2, g2 = fn(torch.as_tensor(imgs[:1]), boxes[:1], labels[:1])
    assert torch.equal(o2.view(torch.int32), out[:1].view(torch.int32)) and torch.equal(g2, gb[:1])
    o3, _ = fn(torch.as_tensor(imgs[1:2]), boxes[1:2], labels[1:2])
    assert torch.equal(o3.view(torch.int32), out[1:2].view(torch.int32))


def test_device_boxes_reach_target_assignment_without_a_copy_back():
    """``apply_batch_device``'s boxes are a device tensor; ``calculate_actual_outputs`` (``ssd_match_encode``'s wrapper) and
    ``augmented`` take them as they are and give what the same boxes give from the host."""
    import torch
    import augmentation as aug
    from utils import bbox_utils, train_utils
    hp = train_utils.get_hyper_params("mobilenet_v2")
    hp["total_labels"] = 21
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    B, S = 3, 32
    imgs = np.random.default_rng(1).random((B, S, S, 3), dtype=np.float32)
    boxes, labels = pc.ground_truth(B, 5, seed=71)
    stream = aug.augmented([(imgs, boxes, labels)], aug.device_draws(pc.SEED, rank_offset=1 << 40))
    (im, gb, gl), = list(stream)
    assert isinstance(gb, torch.Tensor) and gb.is_cuda and gl is labels
    a = train_utils.calculate_actual_outputs(priors, gb, gl, hp)
    b = train_utils.calculate_actual_outputs(priors, gb.cpu().numpy(), gl, hp)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_launch_nothing():
    import torch
    import augmentation as aug
    import ssd_hip as h
    for G, H, msg in ((513, 300, "513"), (5, h.MAX_IMAGE_SIDE, str(h.MAX_IMAGE_SIDE))):
        boxes, labels = np.zeros((2, G, 4), F32), np.full((2, G), -1, np.int32)
        out = [torch.full(s, 7, dtype=d, device=h.device()) for s, d in (
            ((2, 10), torch.int32), ((2, 4), torch.float32), ((2,), torch.int32), ((2,), torch.float32), ((2, 4), torch.int32),
            ((2, G, 4), torch.float32))]
        with pytest.raises(h.SsdHipUnsupported) as e:
            aug.plan_batch_device(boxes, labels, np.array([0, 1]), H, 300, 1, out=tuple(out))
        assert "ssd_augment_plan" in str(e.value) and msg in str(e.value)
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in out)                       # nothing was written
    rc = h.lib().ssd_augment_plan(None, None, None, 2, 513, 300, 300, 0, None, None, None, None, None, None, h.stream())
    assert rc == -3 and b"513" in h.lib().ssd_last_error()


def test_trainer_runs_with_device_draws(tmp_path, monkeypatch):
    """``SSD_TRAINER_AUGMENT=gpu``: the training stream passes through ``device_draws`` (device boxes into the target
    assignment) and the step stays finite."""
    import importlib
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_TRAINER_EPOCHS", "1")
    monkeypatch.setenv("SSD_TRAINER_STEPS", "2")
    monkeypatch.setenv("SSD_TRAINER_BATCH", "4")
    monkeypatch.setenv("SSD_TRAINER_AUGMENT", "gpu")
    import augmentation as aug
    calls = []
    real = aug.device_draws
    monkeypatch.setattr(aug, "device_draws", lambda seed, rank_offset=0: calls.append((seed, rank_offset)) or real(seed, rank_offset))
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    assert calls == [(4242, 0)]
    assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
