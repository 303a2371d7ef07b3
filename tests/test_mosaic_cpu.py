"""Mosaic augmentation without a GPU: the cases of tests/mosaic_cases.py hold what they are for (asserted on the NumPy
restatement alone), invariants of that restatement, ``trainer.mosaic_from_env`` and the argument checks of
``augmentation.mosaicked`` (both raise before anything touches a device)."""
import numpy as np
import pytest

import mosaic_cases as mc

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the cases' coverage
def test_cases_hold_what_they_are_for():
    cov = mc.coverage()
    assert len(cov) == 18
    missing = [name for name, ok in cov.items() if not ok]
    assert not missing, missing


def test_self_partner_image_is_the_searched_one():
    plan = mc.reference("SMALL")["plan"]
    b = mc.SELF_PARTNER_IMAGE
    assert b in plan[b, 7::3] and mc.SMALL_IDS[b] == 1000003 * mc.SELF_PARTNER_K + 7


def test_stride_case_is_longer_than_one_trip_of_the_grid():
    c = mc.case("STRIDE")
    assert c.images.shape[0] * c.H * c.W > mc.bc.ONE_TRIP


# ------------------------------------------------------------------------------------------ the restatement's invariants
@pytest.mark.parametrize("name", ["SMALL", "SMALL_UP", "CAP"])
def test_kept_boxes_lie_inside_their_tile(name):
    c, ref = mc.case(name), mc.reference(name)
    written = [r for r in ref["rows"] if r.written]
    assert written
    at = {}
    for r in written:
        k = at.get(r.image, 0)
        at[r.image] = k + 1
        y1, x1, y2, x2 = ref["boxes"][r.image, k]
        _, (y_lo, y_hi, x_lo, x_hi) = mc.placement([int(v) for v in ref["plan"][r.image]], r.tile, c.H, c.W)
        assert F32(y_lo) / F32(c.H) <= y1 < y2 <= F32(y_hi) / F32(c.H) and F32(x_lo) / F32(c.W) <= x1 < x2 <= F32(x_hi) / F32(c.W)
        assert ref["labels"][r.image, k] == c.labels[r.source, r.row] > 0
    for b in range(c.images.shape[0]):          # and nothing but padding behind them
        n = ref["info"][b, 2]
        assert n == at.get(b, 0) == min(ref["info"][b, 1], mc.rows_out(c))
        assert not ref["boxes"][b, n:].any() and (ref["labels"][b, n:] == mc.PAD_LABEL).all()


def test_p_zero_returns_the_input_padded():
    c = mc.case("SMALL")
    B, G = c.labels.shape
    out = mc.mosaic_batch(mc.SEED, c.ids, c.boxes, c.labels, c.H, c.W, 0.0, c.scale, 4 * G, c.images)
    assert not out["plan"][:, 0].any() and not out["rows"]
    np.testing.assert_array_equal(out["pixels"], c.images)
    np.testing.assert_array_equal(out["boxes"][:, :G], c.boxes)
    np.testing.assert_array_equal(out["labels"][:, :G], c.labels)          # valid or not: as they are
    assert not out["boxes"][:, G:].any() and (out["labels"][:, G:] == mc.PAD_LABEL).all()
    np.testing.assert_array_equal(out["info"], np.tile(np.array([0, 0, G, 0], np.int32), (B, 1)))
    # every other value of the plan is what p = 1 draws: slots are never conditional
    np.testing.assert_array_equal(out["plan"][:, 1:], mc.reference("SMALL")["plan"][:, 1:])


def test_plan_of_an_image_ignores_the_other_images_ids():
    c = mc.case("SMALL")
    ids = c.ids.copy()
    ids[3] += 12345
    a = mc.reference("SMALL")
    b = mc.mosaic_batch(mc.SEED, ids, c.boxes, c.labels, c.H, c.W, c.p, c.scale, mc.rows_out(c))
    keep = np.arange(len(ids)) != 3
    for n in mc.NAMES:
        np.testing.assert_array_equal(a[n][keep], b[n][keep])
    assert not np.array_equal(a["plan"][3], b["plan"][3])


def test_sources_and_sizes_stay_in_range():
    for name in ("SMALL", "SMALL_HALF", "SMALL_UP"):
        c, plan = mc.case(name), mc.reference(name)["plan"]
        assert ((plan[:, 4::3] >= 0) & (plan[:, 4::3] < c.images.shape[0])).all()
        assert (plan[:, 4] == np.arange(c.images.shape[0])).all()
        assert ((plan[:, 1] >= 1) & (plan[:, 1] <= c.H - 1) & (plan[:, 2] >= 1) & (plan[:, 2] <= c.W - 1)).all()
        assert (plan[:, 5::3] >= np.rint(F32(c.H) * F32(c.scale[0]))).all() and (plan[:, 5::3] <= np.rint(F32(c.H) * F32(c.scale[1]))).all()


# ------------------------------------------------------------------------------------------------------ the trainer's knobs
@pytest.fixture
def trainer(monkeypatch):
    import importlib
    for k in ("SSD_TRAINER_MOSAIC", "SSD_TRAINER_MOSAIC_SCALE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SSD_TRAINER_AUGMENT", "gpu")        # what mosaic needs; the host draws are refused below
    return importlib.import_module("trainer")


@pytest.mark.parametrize("value", [None, "", " ", "0", "0.0"])
def test_mosaic_from_env_off(trainer, monkeypatch, value):
    if value is not None:
        monkeypatch.setenv("SSD_TRAINER_MOSAIC", value)
    assert trainer.mosaic_from_env() is None


@pytest.mark.parametrize("value, scale, want", [("1", None, (1.0, (0.5, 1.0))), ("0.5", "", (0.5, (0.5, 1.0))),
                                                 (" 0.25 ", "0.75, 1.5", (0.25, (0.75, 1.5))), ("1.0", "0.1,2", (1.0, (0.1, 2.0))),
                                                 ("1e-3", "1,1", (0.001, (1.0, 1.0)))])
def test_mosaic_from_env_accepts(trainer, monkeypatch, value, scale, want):
    monkeypatch.setenv("SSD_TRAINER_MOSAIC", value)
    if scale is not None:
        monkeypatch.setenv("SSD_TRAINER_MOSAIC_SCALE", scale)
    assert trainer.mosaic_from_env() == want


@pytest.mark.parametrize("value, scale, msg", [
    ("yes", None, "SSD_TRAINER_MOSAIC must"), ("-0.1", None, "SSD_TRAINER_MOSAIC must"), ("1.5", None, "SSD_TRAINER_MOSAIC must"),
    ("nan", None, "SSD_TRAINER_MOSAIC must"),
    ("1", "0.5", "SSD_TRAINER_MOSAIC_SCALE must"), ("1", "0.5,1,2", "SSD_TRAINER_MOSAIC_SCALE must"), ("1", "a,b", "SSD_TRAINER_MOSAIC_SCALE must"),
    ("1", "0.05,1", "SSD_TRAINER_MOSAIC_SCALE must"), ("1", "1,0.5", "SSD_TRAINER_MOSAIC_SCALE must"), ("1", "0.5,2.5", "SSD_TRAINER_MOSAIC_SCALE must"),
    ("1", "nan,1", "SSD_TRAINER_MOSAIC_SCALE must"),
    (None, "0.5,1", "SSD_TRAINER_MOSAIC is not"), ("0", "0.5,1", "SSD_TRAINER_MOSAIC is not")])
def test_mosaic_from_env_refuses(trainer, monkeypatch, value, scale, msg):
    if value is not None:
        monkeypatch.setenv("SSD_TRAINER_MOSAIC", value)
    if scale is not None:
        monkeypatch.setenv("SSD_TRAINER_MOSAIC_SCALE", scale)
    with pytest.raises(ValueError) as e:
        trainer.mosaic_from_env()
    assert msg in str(e.value)


@pytest.mark.parametrize("augment", [None, "1", "host", ""])
def test_mosaic_from_env_refuses_the_host_draws(trainer, monkeypatch, augment):
    """A mosaic may keep no row, and ``apply_batch``'s sampler raises on an image without one: refused at start-up, not at a
    random step.  Without mosaic the host draws stay what they were."""
    if augment is None:
        monkeypatch.delenv("SSD_TRAINER_AUGMENT")
    else:
        monkeypatch.setenv("SSD_TRAINER_AUGMENT", augment)
    assert trainer.mosaic_from_env() is None
    monkeypatch.setenv("SSD_TRAINER_MOSAIC", "0.5")
    with pytest.raises(ValueError) as e:
        trainer.mosaic_from_env()
    assert "SSD_TRAINER_AUGMENT=gpu" in str(e.value)
    monkeypatch.setenv("SSD_TRAINER_AUGMENT", "0")
    assert trainer.mosaic_from_env() == (0.5, (0.5, 1.0))


def test_a_mosaic_can_keep_no_row_and_the_host_sampler_refuses_such_an_image():
    """The reason for the refusal above, on the restatement and the host draws alone."""
    import augmentation as aug
    images, boxes, labels = mc.empty_mosaic_batch()
    B, S = images.shape[0], images.shape[1]
    out = mc.mosaic_batch(mc.SEED, np.arange(B), boxes, labels, S, S, 1.0, (0.5, 1.0), 4)
    assert (out["info"][:, 0] == 1).all() and (out["info"][:, 2] == 0).all() and (out["info"][:, 3] == 4).all()
    assert (out["labels"] == mc.PAD_LABEL).all() and not out["boxes"].any()
    with pytest.raises(ValueError) as e:
        aug.sample_distorted_bounding_box(S, S, out["boxes"][0][out["labels"][0] > 0], 0.1)
    assert "no bounding boxes" in str(e.value)


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def wrap(self, name):
        def fn(*a, **k):
            self.calls.append((name, a, k))
            return (name, len(self.calls))
        return fn


class _Shuffled(object):
    def shuffle(self, n, seed=None):
        return ("shuffled", n, seed)


@pytest.mark.parametrize("augment, augment_gpu", [(True, True), (False, False)])
def test_voc_road_wraps_resize_then_mosaic_then_augmentation(trainer, monkeypatch, augment, augment_gpu):
    """``voc_training_batches`` with mosaic: ``voc_batches`` without an augmentation_fn, ``mosaicked`` around it with the
    knob's values and the rank's id range, ``augmented`` with the device draws around that (not with augmentation off)."""
    import augmentation as aug
    from utils import data_utils
    rec = _Recorder()
    monkeypatch.setattr(data_utils, "voc_batches", rec.wrap("voc_batches"))
    monkeypatch.setattr(aug, "mosaicked", rec.wrap("mosaicked"))
    monkeypatch.setattr(aug, "augmented", rec.wrap("augmented"))
    monkeypatch.setattr(aug, "device_draws", lambda seed, rank_offset=0: ("device_draws", seed, rank_offset))
    got = trainer.voc_training_batches(_Shuffled(), 8, 300, 3, augment, augment_gpu, (0.25, (0.75, 1.5)))
    want = [("voc_batches", (("shuffled", 32, 3), 8, 300, 300), {"augmentation_fn": None}),
            ("mosaicked", (("voc_batches", 1), 0.25, 4242), {"rank_offset": 3 << 40, "scale": (0.75, 1.5)})]
    if augment:
        want.append(("augmented", (("mosaicked", 2), ("device_draws", 4242, 3 << 40)), {}))
    assert rec.calls == want and got == (want[-1][0], len(want))


@pytest.mark.parametrize("augment, augment_gpu", [(True, True), (True, False), (False, False)])
def test_voc_road_without_mosaic_is_one_voc_batches_call(trainer, monkeypatch, augment, augment_gpu):
    """No knob: the augmentation runs inside ``voc_batches`` as before, and neither wrapper is built."""
    import augmentation as aug
    from utils import data_utils
    rec = _Recorder()
    monkeypatch.setattr(data_utils, "voc_batches", rec.wrap("voc_batches"))
    monkeypatch.setattr(aug, "mosaicked", rec.wrap("mosaicked"))
    monkeypatch.setattr(aug, "augmented", rec.wrap("augmented"))
    monkeypatch.setattr(aug, "device_draws", lambda seed, rank_offset=0: ("device_draws", seed, rank_offset))
    monkeypatch.setattr(aug, "seed", lambda s: rec.calls.append(("seed", (s,), {})))
    got = trainer.voc_training_batches(_Shuffled(), 8, 300, 1, augment, augment_gpu, None)
    fn = None if not augment else (("device_draws", 4242, 1 << 40) if augment_gpu else aug.apply_batch)
    want = ([("seed", (4243,), {})] if augment and not augment_gpu else []) + [
        ("voc_batches", (("shuffled", 32, 1), 8, 300, 300), {"augmentation_fn": fn})]
    assert rec.calls == want and got == ("voc_batches", len(want))


# -------------------------------------------------------------------------------------------------- mosaicked's arguments
@pytest.mark.parametrize("p, scale", [(-0.1, (0.5, 1.0)), (1.01, (0.5, 1.0)), (float("nan"), (0.5, 1.0)), ("x", (0.5, 1.0)),
                                       (1.0, (0.05, 1.0)), (1.0, (1.0, 0.5)), (1.0, (0.5, 2.5)), (1.0, (0.5,)), (1.0, 0.5),
                                       (1.0, (float("nan"), 1.0))])
def test_mosaicked_refuses_bad_arguments_at_construction(p, scale):
    import augmentation as aug
    with pytest.raises(ValueError) as e:
        aug.mosaicked([], p, 1, scale=scale)
    assert "mosaic" in str(e.value)


def test_mosaicked_is_lazy_and_restartable():
    """Nothing runs until a batch is asked for: an empty dataset passes through on a machine without a GPU."""
    import augmentation as aug
    stream = aug.mosaicked([], 0.5, 7, rank_offset=1 << 40, scale=(0.75, 1.5), max_boxes=12)
    assert list(stream) == [] and list(stream) == []


def test_library_exports_the_mosaic_entries():
    import ssd_hip
    lib = ssd_hip.lib()
    assert lib.ssd_augment_mosaic_plan is not None and lib.ssd_augment_mosaic_pixels is not None
    # the refusals that come before anything touches a device
    assert lib.ssd_augment_mosaic_plan(None, None, None, 2, 513, 300, 300, 0, 1.0, 0.5, 1.0, 2048, -1, None, None, None, None, None) == -3
    assert b"513" in lib.ssd_last_error()
    assert lib.ssd_augment_mosaic_plan(None, None, None, 2, 6, 300, 300, 0, 1.5, 0.5, 1.0, 24, -1, None, None, None, None, None) == -1
    assert lib.ssd_augment_mosaic_pixels(None, 2, 4097, 300, None, None, None, None) == -3
