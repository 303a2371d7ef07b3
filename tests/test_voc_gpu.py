"""The batched VOC ingest on the device: ``ssd_preprocess_ragged`` / ``data_utils.preprocess_ragged_batch`` against the
oracle (``bbox_oracle.preprocess_image``) and against the per-image ``data_utils.preprocessing``; ``voc_batches`` against
``padded_batch(preprocessing(...))``; the two entry points on a tiny devkit written at test time (tests/voc_cases.py).
Bit-exactness is the bar: no tolerance anywhere."""
import importlib

import numpy as np
import pytest
import torch

import eval_cases as ec
import ssd_hip
import voc_cases as vc
from oracle import bbox_oracle as bo
from utils import data_utils

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL")

OUT_SIZES = [(300, 300), (512, 512), (299, 301)]       # the last: odd row length, image slots not 16-byte aligned


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def devkit(tmp_path_factory):
    root = tmp_path_factory.mktemp("voc")
    vc.write_devkit(root, with_2012=True)
    return root


@pytest.fixture(scope="module")
def images(devkit):
    return vc.all_decoded_2007(devkit)


def _alone(img, oh, ow):
    return _np(data_utils.preprocessing({"image": img, "objects": {"bbox": np.zeros((0, 4)), "label": np.zeros((0,), np.int64),
                                                                   "is_difficult": np.zeros((0,), bool)}}, oh, ow)[0])


@pytest.mark.parametrize("out", OUT_SIZES, ids=lambda o: "%dx%d" % o)
def test_ragged_batch_equals_the_oracle_and_the_per_image_path(images, out):
    oh, ow = out
    assert len({im.shape for im in images}) == len(images) == 10
    got = _np(data_utils.preprocess_ragged_batch(images, oh, ow))
    assert got.dtype == np.float32 and got.shape == (len(images), oh, ow, 3)
    for b, im in enumerate(images):
        want = bo.preprocess_image(im, oh, ow)
        assert np.array_equal(_bits(got[b]), _bits(want)), "image %d %s -> %dx%d: %d values differ from the oracle" % (
            b, im.shape, oh, ow, int((_bits(got[b]) != _bits(want)).sum()))
        assert np.array_equal(_bits(got[b]), _bits(_alone(im, oh, ow))), "image %d differs from preprocessing() alone" % b
    again = _np(data_utils.preprocess_ragged_batch(images, oh, ow))
    assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("n", [1, 33])
def test_batches_of_1_and_33(images, n):
    rng = np.random.default_rng(n)
    batch = [images[i % len(images)] for i in range(n - 1)] + [rng.integers(0, 256, (47, 91, 3), dtype=np.uint8)]
    got = _np(data_utils.preprocess_ragged_batch(batch, 300, 300))
    assert got.shape == (n, 300, 300, 3)
    for b, im in enumerate(batch):
        assert np.array_equal(_bits(got[b]), _bits(bo.preprocess_image(im, 300, 300))), b


def test_out_view_into_a_larger_batch_and_tensor_inputs(images):
    dev = ssd_hip.device()
    part = images[:4]
    big = torch.full((len(part) + 3, 64, 48, 3), -7.0, dtype=torch.float32, device=dev)
    got = data_utils.preprocess_ragged_batch([torch.as_tensor(im) for im in part], 64, 48, out=big[2:2 + len(part)])
    assert got.data_ptr() == big[2].data_ptr()
    big = _np(big)
    for b, im in enumerate(part):
        assert np.array_equal(_bits(big[2 + b]), _bits(bo.preprocess_image(im, 64, 48)))
    assert (big[:2] == -7.0).all() and (big[2 + len(part):] == -7.0).all()      # the neighbours' slots are untouched
    with pytest.raises(ValueError):
        data_utils.preprocess_ragged_batch(part[:1], 64, 48, out=torch.empty((1, 64, 49, 3), device=dev))
    # a non-contiguous view of a larger image is packed as the view's pixels
    view = images[0][10:200:2, 5:300:3]
    assert np.array_equal(_bits(_np(data_utils.preprocess_ragged_batch([view], 300, 300))[0]),
                          _bits(bo.preprocess_image(np.ascontiguousarray(view), 300, 300)))


def test_empty_batch_and_unsupported_shapes_leave_the_output_alone():
    lib = ssd_hip.lib()
    dev = ssd_hip.device()
    out = data_utils.preprocess_ragged_batch([], 20, 20)
    assert tuple(out.shape) == (0, 20, 20, 3)
    sentinel = torch.full((1, 20, 20, 3), 3.0, dtype=torch.float32, device=dev)
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    for C, H, W, oh, ow, off, nbytes, want in [(4, 8, 8, 20, 20, 0, 4096, -3), (3, 0, 8, 20, 20, 0, 4096, -3),
                                               (3, 8, 8, 20, 16385, 0, 4096, -3), (3, 16385, 1, 20, 20, 0, 1 << 20, -3),
                                               (3, 8, 8, 20, 20, 8, 4096, -1), (3, 40, 40, 20, 20, 0, 4096, -1)]:
        desc = np.zeros(1, ssd_hip.IMAGE_DESC_DTYPE)
        desc[0] = (off, H, W)
        ddev = torch.as_tensor(desc.view(np.uint8)).to(dev)
        rc = lib.ssd_preprocess_ragged(ssd_hip.ptr(src), nbytes, desc.ctypes.data, ssd_hip.ptr(ddev), 1, C, oh, ow,
                                       ssd_hip.ptr(sentinel), ssd_hip.stream())
        assert rc == want, (C, H, W, oh, ow, off, rc, lib.ssd_last_error())
    torch.cuda.synchronize()
    assert (_np(sentinel) == 3.0).all()
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        data_utils.preprocess_ragged_batch([np.zeros((8, 8, 4), np.uint8)], 20, 20)
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        data_utils.preprocess_ragged_batch([np.zeros((0, 8, 3), np.uint8)], 20, 20)


@pytest.mark.parametrize("evaluate", [False, True], ids=["train", "evaluate"])
@pytest.mark.parametrize("workers", [1, 4])
def test_voc_batches_equal_padded_batch_of_preprocessing(devkit, evaluate, workers):
    a, _ = data_utils.get_dataset("voc/2007", "train+validation", str(devkit))
    b, _ = data_utils.get_dataset("voc/2007", "test", str(devkit))
    ds = a.concatenate(b)                                                       # all 10 images
    ref = list(data_utils.padded_batch((data_utils.preprocessing(item, 300, 300, evaluate=evaluate) for item in ds), 4))
    batches = data_utils.voc_batches(ds, 4, 300, 300, evaluate=evaluate, workers=workers, prefetch=2)
    for _pass in range(2):                                                      # re-iterable: every pass is the dataset again
        got = list(batches)
        assert [len(x[0]) for x in got] == [4, 4, 2] == [len(x[0]) for x in ref]
        for (x, gt, gl), (rx, rgt, rgl) in zip(got, ref):
            assert x.device == rx.device and x.dtype == torch.float32
            assert np.array_equal(_bits(_np(x)), _bits(_np(rx)))
            assert gt.dtype == rgt.dtype == np.float32 and gl.dtype == rgl.dtype == np.int32
            assert gt.shape == rgt.shape and np.array_equal(_bits(gt), _bits(rgt)) and np.array_equal(gl, rgl)
    if evaluate:                                                                # difficult objects are gone, G >= 1 stays
        assert got[2][1].shape[1] >= 1 and (got[2][2][1] == -1).all()          # 000006: its only object is difficult
    # decoded items (any iterable of tfds-shaped dicts) take the same road
    items = list(ds)
    again = list(data_utils.voc_batches(items, 4, 300, 300, evaluate=evaluate, workers=workers))
    for (x, gt, gl), (rx, rgt, rgl) in zip(again, ref):
        assert np.array_equal(_bits(_np(x)), _bits(_np(rx))) and np.array_equal(gt, rgt) and np.array_equal(gl, rgl)


def test_voc_batches_augmentation_runs_after_the_resize(devkit):
    import augmentation
    ds, _ = data_utils.get_dataset("voc/2007", "train", str(devkit))
    plain = list(data_utils.voc_batches(ds, 4, 300, 300))[0]
    augmentation.seed(11)
    want_x, want_gt = augmentation.apply_batch(plain[0], plain[1], plain[2])
    augmentation.seed(11)
    x, gt, gl = list(data_utils.voc_batches(ds, 4, 300, 300, augmentation_fn=augmentation.apply_batch))[0]
    assert np.array_equal(_bits(_np(x)), _bits(_np(want_x))) and np.array_equal(gt, want_gt) and np.array_equal(gl, plain[2])


def test_predictor_evaluates_the_voc_test_split(devkit, tmp_path, monkeypatch, capsys):
    """``predictor.main(evaluate=True)`` with ``SSD_VOC_DIR``: the stats of the same items fed through the per-image
    path (``preprocessing`` + ``padded_batch``) into the same model."""
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    from utils import bbox_utils, eval_utils, train_utils
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_VOC_DIR", str(devkit))
    monkeypatch.delenv("SSD_SYNTHETIC_ITEMS", raising=False)
    predictor = importlib.import_module("predictor")
    b, l, s, stats = predictor.main(["--backbone", "mobilenet_v2"], evaluate=True, batch_size=2)
    assert b.shape == (3, 200, 4) and "predicted 3 images" in capsys.readouterr().out
    ds, info = data_utils.get_dataset("voc/2007", "test", str(devkit))
    labels = ["bg"] + data_utils.get_labels(info)
    hp = train_utils.get_hyper_params("mobilenet_v2")
    hp["total_labels"] = len(labels)
    ref_data = list(data_utils.padded_batch((data_utils.preprocessing(item, 300, 300, evaluate=True) for item in ds), 2))
    m = get_model(hp, max_batch=2)
    data_utils.synthetic_weights(m)
    pri = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    rb, rl, rs = get_decoder_model(m, pri, hp).predict(ref_data, steps=2)
    np.testing.assert_array_equal(l, rl)
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(b, rb)
    ref = eval_utils.evaluate_predictions(ref_data, rb, rl, rs, labels, 2)
    ec.assert_stats_equal(stats, ref)
    assert sum(int(v["total"]) for v in stats.values()) == 3                    # 5 objects in the split, 2 of them difficult
    # SSD_SYNTHETIC_ITEMS caps the run in this mode too
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "2")
    b2, _, _ = predictor.main(["--backbone", "mobilenet_v2"], batch_size=2)
    assert b2.shape == (2, 200, 4)
    np.testing.assert_array_equal(b2, b[:2])


def test_trainer_runs_on_the_voc_splits(devkit, tmp_path, monkeypatch, capsys):
    """``trainer.main`` with ``SSD_VOC_DIR``: train+validation of 2007 and 2012 (10 images), shuffled, augmented, two
    steps of batch 4 and the capped validation, to a finite loss."""
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_VOC_DIR", str(devkit))
    monkeypatch.setenv("SSD_TRAINER_EPOCHS", "1")
    monkeypatch.setenv("SSD_TRAINER_STEPS", "2")
    monkeypatch.setenv("SSD_TRAINER_BATCH", "4")
    monkeypatch.setenv("SSD_TRAINER_ITEMS", "8")
    monkeypatch.setenv("SSD_DATA_WORKERS", "2")
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "Epoch 1/1" in out and "val_loss" in out
    assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
    assert hist["loss"][0] > 0 and hist["val_loss"][0] > 0
