"""Custom images on the device: ``ssd_resize_lanczos`` / ``data_utils.resize_lanczos_batch`` against Pillow itself --
the committed fixture (tests/golden/lanczos.npz, written by ``Image.resize(..., Image.LANCZOS)``), the NumPy integer
two-pass the CPU tests hold to that fixture, and Pillow run here when PIL imports.  Equality everywhere: uint8 output
== Pillow's bytes, float output bitwise == ``preprocess_batch`` of those bytes."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import lanczos_cases as lc
import ssd_hip
from utils import data_utils

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _resize(images, oh, ow):
    u8 = torch.empty((len(images), oh, ow, 3), dtype=torch.uint8, device=ssd_hip.device())
    return data_utils.resize_lanczos_batch(images, oh, ow, out_u8=u8), u8


def _assert_bits(images, oh, ow, wants, what):
    f, u8 = _resize(images, oh, ow)
    f, u8 = _np(f), _np(u8)
    assert f.dtype == np.float32 and f.shape == (len(images), oh, ow, 3)
    for b, want in enumerate(wants):
        assert np.array_equal(u8[b], want), "%s: image %d (%s -> %dx%d): %d bytes differ from Pillow" % (
            what, b, images[b].shape[:2], oh, ow, int((u8[b] != want).sum()))
    ref = _np(data_utils.preprocess_batch(np.stack(wants), oh, ow))
    assert np.array_equal(f.view(np.uint32), ref.view(np.uint32)), "%s: float output differs from preprocess_batch(pillow)" % what
    return f, u8


@pytest.mark.parametrize("out", lc.FIXTURE_OUT, ids=lambda o: "%dx%d" % o)
def test_ragged_batch_equals_the_pillow_fixture(out):
    cases, version = lc.load_fixture()
    keys = [k for k in cases if k[1:] == out]
    assert len(keys) == len(lc.FIXTURE_SOURCES)
    _assert_bits([cases[k][0] for k in keys], out[0], out[1], [cases[k][1] for k in keys], "fixture (Pillow %s)" % version)


@pytest.mark.parametrize("out", lc.GPU_OUT, ids=lambda o: "%dx%d" % o)
def test_ragged_batch_of_real_sizes_equals_pillow(out):
    """375x500 ... 2000x3000 in ONE call, all three contents; against the integer two-pass always and against live
    Pillow when PIL imports; twice, with identical bits."""
    oh, ow = out
    images = [lc.image(h, w, lc.CONTENTS[i % 3], seed=i) for i, (h, w) in enumerate(lc.GPU_SIZES)]
    wants = [lc.two_pass(im, oh, ow) for im in images]
    if lc.pillow_available():
        for im, want in zip(images, wants):
            assert np.array_equal(lc.pillow(im, oh, ow), want)
    f0, u0 = _assert_bits(images, oh, ow, wants, "two-pass / live Pillow")
    f1, u1 = _resize(images, oh, ow)
    assert np.array_equal(_np(f1).view(np.uint32), f0.view(np.uint32)) and np.array_equal(_np(u1), u0)


def test_every_content_at_every_size():
    """The contents rotate through the sizes: every (size, content) pair of the list, to 300x300."""
    for shift in (1, 2):
        images = [lc.image(h, w, lc.CONTENTS[(i + shift) % 3], seed=7) for i, (h, w) in enumerate(lc.GPU_SIZES)]
        wants = [lc.pillow(im, 300, 300) if lc.pillow_available() else lc.two_pass(im, 300, 300) for im in images]
        _assert_bits(images, 300, 300, wants, "contents shift %d" % shift)


def test_out_view_into_a_larger_batch_and_tensor_inputs():
    cases, _ = lc.load_fixture()
    keys = [k for k in cases if k[1:] == (20, 20)]
    dev = ssd_hip.device()
    big = torch.full((len(keys) + 3, 20, 20, 3), -7.0, dtype=torch.float32, device=dev)
    got = data_utils.resize_lanczos_batch([torch.as_tensor(cases[k][0]) for k in keys], 20, 20, out=big[2:2 + len(keys)])
    assert got.data_ptr() == big[2].data_ptr()
    want = np.stack([cases[k][1] for k in keys]).astype(np.float32) * np.float32(1.0 / 255.0)
    big = _np(big)
    assert np.array_equal(big[2:2 + len(keys)], want)
    assert (big[:2] == -7.0).all() and (big[2 + len(keys):] == -7.0).all()      # the neighbours' slots are untouched
    with pytest.raises(ValueError):
        data_utils.resize_lanczos_batch([cases[keys[0]][0]], 20, 20, out=torch.empty((1, 20, 21, 3), device=dev))


def test_empty_batch_and_unsupported_shapes():
    lib = ssd_hip.lib()
    dev = ssd_hip.device()
    out = data_utils.resize_lanczos_batch([], 20, 20)
    assert tuple(out.shape) == (0, 20, 20, 3)
    assert lib.ssd_resize_lanczos(None, 0, None, 0, None, None, 0, 3, 20, 20, None, None, None, 0, ssd_hip.stream()) == 0
    # C = 4 and a 0-sized side: SSD_E_UNSUPPORTED (-3) before any launch, the output is left alone
    sentinel = torch.full((1, 20, 20, 3), 3.0, dtype=torch.float32, device=dev)
    src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    tables = torch.zeros(4096, dtype=torch.int32, device=dev)
    for C, H, W, oh, ow in [(4, 8, 8, 20, 20), (3, 0, 8, 20, 20), (3, 8, 0, 20, 20), (3, 8, 8, 0, 20), (3, 8, 8, 20, 16385),
                            (3, 16385, 1, 20, 20)]:
        desc = np.zeros(1, ssd_hip.RESIZE_DESC_DTYPE)
        desc[0]["H"], desc[0]["W"], desc[0]["h_ksize"], desc[0]["v_ksize"] = H, W, 7, 7
        ddev = torch.as_tensor(desc.view(np.uint8)).to(dev)
        ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        rc = lib.ssd_resize_lanczos(ssd_hip.ptr(src), 0, ssd_hip.ptr(tables), tables.numel(), desc.ctypes.data,
                                    ssd_hip.ptr(ddev), 1, C, oh, ow, ssd_hip.ptr(sentinel), None, ssd_hip.ptr(ws), ws.numel(),
                                    ssd_hip.stream())
        assert rc == -3, (C, H, W, oh, ow, rc, lib.ssd_last_error())
    torch.cuda.synchronize()
    assert (_np(sentinel) == 3.0).all()
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        data_utils.resize_lanczos_batch([np.zeros((8, 8, 4), np.uint8)], 20, 20)
    with pytest.raises(ssd_hip.SsdHipUnsupported):
        data_utils.resize_lanczos_batch([np.zeros((0, 8, 3), np.uint8)], 20, 20)
    with pytest.raises(ValueError):                                             # a source outside the packed buffer
        desc = np.zeros(1, ssd_hip.RESIZE_DESC_DTYPE)
        desc[0]["H"], desc[0]["W"] = 20, 20
        ssd_hip.check(lib.ssd_resize_lanczos(ssd_hip.ptr(src), 100, ssd_hip.ptr(tables), tables.numel(), desc.ctypes.data,
                                             ssd_hip.ptr(src), 1, 3, 20, 20, ssd_hip.ptr(sentinel), None, None, 0,
                                             ssd_hip.stream()), "bounds")


def _write_folder(d, sizes, seed):
    from PIL import Image
    arrays = []
    for i, (h, w) in enumerate(sizes):
        a = lc.image(h, w, lc.CONTENTS[i % 3], seed=seed)
        name = ("img_%02d.png" if i % 2 else "img_%02d.npy") % i
        if i % 2:
            Image.fromarray(a).save(str(d / name))
        else:
            np.save(str(d / name), a)
        arrays.append((name, a))
    return [a for _, a in sorted(arrays)]


def test_custom_data_batches_equal_the_stacked_generator_items(tmp_path):
    pytest.importorskip("PIL")
    arrays = _write_folder(tmp_path, [(375, 500), (500, 333), (300, 300), (281, 300), (120, 87), (7, 5), (299, 301)], seed=3)
    paths = data_utils.get_custom_imgs(str(tmp_path))
    assert len(paths) == 7
    items = list(data_utils.custom_data_generator(paths, 300, 300))
    for (img, gt, gl), a in zip(items, arrays):
        assert gt.shape == (0, 4) and gl.shape == (0,)
        assert np.array_equal(_np(img), lc.pillow(a, 300, 300).astype(np.float32) * np.float32(1.0 / 255.0))
    batches = list(data_utils.custom_data_batches(paths, 300, 300, 3))
    ref = list(data_utils.padded_batch(iter(items), 3))
    assert [len(b[0]) for b in batches] == [3, 3, 1] == [len(b[0]) for b in ref]
    for (x, gt, gl), (rx, rgt, rgl) in zip(batches, ref):
        assert np.array_equal(_np(x).view(np.uint32), _np(rx).view(np.uint32))
        assert gt.dtype == rgt.dtype and gl.dtype == rgl.dtype
        assert np.array_equal(gt, rgt) and np.array_equal(gl, rgl)


def test_predictor_custom_images_of_mixed_sizes(tmp_path, monkeypatch, capsys):
    """``predictor.main(use_custom_images=True)`` on a folder of mixed-size ``.npy`` / ``.png`` files == the same model
    on arrays Pillow resized on the host."""
    pytest.importorskip("PIL")
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    from utils import bbox_utils, train_utils
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "imgs"
    d.mkdir()
    arrays = _write_folder(d, [(375, 500), (500, 333), (300, 300), (281, 300), (299, 301), (120, 87), (640, 480)], seed=11)
    predictor = importlib.import_module("predictor")
    b, l, s = predictor.main(["--backbone", "mobilenet_v2"], use_custom_images=True, custom_image_path=str(d), batch_size=4)
    assert b.shape == (7, 200, 4) and "predicted 7 images" in capsys.readouterr().out
    hp = train_utils.get_hyper_params("mobilenet_v2")
    hp["total_labels"] = 21
    m = get_model(hp, max_batch=4)
    data_utils.synthetic_weights(m)
    pri = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    host = np.stack([lc.pillow(a, 300, 300) for a in arrays]).astype(np.float32) * np.float32(1.0 / 255.0)
    rb, rl, rs = get_decoder_model(m, pri, hp).predict(host, batch_size=4)
    np.testing.assert_array_equal(l, rl)
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(b, rb)
    assert ((l > 0).sum(-1) > 0).all()
