"""Diagnostics script (not a test): what the device LANCZOS resize (``ssd_resize_lanczos``) buys for custom images.

(a) one batch of B=32 seeded VOC-like uint8 images (H, W in 300..500, about 500x375) to 300x300, from host arrays,
    alternating inside this process, every timed window >= 1 s and closed by a device synchronise:
      host path   -- per image ``PIL.Image.resize(..., Image.LANCZOS)``, upload, ``ssd_preprocess`` (the former
                     ``custom_data_generator``), stacked into the batch;
      device path -- ``resize_lanczos_batch`` (pack, ONE upload, ONE call), the upload included;
    the kernels alone by device events on a resident packed buffer, with the bytes they must move and the share of the
    HBM peak that is; PIL's PNG decode of one such image, separately (out of scope here, the remaining host cost).
(b) predictor-style custom serving, images/sec over --batches batches of 32 decoded images: prepare the batches (either
    path), then ``predict()``.

Every figure is the median of --rounds windows with their spread (min .. max).  Usage: python tests/bench_resize.py
[--rounds 5] [--batches 8] [--skip-batch] [--skip-e2e]"""
import argparse
import io
import os
import statistics
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
from PIL import Image
import helpers
import ssd_hip as h
from utils import bbox_utils, data_utils

HBM_PEAK = 8.0e12        # bytes/s, MI355X specification
B, S = 32, 300


def spread(xs, unit, scale=1.0):
    xs = [x * scale for x in xs]
    return "%.3f %s (median; min %.3f .. max %.3f, n=%d)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def window(fn, min_seconds=1.0):
    """Seconds per call over a window of at least ``min_seconds`` that ends in a device synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def voc_like_batch(seed):
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 375), (333, 500), (500, 333)]
    out = []
    for i in range(B):
        hh, ww = sizes[i % 4] if i % 2 else (int(rng.integers(300, 501)), int(rng.integers(300, 501)))
        out.append(rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8))
    return out


def host_path(arrays):
    """What custom_data_generator + padded_batch did before the kernel existed."""
    imgs = []
    for a in arrays:
        resized = np.ascontiguousarray(np.array(Image.fromarray(a).resize((S, S), Image.LANCZOS), dtype=np.uint8))
        imgs.append(data_utils.preprocess_batch(resized[None], S, S)[0])
    return torch.stack(imgs)


def device_path(arrays):
    return data_utils.resize_lanczos_batch(arrays, S, S)


def needed_bytes(arrays):
    """Source read once + intermediate written and read back + float output written."""
    pitch = h.lib().ssd_resize_lanczos_pitch(S)
    n = 0
    for a in arrays:
        n += a.size + (2 * a.shape[0] * pitch if a.shape[1] != S else 0) + S * S * 12
    return n


def per_batch(rounds):
    arrays = voc_like_batch(0)
    a, b = host_path(arrays), device_path(arrays)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "device path differs from the host path"
    for _ in range(3):
        host_path(arrays); device_path(arrays)
    th, td = [], []
    for _ in range(rounds):
        th.append(window(lambda: host_path(arrays)))
        td.append(window(lambda: device_path(arrays)))
    mp = sum(x.shape[0] * x.shape[1] for x in arrays) / 1e6
    print("(a) B=%d VOC-like uint8 images (%.1f Mpixel, %.1f MB) -> %dx%d, from host arrays; outputs bitwise equal" % (
        B, mp, sum(x.size for x in arrays) / 1e6, S, S))
    print("    host path (PIL resize + upload + ssd_preprocess, per image): " + spread(th, "ms/batch", 1e3))
    print("    device path (resize_lanczos_batch, upload included)        : " + spread(td, "ms/batch", 1e3))
    print("    ratio of the medians                                       : %.1fx" % (statistics.median(th) / statistics.median(td)))
    # the kernels alone: resident packed buffer, device events
    layout = data_utils._lanczos_layout(arrays, S, S)
    host = np.zeros(layout["total"], np.uint8)
    data_utils._lanczos_fill(host, arrays, layout)
    packed = torch.as_tensor(host).to(h.device())
    out = torch.empty((B, S, S, 3), dtype=torch.float32, device=h.device())
    for _ in range(10):
        data_utils._lanczos_launch(packed, layout, out)
    assert torch.equal(out.view(torch.int32), b.view(torch.int32))
    tk, K = [], 200
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            data_utils._lanczos_launch(packed, layout, out)
        e1.record()
        e1.synchronize()
        tk.append(e0.elapsed_time(e1) / K)
    nb = needed_bytes(arrays)
    med = statistics.median(tk) * 1e-3
    print("    ssd_resize_lanczos alone (both passes, device events, %d back-to-back calls): " % K + spread(tk, "us/call", 1e3))
    print("    bytes it must move: %.1f MB -> %.2f TB/s = %.1f%% of the %.1f TB/s HBM peak (the batch fits the Infinity Cache: "
          "an upper bound on HBM traffic)" % (nb / 1e6, nb / med / 1e12, 100.0 * nb / med / HBM_PEAK, HBM_PEAK / 1e12))
    # host stages on their own
    png = io.BytesIO()
    Image.fromarray(arrays[1]).save(png, format="PNG")
    raw = png.getvalue()
    dec = lambda: np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"), dtype=np.uint8)
    pil = lambda: Image.fromarray(arrays[1]).resize((S, S), Image.LANCZOS)
    t_dec = [window(dec, 0.5) for _ in range(rounds)]
    t_pil = [window(pil, 0.5) for _ in range(rounds)]
    print("    PIL LANCZOS resize of one %dx%d image on the host          : " % arrays[1].shape[:2] + spread(t_pil, "ms/image", 1e3))
    print("    PIL PNG decode of one such image (noise; not part of either path): " + spread(t_dec, "ms/image", 1e3))


def end_to_end(rounds, n_batches):
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    model = get_model(hp, max_batch=B)
    model.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    dm = get_decoder_model(model, priors, hp)
    decoded = [voc_like_batch(100 + i % 4) for i in range(n_batches)]          # decoded images in host memory
    gt, gl = np.zeros((B, 1, 4), np.float32), -np.ones((B, 1), np.int32)

    def serve(prepare):
        return dm.predict([(prepare(arrays), gt, gl) for arrays in decoded])
    ref, got = serve(host_path), serve(device_path)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y), "detections differ between the two paths"
    rates = {"host path + predict()": [], "device path + predict()": []}
    for _ in range(rounds):
        rates["host path + predict()"].append(n_batches * B / window(lambda: serve(host_path)))
        rates["device path + predict()"].append(n_batches * B / window(lambda: serve(device_path)))
    print("(b) predictor-style custom serving: %d batches of %d decoded images, SSD300-MobileNetV2, lanes=%s; detections equal" % (
        n_batches, B, dm.lanes))
    for name, xs in rates.items():
        print("    %-26s: " % name + spread(xs, "images/sec"))
    dm.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    if not args.skip_batch:
        per_batch(args.rounds)
    if not args.skip_e2e:
        end_to_end(args.rounds, args.batches)
