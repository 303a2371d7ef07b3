"""Diagnostics script (not a test): what drawing detections on the device (``ssd_image_minmax`` + ``ssd_draw_detections``)
costs against the reference's per-image PIL loop on the host.

One batch of B=64 seeded 300x300 float images with the REAL detections of the synthetic-weight SSD300-MobileNetV2
(``predict``: up to 200 boxes per image), images resident on the device as they are when ``predict`` finishes:
  (a) host path   -- copy the device images to the host, then per image ``array_to_img`` + ``ImageDraw.text`` +
                     ``ImageDraw.rectangle`` per detection (the reference's ``draw_bboxes_with_labels`` without plt);
  (b) device path -- ``draw_detections_batch`` (denormalise, format and encode the text, ONE upload, the kernels), the
                     upload included, closed by a device synchronise;
  (c) the kernels alone on resident inputs, by device events;
and the copy bound: the time to read 12 B and write 3 B per pixel at the bandwidth a device-to-device copy of the same
size reaches on this card.  Every timed window is >= 1 s; every figure is the median of --rounds windows with its spread.
Usage: python tests/bench_draw.py [--rounds 5]"""
import argparse
import os
import statistics
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import drawing_cases as dc
import helpers
import ssd_hip as h
from utils import bbox_utils
from utils import drawing_utils as du

B, S = 64, 300


def spread(xs, unit, scale=1.0):
    xs = [x * scale for x in xs]
    return "%.3f %s (median; min %.3f .. max %.3f, n=%d)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def window(fn, min_seconds=1.0):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def events(fn, K):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / K


def detections():
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    model = get_model(hp, max_batch=B)
    model.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    dm = get_decoder_model(model, priors, hp)
    x = helpers.images(B, S, seed=0)
    b, l, s = dm.predict(x, batch_size=B)
    dm.close()
    return x, b, l, s


def main(rounds):
    imgs, boxes, labels, scores = detections()
    cols = dc.colors(9)
    x = h.to_dev(imgs)
    per_image = (labels > 0).sum(-1)
    print("B=%d images %dx%d, detections per image: mean %.1f, min %d, max %d" % (B, S, S, per_image.mean(), per_image.min(), per_image.max()))

    def host_path():
        host = x.cpu().numpy()
        return [dc.pillow(dc.batch_case(host, boxes, labels, scores, i, cols)) for i in range(B)]

    def device_path():
        return du.draw_detections_batch(x, boxes, labels, scores, dc.LABELS, colors=cols)

    want, got = np.stack(host_path()), device_path().cpu().numpy()
    assert np.array_equal(want, got), "device path differs from the host path in %d pixels" % int((want != got).any(-1).sum())
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(host_path))
        tb.append(window(device_path))
    print("(a) host path (device-to-host copy + PIL loop per image)        : " + spread(ta, "ms/batch", 1e3))
    print("(b) device path (draw_detections_batch, upload included)        : " + spread(tb, "ms/batch", 1e3))
    print("    ratio of the medians (a) / (b)                              : %.1fx; outputs byte-equal" % (
        statistics.median(ta) / statistics.median(tb)))
    # (c) the kernels alone: resident boxes and text
    ib = du._int_boxes(bbox_utils.denormalize_bboxes(torch.as_tensor(boxes), S, S))
    li = labels.astype(np.int64)
    tbytes, tlen = du.encode_texts([t for row in du.label_texts(ib, li, scores, dc.LABELS) for t in row])
    up = du._upload(ib, li.astype(np.int32), tlen, du._colors_u8(cols, 21), tbytes, x.device)
    out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=x.device)
    for _ in range(10):
        du._launch(x, up, out)
    assert np.array_equal(out.cpu().numpy(), want)
    src = torch.empty(B * S * S * 15 // 2, dtype=torch.uint8, device=x.device)      # a copy that reads and writes 15 B/pixel in all
    dst = torch.empty_like(src)
    for _ in range(10):
        dst.copy_(src)
    tc, tm, K = [], [], 200
    for _ in range(rounds):
        tc.append(events(lambda: du._launch(x, up, out), K))
        tm.append(events(lambda: dst.copy_(src), K))
    nbytes = B * S * S * 15
    kc, km = statistics.median(tc), statistics.median(tm)
    print("(c) ssd_image_minmax + ssd_draw_detections alone (device events, %d back-to-back calls): " % K + spread(tc, "us/call", 1e6))
    print("    device-to-device copy moving the same %.1f MB (read + write)  : " % (nbytes / 1e6) + spread(tm, "us/call", 1e6))
    print("    copy bandwidth %.2f TB/s -> copy bound %.1f us; the kernels take %.2fx the copy bound" % (
        nbytes / km / 1e12, km * 1e6, kc / km))
    print("    (the kernels read the float images twice, 27 B/pixel in all: the batch fits the Infinity Cache)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
