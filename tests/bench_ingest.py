"""Diagnostics script (not a test): what the ragged preprocess (``ssd_preprocess_ragged``) buys for the VOC input path.

One batch of B=32 decoded VOC-sized uint8 items (``data_utils.synthetic_voc_items``: H, W in 300..500) to 300x300, from
host arrays, the two paths alternating inside this process, every timed window >= 1 s and closed by a device synchronise:
  (a) per image ``preprocessing`` (upload + ``ssd_preprocess``, B = 1) + ``padded_batch``: the path before the kernel;
  (b) ``preprocess_ragged_batch``: pack, ONE upload, ONE launch, the upload included;
  (b') one pass of ``voc_batches`` over the decoded items (the pool, the ground-truth padding and (b));
  (c) the kernel alone, device events around K back-to-back launches on a resident packed buffer;
  (d) a device-to-device copy that moves the same number of bytes (reads + writes = the kernel's source bytes + output
      bytes), the bandwidth yardstick for (c).
Every figure is the median of --rounds windows with their spread (min .. max).  The outputs of (a) and (b) are compared
bit for bit first.  Usage: python tests/bench_ingest.py [--rounds 5]"""
import argparse
import os
import statistics
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
from utils import data_utils

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


def per_image_path(items):
    return next(iter(data_utils.padded_batch((data_utils.preprocessing(x, S, S) for x in items), B)))


def ragged_path(items):
    return data_utils.preprocess_ragged_batch([x["image"] for x in items], S, S)


def events(fn, K):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / K


def main(rounds):
    assert torch.cuda.is_available(), "bench_ingest.py measures on the GPU"
    items = list(data_utils.synthetic_voc_items(B))
    a, b = per_image_path(items), ragged_path(items)
    assert torch.equal(a[0].view(torch.int32), b.view(torch.int32)), "the ragged path differs from the per-image path"
    vb = data_utils.voc_batches(items, B, S, S)
    x, gt, gl = next(iter(vb))
    assert torch.equal(x.view(torch.int32), a[0].view(torch.int32)) and np.array_equal(gt, a[1]) and np.array_equal(gl, a[2])
    for _ in range(3):
        per_image_path(items); ragged_path(items); list(vb)
    ta, tb, tv = [], [], []
    for _ in range(rounds):
        ta.append(window(lambda: per_image_path(items)))
        tb.append(window(lambda: ragged_path(items)))
        tv.append(window(lambda: list(vb)))
    src_bytes = sum(it["image"].size for it in items)
    out_bytes = B * S * S * 3 * 4
    print("B=%d VOC-sized uint8 images (%.1f MB) -> %dx%d float32 (%.1f MB), from host arrays; outputs bitwise equal" % (
        B, src_bytes / 1e6, S, S, out_bytes / 1e6))
    print("(a)  per image preprocessing + padded_batch (32 uploads, 32 launches): " + spread(ta, "ms/batch", 1e3))
    print("(b)  preprocess_ragged_batch (one upload, one launch), upload included : " + spread(tb, "ms/batch", 1e3))
    print("(b') one voc_batches pass over the decoded items (pool + padding + (b)) : " + spread(tv, "ms/batch", 1e3))
    print("     ratio of the medians (a)/(b): %.2fx" % (statistics.median(ta) / statistics.median(tb)))
    # (c) the kernel alone on a resident packed buffer
    arrays = [it["image"] for it in items]
    layout = data_utils._ragged_layout(arrays)
    host = np.zeros(layout["total"], np.uint8)
    data_utils._ragged_fill(host, arrays, layout)
    packed = torch.as_tensor(host).to(h.device())
    out = torch.empty((B, S, S, 3), dtype=torch.float32, device=h.device())
    launch = lambda: data_utils._ragged_launch(packed, layout, S, S, out)
    for _ in range(10):
        launch()
    assert torch.equal(out.view(torch.int32), b.view(torch.int32))
    # (d) a copy with the same traffic: n bytes read + n bytes written = src_bytes + out_bytes
    n = (src_bytes + out_bytes) // 2
    c_src, c_dst = torch.zeros(n, dtype=torch.uint8, device=h.device()), torch.empty(n, dtype=torch.uint8, device=h.device())
    copy = lambda: c_dst.copy_(c_src)
    for _ in range(10):
        copy()
    K = 200
    tc, td = [], []
    for _ in range(rounds):
        tc.append(events(launch, K))
        td.append(events(copy, K))
    mc, md = statistics.median(tc), statistics.median(td)
    moved = src_bytes + out_bytes
    print("(c)  ssd_preprocess_ragged alone (device events, %d back-to-back launches): " % K + spread(tc, "us/call", 1e6))
    print("     bytes it must move: %.1f MB -> %.2f TB/s" % (moved / 1e6, moved / mc / 1e12))
    print("(d)  device copy of %.1f MB (the same %.1f MB of reads + writes)          : " % (n / 1e6, moved / 1e6)
          + spread(td, "us/call", 1e6) + " -> %.2f TB/s" % (moved / md / 1e12))
    print("     (c)/(d) = %.2f" % (mc / md))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
