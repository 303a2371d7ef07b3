"""Diagnostics script (not a test): what drawing the augmentation plan on the device buys for the training input path.

One resident batch of B=32 images of 300x300 with VOC-like ground truth (1-7 boxes an image, padded to 8 rows), the two
paths alternating inside this process, every timed window >= 1 s with ONE stream synchronise, at its end:
  (a) ``apply_batch``: the plan drawn on the host (``draw_plan`` per image), five small uploads, up to four launches;
  (b) ``apply_batch_device``: the plan drawn by ``ssd_augment_plan``, five launches, nothing uploaded.
Per path two figures, each the median of --rounds windows with its spread (min .. max): the wall time per batch (the
window including its closing synchronise) and the HOST thread's time per batch up to its last launch (the same window
without the synchronise) -- the time the thread that also issues the training step's launches is busy.
(a') is ``draw_plan`` alone for the batch (no device work).  Usage: python tests/bench_augment.py [--rounds 5]"""
import argparse
import os
import statistics
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import augmentation as aug
import ssd_hip as h

B, S, G = 32, 300, 8


def spread(xs, unit, scale=1.0):
    xs = [x * scale for x in xs]
    return "%.3f %s (median; min %.3f .. max %.3f, n=%d)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def window(fn, min_seconds=1.0):
    """(wall seconds per call, host seconds per call up to the last launch) over a window of at least ``min_seconds``
    that ends in a device synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, (t1 - t0) / n


def ground_truth(seed=0):
    rng = np.random.default_rng(seed)
    boxes, labels = np.zeros((B, G, 4), np.float32), np.full((B, G), -1, np.int32)
    for b in range(B):
        n = int(rng.integers(1, 8))
        c, s = rng.uniform(0.15, 0.85, (n, 2)), rng.uniform(0.03, 0.35, (n, 2))
        boxes[b, :n] = np.clip(np.concatenate([c - s, c + s], 1), 0, 1)
        labels[b, :n] = rng.integers(1, 21, n)
    return boxes, labels


def main(rounds):
    assert torch.cuda.is_available(), "bench_augment.py measures on the GPU"
    imgs = torch.rand((B, S, S, 3), dtype=torch.float32, device=h.device())
    boxes, labels = ground_truth()
    aug.seed(0)
    device_fn = aug.device_draws(4242)
    host = lambda: aug.apply_batch(imgs, boxes, labels)
    device = lambda: device_fn(imgs, boxes, labels)

    def draws_only():
        for b in range(B):
            aug.draw_plan(S, S, boxes[b][labels[b] > 0])
    for _ in range(5):
        host(); device()
    ta, tb, td = [], [], []
    for _ in range(rounds):
        ta.append(window(host))
        tb.append(window(device))
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < 0.5:
            draws_only()
            n += 1
        td.append((time.perf_counter() - t0) / n)
    print("B=%d resident %dx%d float32 images, 1-7 boxes each in %d rows; one synchronise per window of >= 1 s" % (B, S, S, G))
    print("(a)  apply_batch, host draws         wall : " + spread([t[0] for t in ta], "ms/batch", 1e3))
    print("                                     host : " + spread([t[1] for t in ta], "ms/batch", 1e3))
    print("(a') draw_plan x %d alone (host only)      : " % B + spread(td, "ms/batch", 1e3))
    print("(b)  apply_batch_device, device plan wall : " + spread([t[0] for t in tb], "ms/batch", 1e3))
    print("                                     host : " + spread([t[1] for t in tb], "ms/batch", 1e3))
    ma, mb = statistics.median(t[0] for t in ta), statistics.median(t[0] for t in tb)
    ha, hb = statistics.median(t[1] for t in ta), statistics.median(t[1] for t in tb)
    print("     ratio of the medians (a)/(b): wall %.2fx, host %.2fx" % (ma / mb, ha / hb))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
