"""Diagnostics script (not a test): what the mosaic augmentation costs, beside the two launches of the existing
augmentation it is closest to.

One resident batch of B=32 images of 300x300 with VOC-like ground truth (1-7 boxes an image, padded to 8 rows), every
path on preallocated outputs, the paths alternating inside this process, every timed window >= 1 s with ONE stream
synchronise, at its end (tests/bench_augment.py's protocol); per path the median of --rounds windows with its spread:
  (a) ``ssd_augment_mosaic_plan``    the plan and the merged ground truth (p = 1, 32 output rows);
  (b) ``ssd_augment_mosaic_pixels``  the images of that plan;
  (c) ``mosaic_batch_device``        both through the Python surface, outputs allocated per call;
  (d) ``ssd_augment_geometry``       the yardstick of (b): a crop plan on the same batch -- the same output bytes, four
                                     taps a pixel;
  (e) ``ssd_augment_plan``           the yardstick of (a): the 100-attempt sampler's plan of the same ground truth.
``--step-ms``: the B = 32 training step to state (c) as a share of, ``--step-note`` where that figure comes from (printed as it
is).  ``--out`` writes exactly the lines printed.
Usage: python tests/bench_mosaic.py [--rounds 5] [--step-ms 10.2 --step-note "bench.py --train --batch 32, same session"]
       [--out profiles/mosaic_bench.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import augmentation as aug
import ssd_hip as h
from bench_augment import B, G, S, ground_truth, spread, window


def main(rounds, step_ms, step_note, out_path):
    assert torch.cuda.is_available(), "bench_mosaic.py measures on the GPU"
    dev, lib = h.device(), h.lib()
    imgs = torch.rand((B, S, S, 3), dtype=torch.float32, device=dev)
    boxes, labels = ground_truth()
    g, gl = h.to_dev(boxes), h.to_dev(labels, torch.int32)
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    G_out = 4 * G
    mplan = aug.mosaic_plan_device(g, gl, ids, S, S, 4242)
    mout = torch.empty_like(imgs)
    fill = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    aplan = aug.plan_batch_device(g, gl, ids, S, S, 4242)
    # the yardstick's crop plan: every image a window of its own, no expand, no flip-only copy path
    rng = np.random.default_rng(1)
    crop = np.zeros((B, 10), np.int32)
    for b in range(B):
        hh, ww = int(rng.integers(100, 301)), int(rng.integers(100, 301))
        crop[b] = [S, S, 0, 0, int(rng.integers(0, S - hh + 1)), int(rng.integers(0, S - ww + 1)), hh, ww, b & 1, 1]
    crop = h.to_dev(crop, torch.int32)
    gfill = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    gout = torch.empty_like(imgs)

    def plan():
        h.check(lib.ssd_augment_mosaic_plan(h.ptr(g), h.ptr(gl), h.ptr(ids), B, G, S, S, 4242, 1.0, 0.5, 1.0, G_out, -1,
                                            *[h.ptr(t) for t in mplan], h.stream()), "ssd_augment_mosaic_plan")

    def pixels():
        h.check(lib.ssd_augment_mosaic_pixels(h.ptr(imgs), B, S, S, h.ptr(mplan[0]), fill, h.ptr(mout), h.stream()), "ssd_augment_mosaic_pixels")

    def whole():
        aug.mosaic_batch_device(imgs, g, gl, ids, seed=4242)

    def geometry():
        h.check(lib.ssd_augment_geometry(h.ptr(imgs), B, S, S, 3, S, S, h.ptr(crop), h.ptr(gfill), h.ptr(gout), h.stream()), "ssd_augment_geometry")

    def sampler_plan():
        h.check(lib.ssd_augment_plan(h.ptr(g), h.ptr(gl), h.ptr(ids), B, G, S, S, 4242, *[h.ptr(t) for t in aplan], h.stream()), "ssd_augment_plan")

    paths = (("(a) ssd_augment_mosaic_plan", plan), ("(b) ssd_augment_mosaic_pixels", pixels), ("(c) mosaic_batch_device", whole),
             ("(d) ssd_augment_geometry, crop plan", geometry), ("(e) ssd_augment_plan", sampler_plan))
    for _ in range(5):
        for _, fn in paths:
            fn()
    times = {name: [] for name, _ in paths}
    for _ in range(rounds):
        for name, fn in paths:
            times[name].append(window(fn)[0])
    med = {name: statistics.median(ts) for name, ts in times.items()}
    info = mplan[3].cpu().numpy()
    lines = ["mosaic augmentation on %s" % torch.cuda.get_device_name(0),
             "B=%d resident %dx%d float32 images, 1-7 boxes each in %d rows, %d output rows (kept %d..%d a mosaic); p = 1, scale 0.5..1;" % (
                 B, S, S, G, G_out, info[:, 1].min(), info[:, 1].max()),
             "preallocated outputs, the paths alternating, one synchronise per window of >= 1 s, wall time per call:"]
    lines += ["  %-38s %s" % (name, spread(times[name], "us", 1e6)) for name, _ in paths]
    a, b, c, d, e = (med[name] for name, _ in paths)
    lines.append("  pixels / geometry (b)/(d): %.2fx (expected within 1.5x);  plan / sampler plan (a)/(e): %.2fx (expected below 1x)" % (b / d, a / e))
    lines.append("  output bytes of (b) and (d): %.1f MB each; (b) at %.0f GB/s of output" % (B * S * S * 12 / 1e6, B * S * S * 12 / b / 1e9))
    if step_ms:
        lines.append("  (c) against the B = 32 training step of %.3f ms (%s): %.2f %%" % (step_ms, step_note, 100.0 * c * 1e3 / step_ms))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=0.0)
    ap.add_argument("--step-note", default="bench.py --train --batch 32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    main(a.rounds, a.step_ms, a.step_note, a.out)
