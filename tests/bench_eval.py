"""Diagnostics script (not a test): what the device scoring path (``ssd_eval_match``) buys.

(a) one batch at B=64, T=200, G=16, L=21 on the detections of tests/test_eval_gpu.py, from host arrays (what
    ``evaluate_predictions`` sees): ``update_stats`` (host walk) against ``update_stats_device``, alternating inside
    this process, every timed window >= 1 s and closed by a device synchronise; the kernel alone by device events.
(b) images/sec over --batches batches of 64 resident images: ``predict()`` alone, ``predict()`` + the host-walk
    ``evaluate_predictions`` and ``evaluate()``.

Every figure is the mean of --rounds windows with their spread (min .. max).  Usage: python tests/bench_eval.py
[--rounds 5] [--batches 64] [--lanes N] [--skip-batch] [--skip-e2e]"""
import argparse
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import eval_cases as ec
import helpers
import ssd_hip as h
from utils import bbox_utils, data_utils, eval_utils as eu


def spread(xs, unit, scale=1.0):
    xs = [x * scale for x in xs]
    return "%.3f %s (min %.3f .. max %.3f, n=%d)" % (sum(xs) / len(xs), unit, min(xs), max(xs), len(xs))


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


def per_batch(rounds):
    B, T, G, L = 64, 200, 16, 21
    pb, pl, ps, gt, gl, _ = ec.case(B, T, G, L)
    labels = ec.labels_for(L)
    host = lambda: eu.update_stats(pb, pl, ps, gt, gl, eu.init_stats(labels))
    device = lambda: eu.update_stats_device(pb, pl, ps, gt, gl, eu.init_stats(labels))
    ec.assert_stats_equal(device(), host())
    for _ in range(3):
        host(); device()
    th, td = [], []
    for _ in range(rounds):
        th.append(window(host))
        td.append(window(device))
    print("(a) B=%d T=%d G=%d L=%d, one batch from host arrays" % (B, T, G, L))
    print("    update_stats (host walk)    : " + spread(th, "ms/batch", 1e3))
    print("    update_stats_device         : " + spread(td, "ms/batch", 1e3))
    print("    ratio of the means          : %.1fx" % (sum(th) / sum(td)))
    dev = [h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32)]
    for _ in range(10):
        eu.match_detections(*dev)
    tk = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        K = 200
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            eu.match_detections(*dev)
        e1.record()
        e1.synchronize()
        tk.append(e0.elapsed_time(e1) / K)
    print("    ssd_eval_match alone (device events, %d back-to-back launches): " % K + spread(tk, "us/launch", 1e3))


def end_to_end(rounds, n_batches, lanes):
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    B = 64
    hp = helpers.hyper_params("mobilenet_v2")
    model = get_model(hp, max_batch=B)
    model.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    dm = get_decoder_model(model, priors, hp, lanes=lanes)
    labels = ["bg"] + data_utils.get_labels()
    images = [h.to_dev(helpers.images(B, 300, seed=i)) for i in range(8)]        # resident; cycled
    data = []
    for i in range(n_batches):
        gt, gl = data_utils.synthetic_gt(B, seed=1000 + i)
        data.append((images[i % 8], gt, gl))

    def predict_only():
        return dm.predict(data)

    def predict_then_host_walk():
        b, l, s = dm.predict(data)
        stats = eu.init_stats(labels)
        for i, (_, gt, gl) in enumerate(data):
            eu.update_stats(b[i * B:(i + 1) * B], l[i * B:(i + 1) * B], s[i * B:(i + 1) * B], gt, gl, stats)
        return eu.calculate_mAP(stats)

    def evaluate():
        return dm.evaluate(data, labels)

    ref, ref_map = predict_then_host_walk()
    got, got_map = evaluate()
    ec.assert_stats_equal(got, ref)
    assert float(got_map) == float(ref_map)
    predict_only()
    rates = {"predict() alone": [], "predict() + host-walk evaluate_predictions": [], "evaluate()": []}
    for _ in range(rounds):
        for name, fn in (("predict() alone", predict_only), ("predict() + host-walk evaluate_predictions", predict_then_host_walk),
                         ("evaluate()", evaluate)):
            rates[name].append(n_batches * B / window(fn))
    print("(b) %d batches of %d resident images, lanes=%s (in use: %s), mean detections/image %.1f" % (
        n_batches, B, dm.lanes, getattr(dm, "_lanes_active", dm.lanes > 1) and dm.lanes > 1,
        sum(len(r["tp"]) for r in ref.values()) / float(n_batches * B)))
    for name, xs in rates.items():
        print("    %-44s: " % name + spread(xs, "images/sec"))
    dm.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--lanes", type=int, default=None)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    args = ap.parse_args()
    if not args.skip_batch:
        per_batch(args.rounds)
    if not args.skip_e2e:
        end_to_end(args.rounds, args.batches, args.lanes)
