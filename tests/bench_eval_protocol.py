"""Diagnostics script (not a test): what the protocol matching kernel (``ssd_eval_match_protocol``) costs.

One batch at B=64, T=200, G=16, L=21 (tests/eval_protocol_cases.py's planted batch), resident on the device:
(a) the existing ``ssd_eval_match``; (b) the new kernel, VOC rule, one threshold; (c) the new kernel, COCO rule, ten
thresholds -- each by device events around --launches back-to-back launches, the three alternating inside every
round; (d) the NumPy oracle on the host for the same batch (VOC, one threshold and COCO, ten), by the host clock.

Every figure is the median of --rounds rounds with its spread (min .. max).  The kernel's records are checked against
the oracle's before anything is timed.  Usage: python tests/bench_eval_protocol.py [--rounds 7] [--launches 200]
[--out FILE]"""
import argparse
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import eval_protocol_cases as pc
import ssd_hip as h
from utils import eval_utils as eu


def spread(xs, unit, scale=1.0):
    xs = sorted(x * scale for x in xs)
    return "median %.3f %s (min %.3f .. max %.3f, n=%d)" % (float(np.median(xs)), unit, xs[0], xs[-1], len(xs))


def events(fn, launches):
    """Milliseconds per call over ``launches`` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def main(rounds, launches, out):
    B, T, G, L = 64, 200, 16, 21
    pb, pl, ps, gt, gl, gi, names = pc.planted(B, T, G, L)
    thr10 = pc.COCO_THRESHOLDS
    dev = [h.to_dev(pb), h.to_dev(pl), h.to_dev(ps), h.to_dev(gt), h.to_dev(gl, dtype=torch.int32)]
    flags = h.to_dev(gi, dtype=torch.uint8)
    for rule, thr in (("voc", (0.5,)), ("coco", thr10)):
        ref = pc.oracle_records(pb, pl, ps, gt, gl, gi, rule, thr)
        got = [t.cpu().numpy() for t in eu.match_detections_protocol(*dev, flags, rule, thr)]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[3]) and np.array_equal(got[3], ref[4])
    # the C entry points on preallocated outputs: the timed loop holds no allocation and no Python marshalling beyond
    # the ctypes call, so the figure is the kernel's (launch included), not the wrapper's
    import ctypes
    lib, dp = h.lib(), [h.ptr(t) for t in dev]
    o32 = [torch.empty((B, T), dtype=torch.int32, device=h.device()) for _ in range(3)]
    osc = torch.empty((B, T), dtype=torch.float32, device=h.device())
    ost = torch.empty((B, 10, T), dtype=torch.int8, device=h.device())
    on = torch.empty((B,), dtype=torch.int32, device=h.device())
    thr1 = np.array([0.5], np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def old_kernel():
        h.check(lib.ssd_eval_match(*dp, B, T, G, 0.5, h.ptr(o32[0]), h.ptr(osc), h.ptr(o32[1]), h.ptr(o32[2]), h.ptr(on), h.stream()))

    def new_kernel(rule, thr):
        h.check(lib.ssd_eval_match_protocol(*dp, h.ptr(flags), B, T, G, rule, fp(thr), len(thr), h.ptr(o32[0]), h.ptr(osc),
                                            h.ptr(o32[2]), h.ptr(ost), h.ptr(on), h.stream()))
    runs = (("(a) ssd_eval_match", old_kernel),
            ("(b) ssd_eval_match_protocol, VOC, NT=1", lambda: new_kernel(h.EVAL_RULE_VOC, thr1)),
            ("(c) ssd_eval_match_protocol, COCO, NT=10", lambda: new_kernel(h.EVAL_RULE_COCO, thr10)),
            ("    the Python wrapper of (c), allocations included", lambda: eu.match_detections_protocol(*dev, flags, "coco", thr10)))
    for _, fn in runs:
        for _ in range(20):
            fn()
    times = {name: [] for name, _ in runs}
    for _ in range(rounds):
        for name, fn in runs:
            times[name].append(events(fn, launches))
    host = {"(d) NumPy oracle on the host, VOC, NT=1": ("voc", (0.5,)), "(d) NumPy oracle on the host, COCO, NT=10": ("coco", thr10)}
    host_times = {name: [] for name in host}
    for _ in range(max(rounds // 2, 3)):
        for name, (rule, thr) in host.items():
            t0 = time.perf_counter()
            pc.oracle_records(pb, pl, ps, gt, gl, gi, rule, thr)
            host_times[name].append(time.perf_counter() - t0)
    lines = ["B=%d T=%d G=%d L=%d, %d records; per launch, %d back-to-back launches between device events, %d rounds" % (
        B, T, G, L, int((pl != 0).sum()), launches, rounds)]
    for name, _ in runs:
        lines.append("    %-52s: %s" % (name, spread(times[name], "us", 1e3)))
    for name in host:
        lines.append("    %-52s: %s" % (name, spread(host_times[name], "ms", 1e3)))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    main(args.rounds, args.launches, args.out)
