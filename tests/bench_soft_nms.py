"""Diagnostics script (not a test): the decoder behind an ``ssd_nms_config`` (``ssd_decode_nms_cfg``, csrc/ssd_decode.hip
``soft_nms_kernel``) beside ``ssd_decode_nms`` at the shape of the benchmark's inference step, B = 64, N = 2268, L = 21
(``helpers.decoder_inputs``, the SSD300-MobileNetV2 priors), at the score thresholds 0.5 (the reference's) and 0.01 (the
evaluation protocols').  Subjects: ``ssd_decode_nms``; hard per class through ``_cfg`` (the same launches); Gaussian and
linear Soft-NMS; class-agnostic hard and Gaussian.

Timing: --graph back-to-back calls on resident inputs and outputs are captured as one linear graph (a replay costs the host one
launch, so the device is timed, not the host's issue rate); device events around a window of --calls replays, three untimed
ones first; the subjects alternate inside one process, --rounds rounds; reported is the median window with min .. max, per
call, and each subject against ``ssd_decode_nms`` of the same run and against --step-ms, the one-at-a-time inference step.
Usage: python tests/bench_soft_nms.py [--rounds 5] [--calls 20] [--graph 10] [--batch 64] [--step-ms 1.46]"""
import argparse
import os
import statistics
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
import helpers
from bench_focal import graphed, window

SUBJECTS = (("ssd_decode_nms", None), ("hard via _cfg", ("hard", False)), ("gaussian", ("gaussian", False)),
            ("linear", ("linear", False)), ("agnostic hard", ("hard", True)), ("agnostic gaussian", ("gaussian", True)))


def main(args):
    B, N, L, T = args.batch, 2268, 21, 200
    lib = h.lib()
    deltas, probs = helpers.decoder_inputs(B, N, L)
    priors = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "priors.npz"))["mobilenet_v2"]
    dd, pd, pri = h.to_dev(deltas), h.to_dev(probs), h.to_dev(priors.astype(np.float32))
    dev = dd.device
    ob, ol, osc = torch.empty((B, T, 4), device=dev), torch.empty((B, T), device=dev), torch.empty((B, T), device=dev)
    v = torch.empty((B,), dtype=torch.int32, device=dev)
    var_p, _keep = h.host4(helpers.VARIANCES)
    ws = torch.empty(lib.ssd_decode_nms_workspace_bytes(B, N, L, T), dtype=torch.uint8, device=dev)
    amax0 = probs.argmax(-1) == 0
    print("B = %d, N = %d, L = %d, max_total = max_per_class = %d; windows of %d %s between two device events, median of %d" % (
        B, N, L, T, args.calls, "replays of a graph of %d calls" % args.graph if args.graph else "calls", args.rounds))
    for thr in (0.5, 0.01):
        cand = np.where(amax0[..., None], 0, probs) > np.float32(thr)
        per_list, per_image = cand.sum(1), cand.sum((1, 2))
        subjects = []
        for name, mode in SUBJECTS:
            if mode is None:
                def fn(thr=thr):
                    h.check(lib.ssd_decode_nms(h.ptr(dd), h.ptr(pd), h.ptr(pri), var_p, B, N, L, T, T, 0.5, thr, h.ptr(ob), h.ptr(ol),
                                               h.ptr(osc), h.ptr(v), None, h.ptr(ws), ws.numel(), h.stream()), "ssd_decode_nms")
            else:
                cfg = h.nms_config(mode[0], mode[1], T, T, 0.5, thr, 0.5)

                def fn(cfg=cfg):
                    h.check(lib.ssd_decode_nms_cfg(h.ptr(dd), h.ptr(pd), h.ptr(pri), var_p, B, N, L, cfg, h.ptr(ob), h.ptr(ol),
                                                   h.ptr(osc), h.ptr(v), None, h.ptr(ws), ws.numel(), h.stream()), "ssd_decode_nms_cfg")
            fn()
            torch.cuda.synchronize()
            kept = int(v.sum().item())
            subjects.append((name, graphed(fn, args.graph) if args.graph else fn, kept))
        times = {name: [] for name, _, _ in subjects}
        for _ in range(args.rounds):
            for name, fn, _ in subjects:
                times[name].append(window(fn, args.calls) / max(args.graph, 1))
        print("score threshold %g: candidates per (image, class) list mean %.1f, max %d; per image mean %.0f, max %d" % (
            thr, per_list.mean(), per_list.max(), per_image.mean(), per_image.max()))
        base = statistics.median(times["ssd_decode_nms"])
        for name, _, kept in subjects:
            xs = times[name]
            med = statistics.median(xs)
            print("  %-18s %8.1f us/call (min %.1f .. max %.1f)   %5.2f x ssd_decode_nms   %5.1f %% of a %.2f ms step   %d rows kept" % (
                name, med, min(xs), max(xs), med / base, med / (args.step_ms * 10.0), args.step_ms, kept))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--graph", type=int, default=10, help="calls per captured graph (0: plain calls, host issue included)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step-ms", type=float, default=1.46, help="the one-at-a-time inference step the figures are set against")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_soft_nms.py measures on the GPU"
    main(args)
