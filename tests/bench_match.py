"""Diagnostics script (not a test): target assignment behind an ``ssd_match_config`` (``ssd_match_encode_cfg``,
csrc/ssd_match.hip) beside ``ssd_match_encode`` at the shape of the training step, B = 32 images of G = 42 padded rows with
VOC-like boxes (1 .. 42 valid rows per image, a share of them small), L = 21, on both prior sets (N = 2268 and 8732).
Subjects: ``ssd_match_encode`` (the yardstick); ``max_iou`` through ``_cfg`` (the same launch); ``bipartite``; ``atss`` at
top-k 9.

Timing: --graph back-to-back calls on resident inputs and outputs are captured as one linear graph (a replay costs the host one
launch, so the device is timed, not the host's issue rate); device events around a window of --calls replays, three untimed
ones first; the subjects alternate inside one process, --rounds rounds; reported is the median window with min .. max, per
batch, and each subject against ``ssd_match_encode`` of the same run and against --step-ms, the training step of
``bench.py --train`` at B = 32.  The budget: a strategy stays below 2 % of that step.
Usage: python tests/bench_match.py [--rounds 5] [--calls 20] [--graph 10] [--batch 32] [--rows 42] [--step-ms 10]"""
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
import match_cases as mc
from bench_focal import graphed, window

SUBJECTS = ("ssd_match_encode", "max_iou via _cfg", "bipartite", "atss top-9")


def main(args):
    B, G, L = args.batch, args.rows, 21
    lib = h.lib()
    var_p, _keep = h.host4(helpers.VARIANCES)
    gt, gl = mc.voc_like(np.random.default_rng(20264), B, G)
    print("B = %d, G = %d (%.1f valid rows per image), L = %d; windows of %d %s between two device events, median of %d; budget 2 %% of a "
          "%.2f ms step = %.0f us" % (B, G, (gl > 0).sum(1).mean(), L, args.calls,
                                      "replays of a graph of %d calls" % args.graph if args.graph else "calls", args.rounds,
                                      args.step_ms, args.step_ms * 20.0))
    for backbone in ("mobilenet_v2", "vgg16"):
        priors = mc.priors_of(backbone)
        N = priors.shape[0]
        p, g, l = h.to_dev(priors), h.to_dev(gt), h.to_dev(gl, torch.int32)
        dev = p.device
        deltas = torch.empty((B, N, 4), device=dev)
        onehot = torch.empty((B, N, L), device=dev)
        lab = torch.empty((B, N), dtype=torch.int32, device=dev)
        am = torch.empty((B, N), dtype=torch.int32, device=dev)
        configs = {"max_iou via _cfg": h.match_config("max_iou", 0.5), "bipartite": h.match_config("bipartite", 0.5),
                   "atss top-9": h.match_config("atss", 0.5, 9, mc.level_starts(backbone))}
        ws = torch.empty((max(16, max(lib.ssd_match_encode_cfg_workspace_bytes(B, N, G, c) for c in configs.values())),),
                         dtype=torch.uint8, device=dev)
        subjects = []
        for name in SUBJECTS:
            if name in configs:
                def fn(cfg=configs[name]):
                    h.check(lib.ssd_match_encode_cfg(h.ptr(p), h.ptr(g), h.ptr(l), var_p, cfg, B, N, G, L, h.ptr(deltas), h.ptr(lab),
                                                     h.ptr(am), h.ptr(onehot), h.ptr(ws), ws.numel(), h.stream()), "ssd_match_encode_cfg")
            else:
                def fn():
                    h.check(lib.ssd_match_encode(h.ptr(p), h.ptr(g), h.ptr(l), var_p, 0.5, B, N, G, L, h.ptr(deltas), h.ptr(lab),
                                                 h.ptr(am), h.ptr(onehot), h.stream()), "ssd_match_encode")
            fn()
            torch.cuda.synchronize()
            positives = int((lab > 0).sum().item())
            subjects.append((name, graphed(fn, args.graph) if args.graph else fn, positives))
        times = {name: [] for name in SUBJECTS}
        for _ in range(args.rounds):
            for name, fn, _ in subjects:
                times[name].append(window(fn, args.calls) / max(args.graph, 1))
        base = statistics.median(times["ssd_match_encode"])
        print("%s, N = %d:" % (backbone, N))
        for name, _, positives in subjects:
            xs = times[name]
            med = statistics.median(xs)
            print("  %-18s %8.1f us/batch (min %.1f .. max %.1f)   %5.2f x ssd_match_encode   %5.2f %% of a %.2f ms step   %s   %d positives" % (
                name, med, min(xs), max(xs), med / base, med / (args.step_ms * 10.0), args.step_ms,
                "within the budget" if med <= args.step_ms * 20.0 else "OVER the budget", positives))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--graph", type=int, default=10, help="calls per captured graph (0: plain calls, host issue included)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=42)
    ap.add_argument("--step-ms", type=float, default=10.0, help="the training step (bench.py --train, B = 32) the figures are set against")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_match.py measures on the GPU"
    main(args)
