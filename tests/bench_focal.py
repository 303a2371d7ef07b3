"""Diagnostics script (not a test): the focal loss kernel pair (``ssd_focal_loss``, csrc/ssd_focal.hip) beside the mining
kernel (``ssd_loss``) at the shape of one MobileNetV2-SSD300 training step, B = 32, N = 2268, L = 21, both with gradients,
and beside a device copy that moves as many bytes as the focal loss must (y, q and the two delta tensors in, the two
gradients out, each once: the copy reads half of that and writes half).

Timing: --graph back-to-back calls on resident inputs and outputs are captured as one linear graph (a replay costs the host one
launch, so the device is timed, not the host's issue rate); device events around a window of --calls replays, three untimed
ones first; the three subjects alternate inside one process, --rounds rounds; reported is the median window with min .. max,
per call.  --graph 0 times plain calls.
Usage: python tests/bench_focal.py [--rounds 5] [--calls 50] [--graph 20] [--batch 32] [--priors 2268] [--labels 21]"""
import argparse
import os
import statistics
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h


def window(fn, calls):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def graphed(fn, inner):
    """``inner`` calls captured as one linear graph: a replay costs the host one launch, so the window times the device."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g.replay


def main(args):
    from ssd_loss import CustomLoss, FocalLoss
    B, N, L = args.batch, args.priors, args.labels
    rng = np.random.default_rng(0)
    z = (rng.standard_normal((B, N, L)) * 2).astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    pos = rng.random((B, N)) < 0.01
    yl = np.zeros((B, N, L), np.float32)
    yl[..., 0] = 1
    bi, ni = np.nonzero(pos)
    yl[bi, ni, 0] = 0
    yl[bi, ni, rng.integers(1, L, len(bi))] = 1
    yd = np.zeros((B, N, 4), np.float32)
    yd[bi, ni] = rng.standard_normal((len(bi), 4)).astype(np.float32)
    yd, yl, pd, pp = (h.to_dev(a) for a in (yd, yl, rng.standard_normal((B, N, 4)).astype(np.float32), e / e.sum(-1, keepdims=True)))
    focal, hard = FocalLoss(1.0, 0.25, 2.0), CustomLoss(3, 1)
    lib, dev = h.lib(), yd.device
    loc, conf = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
    gd, gz = torch.empty_like(pd), torch.empty_like(pp)
    ws = torch.empty(max(lib.ssd_focal_loss_workspace_bytes(B, N, L), lib.ssd_loss_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)

    def run_focal():
        h.check(lib.ssd_focal_loss(h.ptr(yd), h.ptr(pd), h.ptr(yl), h.ptr(pp), B, N, L, focal.loc_loss_alpha, focal.alpha, focal.gamma,
                                   h.ptr(loc), h.ptr(conf), None, None, h.ptr(gd), h.ptr(gz), 1.0 / B, h.ptr(ws), ws.numel(),
                                   h.stream()), "ssd_focal_loss")

    def run_hard():
        h.check(lib.ssd_loss(h.ptr(yd), h.ptr(pd), h.ptr(yl), h.ptr(pp), B, N, L, hard.neg_pos_ratio, hard.loc_loss_alpha, h.ptr(loc),
                             h.ptr(conf), None, None, h.ptr(gd), h.ptr(gz), 1.0 / B, h.ptr(ws), ws.numel(), h.stream()), "ssd_loss")

    moved = 4 * B * N * (3 * L + 3 * 4)                      # y, q, yd, pd in; grad_logits, grad_deltas out
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    subjects = [("ssd_focal_loss, gradients", run_focal), ("ssd_loss (mining 3:1), gradients", run_hard),
                ("device copy of %d bytes" % (moved // 2), lambda: dst.copy_(src))]
    if args.graph:
        subjects = [(name, graphed(fn, args.graph)) for name, fn in subjects]
    times = {name: [] for name, _ in subjects}
    for _ in range(args.rounds):
        for name, fn in subjects:
            times[name].append(window(fn, args.calls) / max(args.graph, 1))
    print("B = %d, N = %d, L = %d (%d positives); windows of %d %s between two device events, median of %d" % (
        B, N, L, len(bi), args.calls, "replays of a graph of %d calls" % args.graph if args.graph else "calls", args.rounds))
    print("  the focal loss must move %d bytes (inputs once, gradients once); tile %d anchors, %d workgroups per launch" % (
        moved, h.lib().ssd_focal_loss_tile(L, None), B * -(-N // h.lib().ssd_focal_loss_tile(L, None))))
    for name, _ in subjects:
        xs = times[name]
        med = statistics.median(xs)
        print("  %-36s %8.1f us/call (min %.1f .. max %.1f)   %6.2f TB/s of those bytes" % (
            name, med, min(xs), max(xs), moved / med * 1e-6))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--graph", type=int, default=20, help="calls per captured graph (0: plain calls, host issue included)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--priors", type=int, default=2268)
    ap.add_argument("--labels", type=int, default=21)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_focal.py measures on the GPU"
    main(args)
