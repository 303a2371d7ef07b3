"""Diagnostics script (not a test): the loss phase of a training step with an IoU-family localisation loss
(``ssd_iou_loc_loss``, csrc/ssd_iouloss.hip) beside the Huber term, at the shape of one MobileNetV2-SSD300 step, B = 32,
N = 2268 (its priors), L = 21, everything with gradients:
  mining, Huber      one ``ssd_loss`` call (both terms)
  mining, <mode>     ``ssd_loss`` on the labels alone, then ``ssd_iou_loc_loss``          (what the training step issues)
  focal, Huber       one ``ssd_focal_loss`` call
  focal, <mode>      ``ssd_focal_loss`` on the labels alone, then ``ssd_iou_loc_loss``
  <mode> alone       ``ssd_iou_loc_loss`` by itself
and, with --step, the whole training step (forward, loss, backward, optimizer) compiled with the Huber term against the same
step compiled with ``IoULocLoss(..., "ciou")``, alternating, host clock around a synchronised window.

Timing of the loss phase: --graph back-to-back calls on resident buffers are captured as one linear graph (a replay costs the
host one launch, so the device is timed, not the host's issue rate); device events around a window of --calls replays, three
untimed ones first; the subjects alternate inside one process, --rounds rounds; reported is the median window with
min .. max, per call.  --graph 0 times plain calls.
--huber-only [--tree DIR] times nothing but the default step (mining loss, Huber term) of the checkout DIR, which needs
nothing this change adds, and prints one line with that library's build id and the first step's losses: run alternately on
a built checkout of the parent commit and on this one, each in a process of its own, it is the A/B against the parent.
Usage: python tests/bench_iou_loss.py [--rounds 5] [--calls 50] [--graph 20] [--batch 32] [--labels 21] [--step 30]
       python tests/bench_iou_loss.py --huber-only [--tree DIR] [--rounds 4] [--step 30] [--batch 32]"""
import argparse
import os
import statistics
import sys
import time

# --tree DIR: the checkout whose package, library, oracle and helpers are measured (default: the one this file lies in)
_TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[:-1] else \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_TREE + "/tf-ssd_amd", _TREE, _TREE + "/tests"]
import numpy as np
import torch
import ssd_hip as h

MODES = ("iou", "giou", "diou", "ciou")


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


def loss_phase(args):
    import helpers
    from oracle import bbox_oracle as bo
    from ssd_loss import LOC_MODES
    hp = helpers.hyper_params("mobilenet_v2", args.labels)
    B, L = args.batch, args.labels
    priors_np = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    N = priors_np.shape[0]
    gt, gl = helpers.gt_inputs(B, G=8, L=L, seed=3)
    yd_np, yl_np = bo.calculate_actual_outputs(priors_np, gt, gl, hp)
    rng = np.random.default_rng(0)
    z = (rng.standard_normal((B, N, L)) * 2).astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    pd_np = (yd_np + rng.standard_normal(yd_np.shape)).astype(np.float32)
    priors, yd, yl, pd, pp = (h.to_dev(a) for a in (priors_np, yd_np, yl_np, pd_np, e / e.sum(-1, keepdims=True)))
    lib, dev = h.lib(), yd.device
    var = (h.ctypes.c_float * 4)(*hp["variances"])
    loc, conf = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
    gd, gz = torch.empty_like(pd), torch.empty_like(pp)
    ws = torch.empty(max(lib.ssd_focal_loss_workspace_bytes(B, N, L), lib.ssd_loss_workspace_bytes(B, N),
                         lib.ssd_iou_loc_loss_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)

    def mining(deltas):
        a, b, c, d = (h.ptr(yd), h.ptr(pd), h.ptr(loc), h.ptr(gd)) if deltas else (None, None, None, None)
        h.check(lib.ssd_loss(a, b, h.ptr(yl), h.ptr(pp), B, N, L, 3.0, 1.0, c, h.ptr(conf), None, None, d, h.ptr(gz), 1.0 / B,
                             h.ptr(ws), ws.numel(), h.stream()), "ssd_loss")

    def focal(deltas):
        a, b, c, d = (h.ptr(yd), h.ptr(pd), h.ptr(loc), h.ptr(gd)) if deltas else (None, None, None, None)
        h.check(lib.ssd_focal_loss(a, b, h.ptr(yl), h.ptr(pp), B, N, L, 1.0, 0.25, 2.0, c, h.ptr(conf), None, None, d, h.ptr(gz),
                                   1.0 / B, h.ptr(ws), ws.numel(), h.stream()), "ssd_focal_loss")

    def iou(mode):
        h.check(lib.ssd_iou_loc_loss(h.ptr(priors), var, h.ptr(yd), h.ptr(pd), B, N, LOC_MODES[mode], 1.0, h.ptr(loc), None,
                                     h.ptr(gd), 1.0 / B, h.ptr(ws), ws.numel(), h.stream()), "ssd_iou_loc_loss")

    def both(first, mode):
        def run():
            first(False)
            iou(mode)
        return run

    subjects = [("mining, Huber (ssd_loss)", lambda: mining(True))]
    subjects += [("mining, %s" % m, both(mining, m)) for m in MODES]
    subjects += [("focal, Huber (ssd_focal_loss)", lambda: focal(True))]
    subjects += [("focal, %s" % m, both(focal, m)) for m in MODES]
    subjects += [("%s alone (ssd_iou_loc_loss)" % m, (lambda m=m: iou(m))) for m in MODES]
    moved = 4 * (N * 4 + B * N * 4 * 3)                      # priors, the two delta tensors in; the gradient out; each once
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    subjects.append(("device copy of %d bytes" % (moved // 2), lambda: dst.copy_(src)))
    if args.graph:
        subjects = [(name, graphed(fn, args.graph)) for name, fn in subjects]
    times = {name: [] for name, _ in subjects}
    for _ in range(args.rounds):
        for name, fn in subjects:
            times[name].append(window(fn, args.calls) / max(args.graph, 1))
    print("B = %d, N = %d, L = %d (%d positives); windows of %d %s between two device events, median of %d" % (
        B, N, L, int((yd_np != 0).any(-1).sum()), args.calls,
        "replays of a graph of %d calls" % args.graph if args.graph else "calls", args.rounds))
    print("  ssd_iou_loc_loss must move %d bytes (priors and both delta tensors in, the gradient out, each once; the finish"
          " launch reads the inputs a second time); %d workgroups of %d anchors per launch" % (
              moved, B * -(-N // lib.ssd_iou_loc_loss_tile()), lib.ssd_iou_loc_loss_tile()))
    for name, _ in subjects:
        xs = times[name]
        print("  %-36s %8.1f us/call (min %.1f .. max %.1f)" % (name, statistics.median(xs), min(xs), max(xs)))


def whole_step(args):
    """The training step of MobileNetV2-SSD300 at B = --batch, synthetic weights and targets: compiled with the Huber term and
    with CIoU, alternating windows of --step steps (three untimed first), a device synchronise at both ends of a window."""
    import helpers
    from models._net import SSDModel
    from oracle import bbox_oracle as bo
    from ssd_loss import CustomLoss
    if not args.huber_only:
        from ssd_loss import IoULocLoss
    assert os.path.abspath(h.__file__).startswith(_TREE + os.sep), h.__file__
    hp = helpers.hyper_params("mobilenet_v2", args.labels)
    B = args.batch
    priors = bo.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    gt, gl = helpers.gt_inputs(B, G=8, L=args.labels, seed=3)
    yd, yl = (h.to_dev(a) for a in bo.calculate_actual_outputs(priors, gt, gl, hp))
    x = h.to_dev(helpers.images(B, 300, seed=5))
    m = SSDModel("mobilenet_v2", hp, B)
    m.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    hard = CustomLoss(3, 1)
    losses = {"Huber": hard} if args.huber_only else {"Huber": hard, "ciou": IoULocLoss(hard, priors, hp["variances"], "ciou")}
    times = {k: [] for k in losses}
    first = None
    for _ in range(args.rounds):
        for name, loss in losses.items():
            m.compile(learning_rate=1e-6, loss=[loss.loc_loss_fn, loss.conf_loss_fn])
            for i in range(3 + args.step):
                if i == 3:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                loc, conf, g = m.forward_backward(x, yd, yl)
                if first is None:
                    first = (float(loc.mean().item()), float(conf.mean().item()))
                m.apply_gradients(g, 1e-6, 1.0)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.step)
    if args.huber_only:
        xs = times["Huber"]
        print("build %s (%s): default step, B = %d, %d windows of %d steps: %.3f ms/step (min %.3f .. max %.3f), first-step loc %.6f conf %.6f" % (
            h.lib().ssd_build_id().decode(), os.path.relpath(_TREE), B, args.rounds, args.step, statistics.median(xs), min(xs), max(xs),
            first[0], first[1]))
        return
    print("training step, B = %d: windows of %d steps (forward, loss, backward, Adam), host clock around a synchronised window,"
          " the two alternating, median of %d" % (B, args.step, args.rounds))
    for name, xs in times.items():
        print("  %-36s %8.3f ms/step (min %.3f .. max %.3f)" % ("localisation term: " + name, statistics.median(xs), min(xs), max(xs)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--graph", type=int, default=20, help="calls per captured graph (0: plain calls, host issue included)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--labels", type=int, default=21)
    ap.add_argument("--step", type=int, default=30, help="steps per window of the whole-step comparison (0: skip it)")
    ap.add_argument("--huber-only", action="store_true", help="only the default step of --tree, one line")
    ap.add_argument("--tree", default=_TREE, help="the checkout to measure (read before anything is imported)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_iou_loss.py measures on the GPU"
    if args.huber_only:
        whole_step(args)
    else:
        loss_phase(args)
        if args.step:
            whole_step(args)
