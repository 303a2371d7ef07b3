"""Diagnostics script (not a test): the time of the optimizer step alone (``ssd_net_optimizer_step``) on the flat trainable
vector of SSD300-MobileNetV2 and SSD300-VGG16 (21 labels), one GPU, a resident synthetic gradient, no forward pass.

Settings: Adam (no clip: what ``ssd_net_adam_step`` and ``compile()``'s default run), SGD plain, SGD with momentum, SGD with momentum + ``clipnorm``, SGD with
momentum + ``global_clipnorm``, SGD with momentum under ``freeze_backbone()``.  The settings alternate inside one process,
round after round; after every change three untimed steps run; every timed window is >= --seconds of back-to-back steps
closed by ONE synchronise.  Reported: median of --rounds windows with min .. max, and the achieved bytes per second against
the traffic the design counts per trainable element: SGD 12 B (gradient in, variable in and out), with momentum 20 B, Adam
28 B, plus 4 B for the norm pass's extra read of the gradient.
Usage: python tests/bench_optimizer.py [--rounds 5] [--seconds 0.5] [--nets mobilenet_v2,vgg16]"""
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

LR = 1e-7


def settings():
    import optimizers as o
    return [("adam", "Adam", lambda: o.Adam(LR), False, 28),
            ("sgd", "SGD", lambda: o.SGD(LR), False, 12),
            ("mom", "SGD momentum 0.9", lambda: o.SGD(LR, momentum=0.9), False, 20),
            ("mom-clipnorm", "SGD momentum 0.9, clipnorm 1", lambda: o.SGD(LR, momentum=0.9, clipnorm=1.0), False, 24),
            ("mom-global", "SGD momentum 0.9, global_clipnorm 5", lambda: o.SGD(LR, momentum=0.9, global_clipnorm=5.0), False, 24),
            ("mom-frozen", "SGD momentum 0.9, backbone frozen", lambda: o.SGD(LR, momentum=0.9), True, 20)]


def window(fn, min_seconds):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench_net(backbone, rounds, seconds):
    import helpers
    from models._net import SSDModel
    hp = helpers.hyper_params(backbone)
    model = SSDModel(backbone, hp)
    model.set_weights(helpers.synthetic_weights(backbone, hp))
    model.compile(learning_rate=LR)
    h.check(h.lib().ssd_net_train_begin(model._net, 1), "ssd_net_train_begin")
    model._train_batch = 1
    P = int(h.lib().ssd_net_trainable_floats(model._net))
    g = torch.from_numpy((np.random.default_rng(0).standard_normal(P) * 0.01).astype(np.float32)).to(h.device())
    offs = model.trainable_offsets()
    times = {k: [] for k, *_ in settings()}
    elems = {}
    for _ in range(rounds):
        for key, _, make, freeze, _ in settings():
            model.set_trainable("*", True)
            frozen = set(model.freeze_backbone()) if freeze else set()
            elems[key] = sum(int(np.prod(s)) for n, (_, s) in offs.items() if n.rsplit("/", 1)[0] not in frozen)
            model.compile(optimizer=make())
            step = lambda: model.apply_gradients(g)
            step(); step(); step()
            times[key].append(window(step, seconds))
    model.set_trainable("*", True)
    print("SSD300 %s optimizer step alone, %d trainable floats in %d variables; windows >= %.2g s, one synchronise each" % (
        backbone, P, len(offs), seconds))
    for key, text, _, _, bytes_per in settings():
        xs = [1e6 * t for t in times[key]]
        med = statistics.median(xs)
        print("  %-40s %9.1f us/step (median; min %.1f .. max %.1f, n=%d)  %9d elements x %2d B -> %6.2f TB/s" % (
            text, med, min(xs), max(xs), len(xs), elems[key], bytes_per, elems[key] * bytes_per / med * 1e-6))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--nets", default="mobilenet_v2,vgg16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optimizer.py measures on the GPU"
    for net in args.nets.split(","):
        bench_net(net, args.rounds, args.seconds)
