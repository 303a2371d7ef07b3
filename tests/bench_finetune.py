"""Diagnostics script (not a test): what freezing layers (``layer.trainable = False``) buys for the training step.

One resident batch of B=32 images of 300x300; one step = GPU target assignment + training forward + loss + backward + Adam
(bench.py --train's step on one GPU).  Per net -- MobileNetV2 fp32, MobileNetV2 bf16, VGG16 fp32 -- ONE model instance
and four configurations that alternate inside this process, round after round:
  (a) everything trainable;
  (b) every BatchNorm frozen (inference mode on the moving statistics, no dgamma / dbeta);
  (c) the backbone's convs frozen, its BatchNorm layers still trainable (batch statistics, moving averages updated);
  (d) the backbone and its BatchNorm layers frozen (``model.freeze_backbone()``): the backward stops at the extras.
VGG16 has no BatchNorm: (b) is (a) and (c) is (d) there, timed all the same.  After every change of configuration two
untimed steps run (the first re-plans the backward and times the tiles of conv shapes it has not met); every timed window is
>= 1 s of back-to-back steps closed by ONE synchronise.  Reported: median of --rounds windows with min .. max.
Usage: python tests/bench_finetune.py [--rounds 5] [--batch 32] [--nets mobilenet_v2:fp32,mobilenet_v2:bf16,vgg16:fp32]"""
import argparse
import os
import statistics
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import torch
import ssd_hip as h

CONFIGS = [("a", "all trainable"), ("b", "every BatchNorm frozen"), ("c", "backbone convs frozen, BatchNorm on batch statistics"),
           ("d", "backbone and its BatchNorm frozen")]


def configure(model, key):
    model.set_trainable("*", True)
    if key == "b" and model.batch_norm_layer_names():
        model.set_trainable(model.batch_norm_layer_names(), False)
    elif key == "c":
        model.freeze_backbone(batch_norm=False)
    elif key == "d":
        model.freeze_backbone()


def window(fn, min_seconds=1.0):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench_net(backbone, precision, B, rounds):
    from utils import bbox_utils, data_utils, train_utils
    if backbone == "mobilenet_v2":
        from models.ssd_mobilenet_v2 import get_model
    else:
        from models.ssd_vgg16 import get_model
    hp = train_utils.get_hyper_params(backbone)
    hp["total_labels"] = 21                      # VOC: 20 classes + background, as trainer.py sets it
    model = get_model(hp, max_batch=B, precision=precision)
    model.compile(learning_rate=1e-5)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    x = h.to_dev(data_utils.synthetic_images(B, hp["img_size"], seed=0))
    gt, gl = data_utils.synthetic_gt(B, total_labels=hp["total_labels"], seed=3)
    gt, gl = h.to_dev(gt), h.to_dev(gl, torch.int32)

    def step():
        yd, yl = train_utils.calculate_actual_outputs(priors, gt, gl, hp)
        _, _, g = model.forward_backward(x, yd, yl)
        model.apply_gradients(g)
    times = {k: [] for k, _ in CONFIGS}
    for _ in range(rounds):
        for key, _ in CONFIGS:
            configure(model, key)
            step(); step()
            times[key].append(window(step))
    print("SSD300 %s %s training step, B=%d, one GPU; windows >= 1 s, one synchronise each" % (backbone, precision, B))
    base = statistics.median(times["a"])
    for key, text in CONFIGS:
        xs = [1e3 * t for t in times[key]]
        print("  (%s) %-52s %8.3f ms/step (median; min %.3f .. max %.3f, n=%d)  %.2fx of (a)" % (
            key, text, statistics.median(xs), min(xs), max(xs), len(xs), statistics.median(times[key]) / base))
    configure(model, "a")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--nets", default="mobilenet_v2:fp32,mobilenet_v2:bf16,vgg16:fp32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_finetune.py measures on the GPU"
    for net in args.nets.split(","):
        bench_net(net.split(":")[0], net.split(":")[1], args.batch, args.rounds)
