"""Drop-in for the reference's ``trainer.py`` entry point (reference trainer.py:8-76): same
flags and knobs (batch 32, 150 epochs, ``load_weights``), same call order -- hyper-parameters,
data, model, ``compile(Adam(1e-3), [loc_loss_fn, conf_loss_fn])``, ``init_model``, prior boxes,
target-encoding generators, ``fit`` with the three callbacks: ``ModelCheckpoint(monitor=
"val_loss", save_best_only, save_weights_only)``, ``LearningRateScheduler(train_utils.scheduler)``
and a scalar log in place of TensorBoard.

Every step is native: GPU target assignment -> training-mode forward -> HIP loss -> backward ->
(RCCL all-reduce of the flat gradient when launched with torchrun, one rank per GPU) -> Adam.
Data: with ``SSD_VOC_DIR`` set to a directory that holds a VOCdevkit, the reference's own calls run
(trainer.py:27-48): ``get_dataset("voc/2007", "train+validation")`` and ``"test"``, voc/2012 added
when that year is there, ``shuffle(batch_size * 4)``, then ``data_utils.voc_batches`` (threaded
decode, one upload and one resize launch per batch, batched augmentation).  Without it the splits are
seeded synthetic padded batches (``SSD_TRAINER_ITEMS`` training images per epoch, default 512).
``SSD_TRAINER_ITEMS`` / ``SSD_TRAINER_EPOCHS`` / ``SSD_TRAINER_STEPS`` / ``SSD_TRAINER_BATCH`` shorten
a run in both modes (tests, smoke).
Fine-tuning: ``SSD_TRAINER_LOAD_WEIGHTS=1`` sets the reference's own ``load_weights`` switch (the checkpoint at the
model path is loaded before training); ``SSD_TRAINER_FREEZE`` (empty by default) freezes layers first: ``backbone``
(``model.freeze_backbone()``: the backbone with its BatchNorm layers), ``backbone-bn`` (its BatchNorm layers only) or
comma-separated ``fnmatch`` patterns over the Keras layer names (``model.set_trainable``).
Optimizer: ``SSD_TRAINER_OPTIMIZER`` (``adam`` | ``sgd``), ``SSD_TRAINER_MOMENTUM``, ``SSD_TRAINER_NESTEROV``,
``SSD_TRAINER_CLIPNORM``, ``SSD_TRAINER_CLIPVALUE``, ``SSD_TRAINER_GLOBAL_CLIPNORM`` (``optimizer_from_env``); with none
of them set the run is the reference's ``Adam(1e-3)``.
Loss: ``SSD_TRAINER_LOSS`` (``hard`` | ``focal``), ``SSD_TRAINER_FOCAL_ALPHA`` (0.25), ``SSD_TRAINER_FOCAL_GAMMA`` (2.0)
(``loss_from_env``); unset: the reference's hard-negative mining.  ``SSD_TRAINER_FOCAL_PRIOR`` (off by default) = pi
writes the prior-probability bias into the label heads after ``init_model`` (``model.set_conf_prior``).
``SSD_TRAINER_LOC_LOSS`` (``huber`` | ``iou`` | ``giou`` | ``diou`` | ``ciou``, ``loc_loss_from_env``) puts an IoU-family loss on
the decoded boxes in place of the Huber localisation term of either; unset: the reference's Huber term.
Target assignment: ``SSD_TRAINER_MATCH`` (``max_iou`` | ``bipartite`` | ``atss``) and ``SSD_TRAINER_MATCH_TOPK`` (atss, default 9)
(``match_from_env``); unset: the reference's threshold rule.
Mosaic: ``SSD_TRAINER_MOSAIC`` = the probability that a training image becomes a mosaic of four images of its batch, in front
of the reference's augmentation, and ``SSD_TRAINER_MOSAIC_SCALE`` = ``lo,hi`` (default ``0.5,1.0``) (``mosaic_from_env``); unset,
empty or 0: no mosaic, the feed is unchanged.  Mosaic needs ``SSD_TRAINER_AUGMENT=gpu`` (or ``0``): a mosaic may keep no box, and the
host draws' window sampler raises on an image without one.  """
import json
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import parallel  # noqa: E402
import ssd_hip  # noqa: E402
from ssd_loss import CustomLoss, FocalLoss, IoULocLoss  # noqa: E402
from utils import bbox_utils, data_utils, io_utils, train_utils, voc_utils  # noqa: E402

with_voc_2012 = True


def _voc_splits(voc_dir, batch_size, rank, world):
    """reference trainer.py:27-38 on the devkit under ``voc_dir`` -> (train dataset, validation dataset, info, training
    items, validation items); ``SSD_TRAINER_ITEMS`` caps the training items (and the validation items as in the
    synthetic mode), every rank reads its own shard."""
    train_data, info = data_utils.get_dataset("voc/2007", "train+validation", voc_dir)
    val_data, _ = data_utils.get_dataset("voc/2007", "test", voc_dir)
    train_total_items = data_utils.get_total_item_size(info, "train+validation")
    val_total_items = data_utils.get_total_item_size(info, "test")
    if with_voc_2012 and voc_utils.has_year(voc_dir, "voc/2012"):
        voc_2012_data, voc_2012_info = data_utils.get_dataset("voc/2012", "train+validation", voc_dir)
        train_total_items += data_utils.get_total_item_size(voc_2012_info, "train+validation")
        train_data = train_data.concatenate(voc_2012_data)
    if world > 1:
        train_data, val_data = train_data.shard(world, rank), val_data.shard(world, rank)
        train_total_items, val_total_items = len(train_data), len(val_data)
    cap = int(os.environ.get("SSD_TRAINER_ITEMS", "0"))
    if cap:
        train_total_items = min(train_total_items, cap)
        val_total_items = min(val_total_items, max(batch_size, train_total_items // 8))
        train_data, val_data = train_data.take(train_total_items), val_data.take(val_total_items)
    return train_data, val_data, info, train_total_items, val_total_items


def fit(model, train_feed, steps_per_epoch, val_feed, validation_steps, epochs, model_path, log_path, rank=0):
    """Keras ``Model.fit`` with the reference's callbacks (trainer.py:65-76): per epoch the
    LearningRateScheduler sets the rate, ``steps_per_epoch`` optimisation steps run, then
    ``validation_steps`` validation batches; the weights are saved whenever ``val_loss`` improves."""
    history = {"loss": [], "loc_loss": [], "conf_loss": [], "val_loss": [], "lr": []}
    best = float("inf")
    log = None
    if rank == 0 and log_path:
        os.makedirs(log_path, exist_ok=True)
        log = open(os.path.join(log_path, "scalars.jsonl"), "w")     # TensorBoard callback stand-in
    for epoch in range(epochs):
        lr = train_utils.scheduler(epoch)
        t0 = time.perf_counter()
        tot = loc = conf = 0.0
        for _ in range(steps_per_epoch):
            img, targets = next(train_feed)
            l, a, b = model.train_on_batch(img, targets, learning_rate=lr)
            tot += l; loc += a; conf += b
        n = max(steps_per_epoch, 1)
        vtot = 0.0
        for _ in range(validation_steps):
            img, targets = next(val_feed)
            vtot += model.evaluate_on_batch(img, targets)[0]
        val = parallel.mean_over_ranks(vtot / max(validation_steps, 1))
        rec = {"epoch": epoch, "loss": tot / n, "loc_loss": loc / n, "conf_loss": conf / n, "val_loss": val, "lr": lr}
        for k in history:
            history[k].append(rec[k])
        if rank == 0:
            print("Epoch %d/%d - %.1fs - loss: %.4f - loc_loss: %.4f - conf_loss: %.4f - val_loss: %.4f - lr: %.0e" % (
                epoch + 1, epochs, time.perf_counter() - t0, rec["loss"], rec["loc_loss"], rec["conf_loss"], val, lr),
                flush=True)
            if log:
                log.write(json.dumps(rec) + "\n")
                log.flush()
            if val < best:          # ModelCheckpoint(monitor="val_loss", save_best_only=True, save_weights_only=True)
                model.save_weights(model_path)
        best = min(best, val)
    if log:
        log.close()
    return history


def freeze_layers(model, spec):
    """``SSD_TRAINER_FREEZE``: ``backbone``, ``backbone-bn`` (the backbone's BatchNorm layers only) or comma-separated
    ``fnmatch`` patterns over the Keras layer names -> the names frozen."""
    if spec == "backbone":
        return model.freeze_backbone()
    if spec == "backbone-bn":
        bn = set(model.batch_norm_layer_names())
        return model.set_trainable([n for n in model.backbone_layer_names() if n in bn], False)
    return model.set_trainable([p.strip() for p in spec.split(",") if p.strip()], False)


def optimizer_from_env():
    """``SSD_TRAINER_OPTIMIZER`` = ``adam`` (default) | ``sgd``, ``SSD_TRAINER_MOMENTUM`` (sgd: default 0.9, SSD's classic
    setting), ``SSD_TRAINER_NESTEROV=1``, ``SSD_TRAINER_CLIPNORM`` / ``SSD_TRAINER_CLIPVALUE`` /
    ``SSD_TRAINER_GLOBAL_CLIPNORM`` -> an ``optimizers`` instance at the reference's rate 1e-3 (the LearningRateScheduler
    sets the rate of every epoch anyway), or None when none of them is set: the run is then the reference's Adam."""
    import optimizers
    env = os.environ
    names = ("OPTIMIZER", "MOMENTUM", "NESTEROV", "CLIPNORM", "CLIPVALUE", "GLOBAL_CLIPNORM")
    if not any(env.get("SSD_TRAINER_" + n, "").strip() for n in names):
        return None
    kind = env.get("SSD_TRAINER_OPTIMIZER", "adam").strip().lower() or "adam"
    clips = {k.lower(): float(env["SSD_TRAINER_" + k]) for k in ("CLIPNORM", "CLIPVALUE", "GLOBAL_CLIPNORM")
             if env.get("SSD_TRAINER_" + k, "").strip()}
    if kind == "adam":
        return optimizers.Adam(learning_rate=1e-3, **clips)
    if kind == "sgd":
        return optimizers.SGD(learning_rate=1e-3, momentum=float(env.get("SSD_TRAINER_MOMENTUM", "").strip() or 0.9),
                              nesterov=env.get("SSD_TRAINER_NESTEROV", "0").strip() == "1", **clips)
    raise ValueError("SSD_TRAINER_OPTIMIZER must be 'adam' or 'sgd', got %r" % kind)


def loss_from_env(hyper_params):
    """``SSD_TRAINER_LOSS`` = ``hard`` (default: the reference's ``CustomLoss(neg_pos_ratio, loc_loss_alpha)``) | ``focal``
    (``FocalLoss(loc_loss_alpha, SSD_TRAINER_FOCAL_ALPHA or 0.25, SSD_TRAINER_FOCAL_GAMMA or 2.0)``).  ValueError for another
    kind, for a number that does not parse or lies outside its range, and for a focal knob set beside the mining loss."""
    env = os.environ
    kind = env.get("SSD_TRAINER_LOSS", "").strip().lower() or "hard"
    knobs = {k: env.get("SSD_TRAINER_FOCAL_" + k, "").strip() for k in ("ALPHA", "GAMMA")}
    if kind == "hard":
        used = sorted("SSD_TRAINER_FOCAL_" + k for k, v in knobs.items() if v)
        if used:
            raise ValueError("%s set, but SSD_TRAINER_LOSS is not 'focal'" % ", ".join(used))
        return CustomLoss(hyper_params["neg_pos_ratio"], hyper_params["loc_loss_alpha"])
    if kind == "focal":
        return FocalLoss(hyper_params["loc_loss_alpha"], alpha=knobs["ALPHA"] or 0.25, gamma=knobs["GAMMA"] or 2.0)
    raise ValueError("SSD_TRAINER_LOSS must be 'hard' or 'focal', got %r" % kind)


def loc_loss_from_env(base, prior_boxes, hyper_params):
    """``SSD_TRAINER_LOC_LOSS`` = ``huber`` (default: ``base`` itself, the Huber term of the reference) | ``iou`` | ``giou`` |
    ``diou`` | ``ciou`` (``IoULocLoss(base, prior_boxes, hyper_params["variances"], mode)``: that loss on the decoded boxes,
    ``base``'s confidence term).  ValueError for anything else."""
    mode = os.environ.get("SSD_TRAINER_LOC_LOSS", "").strip().lower() or "huber"
    if mode == "huber":
        return base
    if mode in ("iou", "giou", "diou", "ciou"):
        return IoULocLoss(base, prior_boxes, hyper_params["variances"], mode=mode)
    raise ValueError("SSD_TRAINER_LOC_LOSS must be 'huber', 'iou', 'giou', 'diou' or 'ciou', got %r" % mode)


def match_from_env(hyper_params):
    """``SSD_TRAINER_MATCH`` = ``max_iou`` (default: the reference's rule, ``hyper_params`` untouched) | ``bipartite`` |
    ``atss`` (``match_strategy``); ``SSD_TRAINER_MATCH_TOPK`` (atss only, 1..64, default 9: ``match_topk``).  Returns the
    hyper-parameters ``train_utils.calculate_actual_outputs`` is to read: a COPY with those keys for another strategy than the
    default (``hyper_params`` is the module-level table of ``train_utils``, which must not gain keys), ``hyper_params`` itself
    otherwise.  ValueError for another strategy, for a top-k that does not parse or lies outside its range, and for a top-k
    set beside a strategy that ignores it."""
    env = os.environ
    kind = env.get("SSD_TRAINER_MATCH", "").strip().lower() or "max_iou"
    topk = env.get("SSD_TRAINER_MATCH_TOPK", "").strip()
    if kind not in ssd_hip.MATCH_STRATEGIES:
        raise ValueError("SSD_TRAINER_MATCH must be 'max_iou', 'bipartite' or 'atss', got %r" % kind)
    if kind != "atss":
        if topk:
            raise ValueError("SSD_TRAINER_MATCH_TOPK set, but SSD_TRAINER_MATCH is not 'atss'")
        return hyper_params if kind == "max_iou" else dict(hyper_params, match_strategy=kind)
    try:
        k = int(topk or 9)
    except ValueError:
        k = 0
    if not 1 <= k <= ssd_hip.MATCH_MAX_TOPK:
        raise ValueError("SSD_TRAINER_MATCH_TOPK must be an integer in 1..%d, got %r" % (ssd_hip.MATCH_MAX_TOPK, topk))
    return dict(hyper_params, match_strategy=kind, match_topk=k)


def mosaic_from_env():
    """``SSD_TRAINER_MOSAIC`` = the probability that a training image is a mosaic of its batch (``augmentation.mosaicked``);
    ``SSD_TRAINER_MOSAIC_SCALE`` = ``"lo,hi"``, the tiles' scale range (default ``0.5,1.0``).  Returns None when the
    probability is unset, empty or 0 -- no wrapper, no launch: the feed is the one without the knob -- and ``(p, (lo, hi))``
    otherwise.  ValueError for a probability that does not parse or lies outside [0, 1], for a scale that is not two numbers
    with 0.1 <= lo <= hi <= 2, for a scale set without mosaic, and for mosaic beside the host draws of the augmentation
    (``SSD_TRAINER_AUGMENT`` anything but ``gpu`` or ``0``): a mosaic may keep no ground-truth row, and ``apply_batch``'s sampler
    raises on such an image, like TF's; the device plan gives it no patch instead."""
    env = os.environ
    raw, raw_scale = env.get("SSD_TRAINER_MOSAIC", "").strip(), env.get("SSD_TRAINER_MOSAIC_SCALE", "").strip()
    try:
        p = float(raw or 0)
    except ValueError:
        p = -1.0
    if not 0.0 <= p <= 1.0:
        raise ValueError("SSD_TRAINER_MOSAIC must be a probability in [0, 1], got %r" % raw)
    if p == 0.0:
        if raw_scale:
            raise ValueError("SSD_TRAINER_MOSAIC_SCALE set, but SSD_TRAINER_MOSAIC is not")
        return None
    try:
        lo, hi = (float(v) for v in (raw_scale or "0.5,1.0").split(","))
    except ValueError:
        lo, hi = 0.0, 0.0
    if not 0.1 <= lo <= hi <= 2.0:
        raise ValueError("SSD_TRAINER_MOSAIC_SCALE must be 'lo,hi' with 0.1 <= lo <= hi <= 2, got %r" % raw_scale)
    if env.get("SSD_TRAINER_AUGMENT", "1") not in ("gpu", "0"):
        raise ValueError("SSD_TRAINER_MOSAIC needs SSD_TRAINER_AUGMENT=gpu (or 0): a mosaic may keep no ground-truth row, which "
                         "the host draws' window sampler refuses; got SSD_TRAINER_AUGMENT=%r" % env.get("SSD_TRAINER_AUGMENT", "1"))
    return p, (lo, hi)


def voc_training_batches(train_data, batch_size, img_size, rank, augment, augment_gpu, mosaic):
    """The training stream of the VOC road (reference trainer.py:42-48: preprocessing + augmentation, shuffle, padded batches).
    Without mosaic the augmentation runs inside ``voc_batches``; with it ``voc_batches`` only resizes, ``mosaicked`` wraps it
    and ``augmented`` wraps that, so the reference's augmentation treats a mosaic like any image."""
    import augmentation
    if augment and not augment_gpu:
        augmentation.seed(4242 + rank)
    augmentation_fn = augmentation.device_draws(4242, rank_offset=rank << 40) if augment_gpu else augmentation.apply_batch
    shuffled = train_data.shuffle(batch_size * 4, seed=rank)
    if mosaic is None:
        return data_utils.voc_batches(shuffled, batch_size, img_size, img_size, augmentation_fn=augmentation_fn if augment else None)
    batches = data_utils.voc_batches(shuffled, batch_size, img_size, img_size, augmentation_fn=None)
    batches = augmentation.mosaicked(batches, mosaic[0], 4242, rank_offset=rank << 40, scale=mosaic[1])
    return augmentation.augmented(batches, augmentation_fn) if augment else batches


def main(argv=None):
    args = io_utils.handle_args(argv)
    if args.handle_gpu:
        io_utils.handle_gpu_compatibility()
    rank, _, world = parallel.init_distributed()

    batch_size = int(os.environ.get("SSD_TRAINER_BATCH", "32"))
    epochs = int(os.environ.get("SSD_TRAINER_EPOCHS", "150"))
    load_weights = os.environ.get("SSD_TRAINER_LOAD_WEIGHTS", "0") == "1"
    backbone = args.backbone
    io_utils.is_valid_backbone(backbone)
    if backbone == "mobilenet_v2":
        from models.ssd_mobilenet_v2 import get_model, init_model
    else:
        from models.ssd_vgg16 import get_model, init_model
    hyper_params = train_utils.get_hyper_params(backbone)
    voc_dir = os.environ.get("SSD_VOC_DIR")
    mosaic = mosaic_from_env()
    if mosaic is not None and rank == 0:
        print("mosaic: p %g, scale %g..%g" % (mosaic[0], mosaic[1][0], mosaic[1][1]), flush=True)
    augment = os.environ.get("SSD_TRAINER_AUGMENT", "1") != "0"
    # SSD_TRAINER_AUGMENT=gpu: the random plan is drawn on the device (augmentation.device_draws: a counter-based
    # generator, every rank numbers its images in a range of its own); any other value but 0 keeps the host draws
    augment_gpu = os.environ.get("SSD_TRAINER_AUGMENT", "1") == "gpu"
    if voc_dir:
        train_data, val_data, info, train_total_items, val_total_items = _voc_splits(voc_dir, batch_size, rank, world)
        labels = ["bg"] + data_utils.get_labels(info)
        hyper_params["total_labels"] = len(labels)
        img_size = hyper_params["img_size"]
        step_size_train = int(os.environ.get("SSD_TRAINER_STEPS", "0")) or train_utils.get_step_size(train_total_items, batch_size)
        step_size_val = train_utils.get_step_size(val_total_items, batch_size)
        train_data = voc_training_batches(train_data, batch_size, img_size, rank, augment, augment_gpu, mosaic)
        val_data = data_utils.voc_batches(val_data, batch_size, img_size, img_size)
        augment = False                                   # done inside the batches
    else:
        labels = ["bg"] + data_utils.get_labels()
        hyper_params["total_labels"] = len(labels)
        img_size = hyper_params["img_size"]

        train_total_items = int(os.environ.get("SSD_TRAINER_ITEMS", "512"))
        val_total_items = max(batch_size, train_total_items // 8)
        step_size_train = int(os.environ.get("SSD_TRAINER_STEPS", "0")) or train_utils.get_step_size(train_total_items, batch_size)
        step_size_val = min(2, train_utils.get_step_size(val_total_items, batch_size))
        # every rank draws its own shard of the synthetic stream (batch data-parallel)
        train_data = list(data_utils.synthetic_dataset(step_size_train * batch_size, batch_size, img_size, len(labels),
                                                       seed=1000 * rank))
        val_data = list(data_utils.synthetic_dataset(step_size_val * batch_size, batch_size, img_size, len(labels),
                                                     seed=777 + 1000 * rank))

    target_params = match_from_env(hyper_params)
    if target_params is not hyper_params and rank == 0:
        print("target assignment: %s%s" % (target_params["match_strategy"],
                                           " (top-k %d)" % target_params["match_topk"] if "match_topk" in target_params else ""),
              flush=True)
    ssd_model = get_model(hyper_params, max_batch=batch_size)
    prior_boxes = bbox_utils.generate_prior_boxes(hyper_params["feature_map_shapes"], hyper_params["aspect_ratios"])
    ssd_custom_losses = loc_loss_from_env(loss_from_env(hyper_params), prior_boxes, hyper_params)
    optimizer = optimizer_from_env()
    ssd_model.compile(optimizer=optimizer, learning_rate=1e-3, loss=[ssd_custom_losses.loc_loss_fn, ssd_custom_losses.conf_loss_fn])
    if optimizer is not None and rank == 0:
        print("optimizer: %r" % (optimizer,), flush=True)
    if isinstance(ssd_custom_losses, (FocalLoss, IoULocLoss)) and rank == 0:
        print("loss: %r" % (ssd_custom_losses,), flush=True)
    init_model(ssd_model)
    focal_prior = os.environ.get("SSD_TRAINER_FOCAL_PRIOR", "").strip()
    if focal_prior:
        try:
            pi = float(focal_prior)
        except ValueError:
            raise ValueError("SSD_TRAINER_FOCAL_PRIOR must be a number in (0, 1), got %r" % focal_prior)
        ssd_model.set_conf_prior(pi)
        if rank == 0:
            print("label heads: prior probability %g" % pi, flush=True)
    ssd_model_path = io_utils.get_model_path(backbone)
    if load_weights:
        ssd_model.load_weights(ssd_model_path)
    freeze = os.environ.get("SSD_TRAINER_FREEZE", "").strip()
    if freeze:
        frozen = freeze_layers(ssd_model, freeze)
        if rank == 0:
            print("frozen: %d layers (%s)" % (len(frozen), freeze), flush=True)
    ssd_log_path = io_utils.get_log_path(backbone)
    # reference trainer.py:42: the TRAINING stream is augmented (fresh draws every epoch), the validation stream is not.
    # SSD_TRAINER_AUGMENT=0 turns it off (deterministic smoke runs).
    if mosaic is not None and not voc_dir:          # SSD_TRAINER_MOSAIC: in front of the augmentation (the VOC road did it above)
        import augmentation
        train_data = augmentation.mosaicked(train_data, mosaic[0], 4242, rank_offset=rank << 40, scale=mosaic[1])
    if augment:
        import augmentation
        if augment_gpu:
            train_data = augmentation.augmented(train_data, augmentation.device_draws(4242, rank_offset=rank << 40))
        else:
            augmentation.seed(4242 + rank)
            train_data = augmentation.augmented(train_data)
    ssd_train_feed = train_utils.generator(train_data, prior_boxes, target_params)
    ssd_val_feed = train_utils.generator(val_data, prior_boxes, target_params)

    return fit(ssd_model, ssd_train_feed, step_size_train, ssd_val_feed, step_size_val, epochs, ssd_model_path,
               ssd_log_path, rank)


if __name__ == "__main__":
    main()
