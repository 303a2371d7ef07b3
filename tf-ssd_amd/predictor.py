"""Host-side mirror of the reference's ``predictor.py`` (predictor.py:5-57): the same CLI
(``-handle-gpu``, ``--backbone``), the same knobs (batch 32, ``evaluate`` switch, "bg" + VOC
labels) and the same call order -- hyper-parameters, model, weights, priors, decoder model,
``predict`` over the test split, optional VOC07 mAP, optional drawing (``draw=True``: ``drawing_utils.draw_predictions``
on the GPU, PNGs into ``draw_dir``, or JPEGs with ``draw_format="jpeg"``: forward DCT on the GPU, Huffman coding on the
data pool's threads).

Data: with ``SSD_VOC_DIR`` set to a directory that holds a VOCdevkit, the reference's own calls run
(predictor.py:22-25, 40-43): ``get_dataset("voc/2007", "test")``, ``get_total_item_size``,
``get_labels(info)``, then ``data_utils.voc_batches`` (threaded decode, one upload and one resize launch
per batch); ``SSD_SYNTHETIC_ITEMS``, when set, caps the items.  The preprocessed split is held on the
device, since ``predict`` and then ``evaluate_predictions`` / ``draw_predictions`` walk it: 1.08 MB per
image at 300x300, 5.3 GB for the 4952 images of VOC2007 test (15.6 GB at 512x512).  Without the variable
the test split is a seeded synthetic stand-in for its items (``SSD_SYNTHETIC_ITEMS`` uint8 images of
VOC-like sizes with boxes / labels / difficult flags, default 128) that goes through the same ``preprocessing`` (GPU convert + bilinear
resize) -> padded batches -> ``predict`` -> optional ``evaluate_predictions``; ``use_custom_images`` reads
``custom_image_path`` like the reference (PIL decodes; the LANCZOS resize, Pillow's bit for bit, and the float
conversion run on the GPU, one upload and one ``ssd_resize_lanczos`` call per batch: ``data_utils.custom_data_batches``);
trained weights are loaded when ``trained/ssd_<backbone>_model_weights.h5`` exists, otherwise
seeded synthetic weights are used and that is said on stdout."""
import os
import sys
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import ssd_hip  # noqa: E402
ssd_hip.configure_serving()        # the serving entry point opts in to three lanes / three hardware queues before the runtime starts
from utils import bbox_utils, data_utils, drawing_utils, eval_utils, io_utils, train_utils  # noqa: E402
from models.decoder import get_decoder_model  # noqa: E402

# the reference's script-level knobs (predictor.py:9-12), same names and defaults
batch_size = 32
evaluate = False
use_custom_images = False
custom_image_path = "data/images/"
# additions: the reference always draws when it does not evaluate (and blocks in plt.show()); here drawing is opt-in and
# writes draw_dir/img_%05d.png when draw_dir is set (draw_format "jpeg": img_%05d.jpg at quality draw_quality)
draw = False
draw_dir = None
draw_format = "png"
draw_quality = 75
# additions: eval_protocol "voc07" / "voc10" / "coco" scores by the devkit's / pycocotools' rules (DecoderModel.evaluate on the
# split built with keep_difficult=True) instead of the reference's; eval_score_threshold replaces the decoder's 0.5 (the
# protocols are meant to be run at a low threshold, e.g. 0.01: 0.5 cuts the precision-recall curve short)
eval_protocol = None
eval_score_threshold = None
# additions: the decoder's suppression (models/decoder.py SSDDecoder), with and without evaluate; None keeps the reference's
# (hard, per class, IoU 0.5).  nms_method "hard" / "gaussian" / "linear" (Soft-NMS; nms_sigma is TF's soft_nms_sigma),
# nms_class_agnostic True: one list per image, a box comes out under one class only
nms_method = None
nms_sigma = None
nms_iou_threshold = None
nms_class_agnostic = None


def _model_factory(backbone):
    if backbone == "mobilenet_v2":
        from models.ssd_mobilenet_v2 import get_model
    else:
        from models.ssd_vgg16 import get_model
    return get_model


def _load_or_synthesise_weights(model, backbone):
    path = io_utils.get_model_path(backbone)
    if os.path.exists(path):
        model.load_weights(path)
    else:
        print("no trained weights at %s: using seeded synthetic weights" % path)
        data_utils.synthetic_weights(model)


def main(argv=None, **knobs):
    """``knobs`` override the module-level switches for one call (``evaluate``, ``use_custom_images``,
    ``custom_image_path``, ``batch_size``, ``draw``, ``draw_dir``, ``draw_format``, ``draw_quality``, ``eval_protocol``,
    ``eval_score_threshold``, ``nms_method``, ``nms_sigma``, ``nms_iou_threshold``, ``nms_class_agnostic``).  With ``evaluate`` and an ``eval_protocol`` the fourth return value is
    ``DetectionEvaluator.result()``."""
    args = io_utils.handle_args(argv)
    if args.handle_gpu:
        io_utils.handle_gpu_compatibility()
    io_utils.is_valid_backbone(args.backbone)
    bs = int(knobs.get("batch_size", batch_size))
    do_eval = bool(knobs.get("evaluate", evaluate))
    custom = bool(knobs.get("use_custom_images", use_custom_images))
    custom_path = knobs.get("custom_image_path", custom_image_path)
    do_draw = bool(knobs.get("draw", draw))
    out_dir = knobs.get("draw_dir", draw_dir)
    out_format = knobs.get("draw_format", draw_format)
    out_quality = int(knobs.get("draw_quality", draw_quality))
    protocol = knobs.get("eval_protocol", eval_protocol) if do_eval else None
    score_thr = knobs.get("eval_score_threshold", eval_score_threshold)
    if protocol is not None:
        eval_utils.protocol_spec(protocol)                # an unknown name fails before anything is built
    keep = protocol is not None
    if out_format not in ("png", "jpeg"):
        raise ValueError('draw_format must be "png" or "jpeg", got %r' % (out_format,))

    labels = ["bg"] + data_utils.get_labels()
    hyper_params = train_utils.get_hyper_params(args.backbone)
    hyper_params["total_labels"] = len(labels)
    img_size = hyper_params["img_size"]
    padding_values = data_utils.get_padding_values()

    if custom:                                            # predictor.py:35-39
        img_paths = data_utils.get_custom_imgs(custom_path)
        total_items = len(img_paths)
        test_data = list(data_utils.custom_data_batches(img_paths, img_size, img_size, bs))
    elif os.environ.get("SSD_VOC_DIR"):                   # predictor.py:22-25, 40-43
        test_data, info = data_utils.get_dataset("voc/2007", "test", os.environ["SSD_VOC_DIR"])
        total_items = data_utils.get_total_item_size(info, "test")
        labels = ["bg"] + data_utils.get_labels(info)
        if os.environ.get("SSD_SYNTHETIC_ITEMS"):
            total_items = min(total_items, int(os.environ["SSD_SYNTHETIC_ITEMS"]))
            test_data = test_data.take(total_items)
        # materialised like the synthetic split below: predict() and evaluate_predictions() / draw_predictions() both
        # walk it (1.08 MB of device memory per 300x300 image: 5.3 GB for all of VOC2007 test)
        test_data = list(data_utils.voc_batches(test_data, bs, img_size, img_size, evaluate=do_eval, keep_difficult=keep))
    else:                                                 # no devkit: a synthetic stand-in for voc/2007 test
        total_items = int(os.environ.get("SSD_SYNTHETIC_ITEMS", "128"))
        raw = data_utils.synthetic_voc_items(total_items, len(labels))
        items = (data_utils.preprocessing(x, img_size, img_size, evaluate=do_eval, keep_difficult=keep) for x in raw)
        # predictor.py:43 -- materialised: predict() and evaluate_predictions() both walk it
        test_data = list(data_utils.padded_batch(items, bs, padding_values))

    ssd_model = _model_factory(args.backbone)(hyper_params, max_batch=bs)
    _load_or_synthesise_weights(ssd_model, args.backbone)
    prior_boxes = bbox_utils.generate_prior_boxes(hyper_params["feature_map_shapes"], hyper_params["aspect_ratios"])
    ssd_decoder_model = get_decoder_model(ssd_model, prior_boxes, hyper_params, score_threshold=score_thr,
                                          iou_threshold=knobs.get("nms_iou_threshold", nms_iou_threshold),
                                          nms_method=knobs.get("nms_method", nms_method),
                                          soft_nms_sigma=knobs.get("nms_sigma", nms_sigma),
                                          class_agnostic=knobs.get("nms_class_agnostic", nms_class_agnostic))

    t0 = time.perf_counter()
    boxes, classes, scores = ssd_decoder_model.predict(
        test_data, steps=train_utils.get_step_size(total_items, bs), verbose=1)
    dt = time.perf_counter() - t0
    print("predicted %d images in %.3f s (%.1f images/sec incl. host transfers); mean detections/image %.1f" % (
        boxes.shape[0], dt, boxes.shape[0] / max(dt, 1e-9), float((classes > 0).sum(-1).mean()) if boxes.shape[0] else 0.0))

    if protocol is not None:
        result, mean_ap = ssd_decoder_model.evaluate(test_data, labels, steps=train_utils.get_step_size(total_items, bs),
                                                     protocol=protocol)
        print("mAP ({}): {}".format(protocol, float(mean_ap)))
        if protocol == "coco":
            print("AP50: {}".format(result["AP50"]))
            print("AP75: {}".format(result["AP75"]))
        return boxes, classes, scores, result
    if do_eval:                                           # predictor.py:54-55
        stats = eval_utils.evaluate_predictions(test_data, boxes, classes, scores, labels, bs)
        return boxes, classes, scores, stats
    if do_draw:                                           # predictor.py:56-57, on the GPU; files instead of plt.show()
        for _ in drawing_utils.draw_predictions(test_data, boxes, classes, scores, labels, bs, out_dir=out_dir,
                                                out_format=out_format, out_quality=out_quality):
            pass
    return boxes, classes, scores


if __name__ == "__main__":
    main()
