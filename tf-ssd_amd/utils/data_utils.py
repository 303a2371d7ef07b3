"""Data side of the drop-in.  The reference's ``utils/data_utils.py`` loads PASCAL VOC via
tensorflow_datasets and converts / resizes every image with TF ops; here ``get_dataset`` reads a
VOCdevkit directory from disk (``utils/voc_utils.py``; without one it raises as before),
``preprocessing`` runs that conversion + bilinear resize as one HIP kernel,
``voc_batches`` does it for a whole ragged batch per launch (``ssd_preprocess_ragged``) behind a
decoding thread pool, and custom images -- PIL + LANCZOS in the reference -- are only decoded by
PIL: the resize is Pillow's 8-bit resampler restated as HIP kernels (``ssd_resize_lanczos``), a
ragged batch per call.  Also kept: the VOC label list, the padded-batch conventions (gt boxes
padded with 0, labels with -1), and seeded synthetic generators shaped like the reference's
batches."""
import functools
import math

import numpy as np

from . import voc_utils
from .voc_utils import VOC_LABELS  # noqa: F401  (the 20 class names, alphabetical)


def preprocessing(image_data, final_height, final_width, augmentation_fn=None, evaluate=False, keep_difficult=False):
    """reference utils/data_utils.py:7-30: uint8 image -> float32 [0,1] resized (bilinear) to
    ``(final_height, final_width)`` ON THE GPU (``ssd_preprocess``: one kernel, no float copy of
    the original image), labels shifted by +1 (0 is the background), difficult objects dropped when
    ``evaluate``.  ``image_data`` is the tfds-style dict ``{"image": uint8 [H,W,3], "objects":
    {"bbox": [G,4], "label": [G], "is_difficult": [G]}}``.  Returns (img device tensor, gt_boxes,
    gt_labels).  ``keep_difficult`` (not in the reference; for the devkit / COCO protocols of
    ``eval_utils.DetectionEvaluator``): no object is dropped, whatever ``evaluate`` says, and a fourth item
    ``gt_difficult`` (uint8 [G]) is returned."""
    import torch
    import ssd_hip as _h
    img = image_data["image"]
    img = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(img))
    if img.dtype != torch.uint8 or img.dim() != 3:
        raise ValueError("image must be uint8 [H,W,C], got %s %s" % (img.dtype, tuple(img.shape)))
    src = img.to(_h.device()).contiguous()
    H, W, C = src.shape
    out = torch.empty((int(final_height), int(final_width), C), dtype=torch.float32, device=src.device)
    _h.check(_h.lib().ssd_preprocess(_h.ptr(src), 1, H, W, C, int(final_height), int(final_width), _h.ptr(out),
                                     _h.stream()), "preprocessing")
    gt_boxes, gt_labels = _ground_truth(image_data, evaluate and not keep_difficult)
    if augmentation_fn:
        out, gt_boxes = augmentation_fn(out, gt_boxes)
    if keep_difficult:
        return out, gt_boxes, gt_labels, _difficult(image_data)
    return out, gt_boxes, gt_labels


def _ground_truth(image_data, evaluate):
    """``preprocessing``'s ground truth of one item: float32 boxes, labels + 1 as int32, difficult objects dropped
    when ``evaluate``."""
    gt_boxes = np.asarray(image_data["objects"]["bbox"], np.float32)
    gt_labels = (np.asarray(image_data["objects"]["label"]) + 1).astype(np.int32)
    if evaluate:
        not_diff = np.logical_not(np.asarray(image_data["objects"]["is_difficult"], bool))
        gt_boxes, gt_labels = gt_boxes[not_diff], gt_labels[not_diff]
    return gt_boxes, gt_labels


def _difficult(image_data):
    """The difficult flags of one item's objects as uint8 [G], in the order of its boxes."""
    return np.asarray(image_data["objects"]["is_difficult"], bool).astype(np.uint8).reshape(-1)


def _pad_flags(flags, width):
    """``padded_batch``'s fourth item: uint8 flag vectors padded with 0 to ``width``."""
    out = np.zeros((len(flags), width), np.uint8)
    for i, f in enumerate(flags):
        out[i, :len(f)] = np.asarray(f, np.uint8)
    return out


def preprocess_batch(images_u8, final_height, final_width):
    """A batch of same-sized uint8 images [B,H,W,3] -> float32 [B,final_height,final_width,3] in one launch."""
    import torch
    import ssd_hip as _h
    x = images_u8 if isinstance(images_u8, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(images_u8))
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError("images must be uint8 [B,H,W,C]")
    x = x.to(_h.device()).contiguous()
    B, H, W, C = x.shape
    out = torch.empty((B, int(final_height), int(final_width), C), dtype=torch.float32, device=x.device)
    _h.check(_h.lib().ssd_preprocess(_h.ptr(x), B, H, W, C, int(final_height), int(final_width), _h.ptr(out),
                                     _h.stream()), "preprocess_batch")
    return out


def get_labels(info=None):
    """reference utils/data_utils.py:61-69: ``info.features["labels"].names`` of a tfds info object; without one
    (tfds is not available here) the 20 VOC class names the reference's datasets carry."""
    if info is not None and hasattr(info, "features"):
        return info.features["labels"].names
    return list(VOC_LABELS)


def get_dataset(name, split, data_dir="~/tensorflow_datasets"):
    """reference utils/data_utils.py:32-45.  tfds is not available in this build: ``voc/2007`` and ``voc/2012`` are read
    from a VOCdevkit directory under ``data_dir`` (``voc_utils.get_dataset``: a lazy ``VocDataset`` and an info object
    ``get_total_item_size`` / ``get_labels`` accept); without that directory this raises ``RuntimeError`` as it always
    did, naming the path it looked for.  Nothing is downloaded."""
    assert split in ["train", "train+validation", "validation", "test"]
    return voc_utils.get_dataset(name, split, data_dir)


def get_total_item_size(info, split):
    """reference utils/data_utils.py:47-59.  ``info``: a tfds info object (``info.splits[name].num_examples``, the
    reference's argument), or -- tfds is not available here -- a dict ``{"splits": {name: count}}`` or an int."""
    assert split in ["train", "train+validation", "validation", "test"]
    if isinstance(info, int):
        return info
    splits = info.splits if hasattr(info, "splits") else info["splits"]

    def count(name):
        v = splits[name]
        return v.num_examples if hasattr(v, "num_examples") else v
    if split == "train+validation":
        return count("train") + count("validation")
    return count(split)


def get_custom_imgs(custom_image_path):
    """reference utils/data_utils.py:80-91: the files directly inside ``custom_image_path`` (no recursion)."""
    import os
    img_paths = []
    for path, _dirs, filenames in os.walk(custom_image_path):
        for filename in sorted(filenames):
            img_paths.append(os.path.join(path, filename))
        break
    return img_paths


@functools.lru_cache(maxsize=4096)
def lanczos_coefficients(in_size, out_size):
    """[3P] The fixed-point tables of Pillow's 8-bit LANCZOS resampler for one axis (Resample.c ``precompute_coeffs`` +
    ``normalize_coeffs_8bpc``), computed in float64 in Pillow's order: ``scale = in / out``, ``fs = max(scale, 1)``,
    ``support = 3 fs``, ``ksize = ceil(support) * 2 + 1``; for output ``i``: ``center = (i + 0.5) scale``, ``xmin =
    max(int(center - support + 0.5), 0)``, ``xmax = min(int(center + support + 0.5), in) - xmin``, ``w[x] = L((x + xmin -
    center + 0.5) * (1 / fs))`` with ``L(t) = sinc(t) sinc(t / 3)`` on ``-3 <= t < 3``, normalised by the running sum in index
    order, then ``k = (int)(+-0.5 + w * 2**22)``.  Returns read-only ``(bounds [out,2] int32 = (xmin, xmax), k
    [out,ksize] int32)``; host only, cached per ``(in_size, out_size)``."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)               # astype: truncation, like the C cast
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    inside = (x < xmax[:, None]) & (t >= -3.0) & (t < 3.0)

    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v                                                    # libm's sin, the one Pillow calls
    w = np.zeros(t.shape, np.float64)
    w[inside] = [sinc(v) * sinc(v / 3) for v in t[inside].tolist()]
    ww = np.cumsum(w, axis=1)[:, -1:]                                             # sequential sum, index order
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.where(w < 0.0, -0.5 + w * 4194304.0, 0.5 + w * 4194304.0).astype(np.int32)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


# ---------------------------------------------------------------------------------------------------------------------
# What the batch functions below share.  Every call's input travels as ONE packed buffer -- descriptors | tables |
# payload, each part at a multiple of 16 bytes -- written into pinned staging memory and uploaded with one copy.

def _round16(n):
    """THE packing rule: every part of a packed buffer, and every image inside one, begins at a multiple of 16 bytes."""
    return (n + 15) & ~15


def _place(sizes, at=0):
    """Parts of ``sizes`` bytes one after the other from ``at`` on, each begun at a multiple of 16: ``(where each
    begins, where the last one ends, rounded up)``."""
    starts = []
    for n in sizes:
        starts.append(_round16(at))
        at = starts[-1] + int(n)
    return starts, _round16(at)


def _put(host, at, a):
    """``a``'s bytes (descriptor records, an int table, uint8 pixels of any strides) to ``host[at:]``."""
    if a.dtype != np.uint8:
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    host[at:at + a.size].reshape(a.shape)[...] = a


def _put_images(host, at, offsets, arrays):
    for offset, a in zip(offsets, arrays):
        _put(host, at + int(offset), a)


def _sizes_ok(*sides):
    import ssd_hip as _h
    return all(1 <= v <= _h.MAX_IMAGE_SIDE for v in sides)


def _ragged_arrays(images):
    """The uint8 ``[H,W,C]`` NumPy arrays of a batch and their common ``C`` (3 for an empty batch)."""
    import torch
    arrays = []
    for im in images:
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3:
            raise ValueError("images must be uint8 [H,W,3], got %s %s" % (a.dtype, tuple(a.shape)))
        arrays.append(a)
    C = arrays[0].shape[2] if arrays else 3
    if any(a.shape[2] != C for a in arrays):
        raise ValueError("images of one batch must have the same number of channels")
    return arrays, C


def _check_out(out, shape, dtype, dev, name="out", create=False):
    """``out`` if it is a contiguous device tensor of that shape and type (else ``ValueError``); for None a fresh one
    when ``create``."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev) if create else None
    if tuple(out.shape) != shape or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError("%s must be a contiguous %s device tensor %s" % (name, dtype, shape))
    return out


_staging = {}


def _pinned_staging(kind, dev, nbytes):
    """``[buffer, event]``: the device's pinned staging buffer of this ``kind`` ("upload" / "download"), at least
    ``nbytes`` long, grown in powers of two from 1 MiB and kept between calls."""
    import torch
    import ssd_hip as _h
    st = _staging.get((kind, dev.index))
    if st is None or st[0].numel() < nbytes:
        st = _staging[(kind, dev.index)] = [_h.pinned_empty((max(1 << (nbytes - 1).bit_length(), 1 << 20),), torch.uint8), None]
    return st


def _upload_packed(dev, total, fill, device_total=None):
    """``fill(host)`` writes ``total`` bytes into the device's pinned staging buffer (reused once the previous batch's
    copy has left it); ONE asynchronous copy on the current stream makes the device buffer.  ``device_total``: the device
    buffer is that long, and what lies behind the upload is left for kernels to write."""
    import torch
    st = _pinned_staging("upload", dev, total)
    if st[1] is not None:
        st[1].synchronize()                                                       # the previous batch's copy has left the buffer
    fill(st[0].numpy())
    packed = torch.empty(total if device_total is None else device_total, dtype=torch.uint8, device=dev)
    packed[:total].copy_(st[0][:total], non_blocking=True)
    st[1] = torch.cuda.Event()
    st[1].record()
    return packed


def resize_lanczos_batch(images, final_height, final_width, out=None, out_u8=None):
    """``PIL.Image.resize((final_width, final_height), Image.LANCZOS)`` + uint8 -> float32 ``* 1/255`` of a list of uint8
    ``[H,W,3]`` arrays / tensors of ANY sizes, on the GPU, bit for bit (``ssd_resize_lanczos``).  One packed upload
    (descriptors, coefficient tables, pixels: one pinned staging buffer, one copy) and one call per batch.  Returns the
    float32 device tensor ``[B,final_height,final_width,3]`` (``out`` when given: a contiguous float32 device tensor of
    that shape, e.g. a slice of a larger batch); ``out_u8`` (uint8, same shape) also receives the resized bytes."""
    import torch
    import ssd_hip as _h
    fh, fw = int(final_height), int(final_width)
    arrays, C = _ragged_arrays(images)
    B, dev = len(arrays), _h.device()
    out = _check_out(out, (B, fh, fw, C), torch.float32, dev, create=True)
    _check_out(out_u8, (B, fh, fw, C), torch.uint8, dev, "out_u8")
    if _lanczos_nothing_to_pack(B, C, fh, fw, out, out_u8, "resize_lanczos_batch"):
        return out
    layout = _lanczos_layout(arrays, fh, fw)
    packed = _upload_packed(dev, layout["total"], lambda host: _lanczos_fill(host, arrays, layout))
    _lanczos_launch(packed, layout, out, out_u8)
    return out


def _lanczos_nothing_to_pack(B, C, fh, fw, out, out_u8, what):
    """An empty batch, or one the library refuses by its sizes alone: the library answers, nothing is packed."""
    import ssd_hip as _h
    if B > 0 and C == 3 and _sizes_ok(fh, fw):
        return False
    _h.check(_h.lib().ssd_resize_lanczos(None, 0, None, 0, None, None, B, C, fh, fw, _h.ptr(out), _h.ptr(out_u8), None, 0,
                                         _h.stream()), what)
    return True


def _lanczos_layout(arrays, fh, fw, src_offsets=None):
    """Where everything one ``ssd_resize_lanczos`` call reads sits in ONE buffer: descriptors | coefficient tables (int32,
    one per distinct (in, out) pair of the batch) | images, each part at a multiple of 16 bytes.  ``arrays``: the images,
    or only their shapes.  ``src_offsets``: the pixels are on the device already, image b at that offset of a buffer of
    its own (``decode_jpeg_batch``'s), and this buffer ends after the tables."""
    import ssd_hip as _h
    shapes = [tuple(getattr(a, "shape", a)) for a in arrays]
    B = len(shapes)
    desc = np.zeros(B, _h.RESIZE_DESC_DTYPE)
    tables, table_at, n_ints = [], {}, 0

    def table(in_size, out_size):
        nonlocal n_ints
        key = (in_size, out_size)
        if key not in table_at:
            bounds, k = lanczos_coefficients(in_size, out_size)
            table_at[key] = (n_ints, n_ints + bounds.size, k.shape[1])
            tables.extend((bounds, k))
            n_ints += bounds.size + k.size
        return table_at[key]
    pitch = _h.lib().ssd_resize_lanczos_pitch(fw)
    tmp_bytes = 0
    for b, (H, W) in enumerate(s[:2] for s in shapes):
        desc[b]["H"], desc[b]["W"] = H, W
        if not _sizes_ok(H, W):
            continue                                                              # the library reports it (unsupported)
        if W != fw:
            desc[b]["h_bounds"], desc[b]["h_k"], desc[b]["h_ksize"] = table(W, fw)
            desc[b]["tmp_offset"] = tmp_bytes
            tmp_bytes += _round16(H * pitch)
        if H != fh:
            desc[b]["v_bounds"], desc[b]["v_k"], desc[b]["v_ksize"] = table(H, fh)
    (_, tables_at), src_at = _place([desc.nbytes, 4 * n_ints])
    total = src_at
    if src_offsets is None:
        starts, total = _place([int(np.prod(s)) for s in shapes], src_at)
        src_offsets = [at - src_at for at in starts]
    desc["src_offset"] = src_offsets
    assert tmp_bytes == _h.lib().ssd_resize_lanczos_workspace_bytes(desc.ctypes.data, B, fh, fw)
    return {"desc": desc, "tables": tables, "n_ints": n_ints, "tables_at": tables_at, "src_at": src_at, "total": total,
            "tmp_bytes": tmp_bytes, "size": (fh, fw)}


def _lanczos_fill(host, arrays, layout):
    """Write the batch into ``host`` (uint8 NumPy view of at least ``layout["total"]`` bytes); ``arrays``: the images the
    layout was made for, or none when their pixels are on the device already."""
    _put(host, 0, layout["desc"])
    at = layout["tables_at"]
    for tb in layout["tables"]:
        _put(host, at, tb)
        at += tb.nbytes
    _put_images(host, layout["src_at"], layout["desc"]["src_offset"], arrays)


def _lanczos_launch(packed, layout, out, out_u8=None, src=None, what="resize_lanczos_batch"):
    """``ssd_resize_lanczos`` on a device copy ``packed`` of the filled buffer, on the current stream.  ``src``: the
    device buffer that holds the pixels when ``packed`` does not."""
    import ssd_hip as _h
    desc, (fh, fw) = layout["desc"], layout["size"]
    ws = _h.workspace(max(layout["tmp_bytes"], 16))
    base, src_at = packed.data_ptr(), layout["src_at"]
    src_ptr, src_bytes = (base + src_at, layout["total"] - src_at) if src is None else (_h.ptr(src), src.numel())
    _h.check(_h.lib().ssd_resize_lanczos(src_ptr, src_bytes, base + layout["tables_at"], layout["n_ints"],
                                         desc.ctypes.data, base, len(desc), 3, fh, fw, _h.ptr(out), _h.ptr(out_u8),
                                         _h.ptr(ws), ws.numel(), _h.stream()), what)


def _ragged_layout(arrays):
    """Where one ``ssd_preprocess_ragged`` call's input sits in ONE buffer: descriptors | images, each part at a multiple
    of 16 bytes (``src_offset`` counts from the first image)."""
    import ssd_hip as _h
    desc = np.zeros(len(arrays), _h.IMAGE_DESC_DTYPE)
    src_at = _round16(desc.nbytes)
    starts, total = _place([a.size for a in arrays], src_at)
    for b, a in enumerate(arrays):
        desc[b]["H"], desc[b]["W"] = a.shape[:2]
        desc[b]["src_offset"] = starts[b] - src_at
    return {"desc": desc, "src_at": src_at, "total": total}


def _ragged_fill(host, arrays, layout):
    _put(host, 0, layout["desc"])
    _put_images(host, layout["src_at"], layout["desc"]["src_offset"], arrays)


def _ragged_launch(packed, layout, fh, fw, out):
    """``ssd_preprocess_ragged`` on a device copy ``packed`` of the filled buffer, on the current stream."""
    import ssd_hip as _h
    desc, base, src_at = layout["desc"], packed.data_ptr(), layout["src_at"]
    _h.check(_h.lib().ssd_preprocess_ragged(base + src_at, layout["total"] - src_at, desc.ctypes.data, base, len(desc), 3,
                                            fh, fw, _h.ptr(out), _h.stream()), "preprocess_ragged_batch")


def preprocess_ragged_batch(images, final_height, final_width, out=None):
    """``preprocessing``'s image half for a whole batch: a list of uint8 ``[H,W,3]`` arrays / tensors of ANY sizes ->
    float32 ``[B,final_height,final_width,3]`` on the GPU, image b bitwise what ``preprocessing`` makes of it alone.  One
    packed upload (descriptors, pixels: one pinned staging buffer, one asynchronous copy) and ONE launch
    (``ssd_preprocess_ragged``) per batch.  ``out``: a contiguous float32 device tensor of that shape to write into
    (e.g. a slice of a larger batch)."""
    import torch
    import ssd_hip as _h
    fh, fw = int(final_height), int(final_width)
    arrays, C = _ragged_arrays(images)
    B, dev = len(arrays), _h.device()
    out = _check_out(out, (B, fh, fw, C), torch.float32, dev, create=True)
    if B == 0 or C != 3 or not _sizes_ok(fh, fw):                                   # nothing to pack: the library answers
        _h.check(_h.lib().ssd_preprocess_ragged(None, 0, None, None, B, C, fh, fw, _h.ptr(out), _h.stream()),
                 "preprocess_ragged_batch")
        return out
    layout = _ragged_layout(arrays)
    packed = _upload_packed(dev, layout["total"], lambda host: _ragged_fill(host, arrays, layout))
    _ragged_launch(packed, layout, fh, fw, out)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Baseline JPEGs decoded on the GPU behind a host entropy decoder (include/ssd_hip.h, "JPEG decoding"; DESIGN.md
# section 7).  The host parses the markers and decodes the Huffman stream (``ssd_jpeg_parse`` / ``ssd_jpeg_entropy_decode``:
# plain C++, the GIL is released around them); dequantisation, inverse DCT, chroma upsampling and colour conversion run on
# the device (``ssd_jpeg_decode``), Pillow's bytes exactly, and the pixels never exist in host memory.

def jpeg_gpu_enabled():
    """Whether ``voc_batches`` and the custom-image generators decode baseline JPEGs this way: yes unless
    ``SSD_JPEG_GPU=0``.  On by default since the measurement (profiles/HISTORY.md): 2.1x the
    images/s of the Pillow pool at 8 workers, the same bits."""
    import os
    return os.environ.get("SSD_JPEG_GPU", "1") != "0"


class JpegCoefficients(object):
    """One baseline JPEG after the host half: ``info`` (``ssd_hip.JpegInfo``) and ``coef`` (int16, the library's
    coefficient storage), or, while ``coef`` is None, the bytes still to be entropy-decoded (``blob``)."""
    __slots__ = ("info", "coef", "blob")

    def __init__(self, info, coef=None, blob=None):
        self.info, self.coef, self.blob = info, coef, blob


class JpegScan(JpegCoefficients):
    """One baseline JPEG whose Huffman decoding is left to the device (``ssd_jpeg_unpack``): ``info``, the file's bytes
    (``blob``), ``plan`` (``ssd_hip.JpegScanPlan``) and ``segments`` (``JPEG_SEGMENT_DTYPE`` records); ``coef`` stays None."""
    __slots__ = ("plan", "segments")

    def __init__(self, info, blob, plan, segments):
        JpegCoefficients.__init__(self, info, None, blob)
        self.plan, self.segments = plan, segments


def jpeg_entropy_decode_gpu_enabled():
    """Whether the JPEG road also Huffman-decodes on the GPU (``ssd_jpeg_unpack``): only with
    ``SSD_JPEG_ENTROPY_DECODE_GPU=1``.  Opt-in (DESIGN.md section 7 has the measurement); the pixels are the same either
    way.  ``SSD_JPEG_ENTROPY_GPU`` is the encoder's switch."""
    import os
    return os.environ.get("SSD_JPEG_ENTROPY_DECODE_GPU", "0") == "1"


def _pillow_rgb(blob):
    """What the loaders did before: ``Image.open(...).convert("RGB")`` (raises what it raised before)."""
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)


_JPEG_SOI = b"\xff\xd8"


def _jpeg_parse(blob):
    """``ssd_hip.JpegInfo`` of a stream the library decodes, else None (no JPEG at all, unsupported or malformed:
    Pillow's business)."""
    import ctypes
    import ssd_hip as _h
    if blob[:2] != _JPEG_SOI:
        return None
    info = _h.JpegInfo()
    rc = _h.lib().ssd_jpeg_parse(blob, len(blob), ctypes.byref(info))
    return info if rc == 0 else None


def _jpeg_entropy_into(blob, info, address, nbytes):
    import ctypes
    import ssd_hip as _h
    return _h.lib().ssd_jpeg_entropy_decode(blob, len(blob), ctypes.byref(info), address, nbytes) == 0


def _jpeg_plan(blob, info):
    """``JpegScan`` of a parsed stream, or None where ``ssd_jpeg_scan_plan`` refuses it (a bad restart marker, a scan too
    large for the device decoder): the host decoder's business then."""
    import ctypes
    import ssd_hip as _h
    mcus = info.mcus_x * info.mcus_y
    segments = np.zeros(-(-mcus // info.restart_interval) if info.restart_interval else 1, _h.JPEG_SEGMENT_DTYPE)
    plan = _h.JpegScanPlan()
    rc = _h.lib().ssd_jpeg_scan_plan(blob, len(blob), ctypes.byref(info), ctypes.byref(plan), segments.ctypes.data, len(segments))
    return JpegScan(info, blob, plan, segments) if rc == 0 else None


def jpeg_host_plan(blob, fallback=_pillow_rgb):
    """``jpeg_host_decode``'s sibling for ``SSD_JPEG_ENTROPY_DECODE_GPU=1``, for a worker thread: parse the file and plan
    its scan -- a walk over the markers, no code is decoded -- into a ``JpegScan``.  A stream the plan refuses goes the
    way of ``jpeg_host_decode``."""
    blob = bytes(blob)
    info = _jpeg_parse(blob)
    if info is None:
        return fallback(blob)
    return _jpeg_plan(blob, info) or jpeg_host_decode(blob, fallback)


def jpeg_host_decode(blob, fallback=_pillow_rgb):
    """The host half for one file's bytes, for a worker thread: ``JpegCoefficients`` with the coefficients decoded into
    memory of its own, or -- a stream the library calls unsupported or invalid, or no JPEG at all -- ``fallback(blob)``'s
    uint8 ``[H,W,3]`` pixels."""
    blob = bytes(blob)
    info = _jpeg_parse(blob)
    if info is None:
        return fallback(blob)
    coef = np.empty(int(info.coef_bytes) // 2, np.int16)
    if not _jpeg_entropy_into(blob, info, coef.ctypes.data, coef.nbytes):
        return fallback(blob)
    return JpegCoefficients(info, coef)


def _jpeg_items(blobs, fallback):
    """Every entry as ``JpegCoefficients`` (decoded already, or parsed with the entropy decode still to do) or a uint8
    ``[H,W,3]`` array (raw pixels)."""
    items = []
    for x in blobs:
        if isinstance(x, JpegCoefficients):
            items.append(x)
        elif isinstance(x, (bytes, bytearray, memoryview)):
            x = bytes(x)
            info = _jpeg_parse(x)
            items.append(JpegCoefficients(info, None, x) if info is not None else fallback(x))
        else:
            items.append(x)
    for i, x in enumerate(items):
        if not isinstance(x, JpegCoefficients):
            a = np.asarray(x)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("raw images must be uint8 [H,W,3], got %s %s" % (a.dtype, tuple(a.shape)))
            items[i] = a
    return items


def _jpeg_layout(items, subseq_bits=0):
    """Where one ``ssd_jpeg_decode`` call's input sits in ONE buffer: jpeg descriptors | output descriptors | quantisation
    tables | per image its coefficients or raw pixels, each part at a multiple of 16 bytes; and where the output images
    and the component planes go.  With ``JpegScan`` items the buffer goes on: ``ssd_jpeg_unpack``'s input
    (``_jpeg_unpack_layout``) up to ``upload``, and behind it, never uploaded, the coefficients that call writes."""
    import ssd_hip as _h
    B = len(items)
    desc = np.zeros(B, _h.JPEG_DESC_DTYPE)
    out_desc = np.zeros(B, _h.IMAGE_DESC_DTYPE)
    quant_bytes = _h.JpegInfo.quant.size
    (_, out_at, quant_at), payload_at = _place([desc.nbytes, out_desc.nbytes, quant_bytes * B])
    coded = [isinstance(x, JpegCoefficients) for x in items]
    sizes = [int(x.info.coef_bytes) if c else x.size for x, c in zip(items, coded)]
    scans = [b for b, x in enumerate(items) if isinstance(x, JpegScan)]
    unpack = None
    if not scans:
        starts, total = _place(sizes, payload_at)
        upload = total
    else:
        # what the host fills first, then ssd_jpeg_unpack's input, and behind the upload the coefficients it writes
        held = [b for b in range(B) if b not in set(scans)]
        starts = [0] * B
        at, upload = _place([sizes[b] for b in held], payload_at)
        for b, a in zip(held, at):
            starts[b] = a
        unpack = _jpeg_unpack_layout([items[b] for b in scans], subseq_bits, at=upload)
        upload = unpack["total"]
        at, total = _place([sizes[b] for b in scans], upload)
        for b, a in zip(scans, at):
            starts[b] = a
        unpack["desc"]["coef_offset"] = [a - upload for a in at]
        unpack["coef_bytes"] = total - upload
    blocks = n_items = rgb_bytes = plane_bytes = 0
    for b, x in enumerate(items):
        d = desc[b]
        d["coef_offset"], d["block_start"], d["item_start"] = starts[b], blocks, n_items
        if coded[b]:
            i = x.info
            d["kind"], d["H"], d["W"], d["components"] = _h.JPEG_COEFFICIENTS, i.height, i.width, i.components
            d["h_samp"], d["v_samp"] = i.h_samp[0], i.v_samp[0]
            d["quant_offset"], d["plane_offset"] = quant_at + quant_bytes * b, plane_bytes
            blocks += int(i.coef_bytes) // 128
            plane_bytes += _round16(int(i.coef_bytes) // 2)
        else:
            d["kind"], d["H"], d["W"], d["components"], d["h_samp"], d["v_samp"] = _h.JPEG_RAW, x.shape[0], x.shape[1], 3, 1, 1
        out_desc[b]["H"], out_desc[b]["W"], out_desc[b]["src_offset"] = d["H"], d["W"], rgb_bytes
        rgb_bytes += _round16(int(d["H"]) * int(d["W"]) * 3)
        n_items += (int(d["H"]) * int(d["W"]) + 3) // 4
    assert plane_bytes == _h.lib().ssd_jpeg_decode_workspace_bytes(desc.ctypes.data, B)
    return {"desc": desc, "out_desc": out_desc, "out_at": out_at, "total": total, "rgb_bytes": rgb_bytes,
            "plane_bytes": plane_bytes, "upload": upload, "unpack": unpack, "scans": scans}


def _jpeg_fill(host, items, layout, failed):
    """Write the batch into ``host``; a stream still to be entropy-decoded is decoded straight into its place (the
    staging buffer is pinned memory).  Indices of streams the decoder refuses are appended to ``failed``."""
    import ssd_hip as _h
    desc = layout["desc"]
    _put(host, 0, desc)
    _put(host, layout["out_at"], layout["out_desc"])
    quant = _h.JpegInfo.quant
    for b, x in enumerate(items):
        at = int(desc[b]["coef_offset"])
        if not isinstance(x, JpegCoefficients):
            _put(host, at, x)
            continue
        _put(host, int(desc[b]["quant_offset"]), np.frombuffer(x.info, np.uint8)[quant.offset:quant.offset + quant.size])
        if x.coef is not None:
            _put(host, at, x.coef)
        elif isinstance(x, JpegScan):
            continue                                                              # ssd_jpeg_unpack writes them on the device
        elif not _jpeg_entropy_into(x.blob, x.info, host.ctypes.data + at, int(x.info.coef_bytes)):
            failed.append(b)
    if layout["unpack"] is not None:
        _jpeg_unpack_fill(host, [items[b] for b in layout["scans"]], layout["unpack"])


def _jpeg_unpack_layout(scans, subseq_bits=0, at=0):
    """Where one ``ssd_jpeg_unpack`` call's input sits from ``at`` on: descriptors | per image its six Huffman tables |
    its segment table | its stuffed scan bytes, each part at a multiple of 16.  ``coef_offset`` is laid out for a
    coefficient buffer of its own (``coef_bytes``); a caller that places the coefficients elsewhere overwrites it."""
    import ssd_hip as _h
    B = len(scans)
    desc = np.zeros(B, _h.JPEG_UNPACK_DESC_DTYPE)
    sizes = [desc.nbytes] + [_h.JPEG_HUFF_BYTES] * B + [x.segments.nbytes for x in scans] + [
        int(x.plan.data_end - x.plan.data_begin) for x in scans]
    starts, total = _place(sizes, at)
    coef_at, coef_bytes = _place([int(x.info.coef_bytes) for x in scans])
    blocks = segs = slots = 0
    for b, x in enumerate(scans):
        d, i = desc[b], x.info
        d["huff_offset"], d["seg_offset"], d["scan_offset"] = starts[1 + b], starts[1 + B + b], starts[1 + 2 * B + b]
        d["scan_bytes"], d["coef_offset"] = sizes[1 + 2 * B + b], coef_at[b]
        d["H"], d["W"], d["components"], d["h_samp"], d["v_samp"] = i.height, i.width, i.components, i.h_samp[0], i.v_samp[0]
        d["restart_interval"], d["segments"] = i.restart_interval, len(x.segments)
        d["block_start"], d["seg_start"], d["sub_start"] = blocks, segs, slots
        blocks += int(i.coef_bytes) // 128
        segs += len(x.segments) + 1
        slots += _h.lib().ssd_jpeg_unpack_slots(int(d["scan_bytes"]), len(x.segments), subseq_bits)
    return {"desc": desc, "desc_at": starts[0], "total": total, "coef_bytes": coef_bytes, "subseq_bits": int(subseq_bits)}


def _jpeg_unpack_fill(host, scans, layout):
    import ssd_hip as _h
    desc = layout["desc"]
    _put(host, layout["desc_at"], desc)
    huff = _h.JpegScanPlan.huff
    for d, x in zip(desc, scans):
        _put(host, int(d["huff_offset"]), np.frombuffer(x.plan, np.uint8)[huff.offset:huff.offset + huff.size])
        _put(host, int(d["seg_offset"]), x.segments)
        _put(host, int(d["scan_offset"]), np.frombuffer(x.blob, np.uint8)[int(x.plan.data_begin):int(x.plan.data_end)])


def _jpeg_unpack_launch(packed_ptr, layout, coef_ptr, ws_extra=0, what="jpeg_unpack_batch"):
    """``ssd_jpeg_unpack`` on a device copy of the filled buffer (``packed_ptr``: its first byte), on the current stream;
    returns the int32 device tensor ``[2, B]``: ``status`` and the debug counter ``sweeps``.  The workspace is at least
    ``ws_extra`` bytes, for the call that follows on the same stream."""
    import torch
    import ssd_hip as _h
    desc, bits = layout["desc"], layout["subseq_bits"]
    B = len(desc)
    need = int(_h.lib().ssd_jpeg_unpack_workspace_bytes(desc.ctypes.data, B, bits))
    ws = _h.workspace(max(need, ws_extra, 16))
    meta = torch.empty((2, B), dtype=torch.int32, device=_h.device())
    _h.check(_h.lib().ssd_jpeg_unpack(packed_ptr, layout["total"], desc.ctypes.data, packed_ptr + layout["desc_at"], B, bits, coef_ptr,
                                      layout["coef_bytes"], meta.data_ptr(), _h.ptr(ws), ws.numel(), _h.stream()), what)
    meta[1].copy_(ws[:4 * B].view(torch.int32))                                    # the sweeps: the workspace's first B int32
    return meta


def jpeg_unpack_batch(blobs, subseq_bits=0):
    """The bare ``ssd_jpeg_unpack`` call: baseline JPEG files' ``bytes`` (or ``JpegScan``) -> ``(coef, desc, status,
    sweeps)``: a uint8 device buffer that holds image b's coefficient storage -- ``ssd_jpeg_entropy_decode``'s, bit for
    bit -- at ``desc[b]["coef_offset"]``, the ``JPEG_UNPACK_DESC_DTYPE`` descriptors, and two int32 device tensors
    ``[B]``: ``status`` (nonzero: the host decoder's business) and the sweeps the synchronise phase took.  ONE upload: the
    files' scan bytes and their plans.  ``ValueError`` for a stream ``ssd_jpeg_parse`` or ``ssd_jpeg_scan_plan`` refuses."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    scans = []
    for x in blobs:
        if not isinstance(x, JpegScan):
            x = bytes(x)
            info = _jpeg_parse(x)
            x = _jpeg_plan(x, info) if info is not None else None
            if x is None:
                raise ValueError("jpeg_unpack_batch: %s" % _h.lib().ssd_last_error().decode())
        scans.append(x)
    if not scans:
        _h.check(_h.lib().ssd_jpeg_unpack(None, 0, None, None, 0, int(subseq_bits), None, 0, None, None, 0, _h.stream()), "jpeg_unpack_batch")
        empty = torch.empty(0, dtype=torch.int32, device=dev)
        return torch.empty(0, dtype=torch.uint8, device=dev), np.zeros(0, _h.JPEG_UNPACK_DESC_DTYPE), empty, empty
    layout = _jpeg_unpack_layout(scans, subseq_bits)
    packed = _upload_packed(dev, layout["total"], lambda host: _jpeg_unpack_fill(host, scans, layout))
    coef = torch.empty(max(layout["coef_bytes"], 16), dtype=torch.uint8, device=dev)
    meta = _jpeg_unpack_launch(packed.data_ptr(), layout, _h.ptr(coef))
    return coef, layout["desc"], meta[0], meta[1]


class JpegBatch(object):
    """What ``decode_jpeg_batch`` returns: ``images`` (uint8 device views ``[H_b,W_b,3]`` into ``rgb``), ``rgb`` (the
    packed device buffer), ``desc`` (its ``ssd_image_desc`` layout, host) and ``desc_ptr`` (the same descriptors in
    device memory, inside ``packed``, which is kept alive here)."""
    __slots__ = ("images", "rgb", "desc", "desc_ptr", "packed", "kinds")

    def __init__(self, images, rgb, desc, desc_ptr, packed, kinds):
        self.images, self.rgb, self.desc, self.desc_ptr, self.packed, self.kinds = images, rgb, desc, desc_ptr, packed, kinds


def decode_jpeg_batch(blobs, out_u8=False, fallback=_pillow_rgb):
    """A list of JPEG files' ``bytes`` -> their pixels on the GPU, bitwise ``PIL.Image.open(...).convert("RGB")``'s, as a
    ``JpegBatch``.  Per batch: parse, lay out, entropy-decode straight into the pinned staging buffer, ONE upload, ONE
    ``ssd_jpeg_decode`` call (two launches).  ``SSD_JPEG_ENTROPY_DECODE_GPU=1`` (opt-in): the host only plans each scan
    (``ssd_jpeg_scan_plan``), the upload carries the files' scan bytes instead of their coefficients, and
    ``ssd_jpeg_unpack`` Huffman-decodes them into the buffer ``ssd_jpeg_decode`` then reads; an image that call flags is
    redone by the host decoder, so the pixels are the same for every input.  A stream the library calls unsupported (progressive, CMYK, ...) or
    malformed is decoded by ``fallback`` -- Pillow, exactly as before, raising what it raised before -- and travels as raw
    pixels in the same upload; entries may also be ``JpegCoefficients`` from ``jpeg_host_decode`` (the data pool's
    threads) or uint8 ``[H,W,3]`` arrays.  ``out_u8``: a contiguous 1-D uint8 device tensor, 16-byte aligned and large
    enough (``sum(round16(H*W*3))``), to decode into instead of a fresh buffer; nothing outside the images is written."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    items = _jpeg_items(blobs, fallback)
    B = len(items)
    if B == 0:
        _h.check(_h.lib().ssd_jpeg_decode(None, 0, None, None, 0, None, 0, None, None, None, 0, _h.stream()), "decode_jpeg_batch")
        return JpegBatch([], torch.empty(0, dtype=torch.uint8, device=dev), np.zeros(0, _h.IMAGE_DESC_DTYPE), 0, None, [])
    if jpeg_entropy_decode_gpu_enabled():                                         # the files' scans go up, not their coefficients
        for b, x in enumerate(items):
            if isinstance(x, JpegCoefficients) and x.coef is None and not isinstance(x, JpegScan):
                items[b] = _jpeg_plan(x.blob, x.info) or x
    def to_host_decoder():
        # rare: what the device decoder flags or cannot take goes the host decoder's way (and Pillow's, if that refuses
        # too) with the whole batch, so the result is the default road's for every input whatsoever
        for b, x in enumerate(items):
            if isinstance(x, JpegScan):
                items[b] = JpegCoefficients(x.info, None, x.blob)
    while True:
        while True:
            layout = _jpeg_layout(items)
            failed = []
            packed = _upload_packed(dev, layout["upload"], lambda host: _jpeg_fill(host, items, layout, failed), layout["total"])
            if not failed:
                break
            for b in failed:                                                      # malformed past the header: Pillow's business
                items[b] = np.asarray(fallback(items[b].blob))
        base, meta = packed.data_ptr(), None
        if layout["unpack"] is not None:
            try:
                meta = _jpeg_unpack_launch(base, layout["unpack"], base + layout["upload"], layout["plane_bytes"], "decode_jpeg_batch")
            except _h.SsdHipUnsupported:
                to_host_decoder()
                continue
        if out_u8 is None or out_u8 is False:
            rgb = torch.empty(max(layout["rgb_bytes"], 16), dtype=torch.uint8, device=dev)
        else:
            rgb = out_u8
            if (not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.device != dev or rgb.dim() != 1
                    or not rgb.is_contiguous() or rgb.numel() < layout["rgb_bytes"] or rgb.data_ptr() % 16):
                raise ValueError("out_u8 must be a contiguous 1-D uint8 device tensor of at least %d bytes, 16-byte aligned"
                                 % layout["rgb_bytes"])
        ws = _h.workspace(max(layout["plane_bytes"], 16))
        desc, out_desc = layout["desc"], layout["out_desc"]
        _h.check(_h.lib().ssd_jpeg_decode(base, layout["total"], desc.ctypes.data, base, B, _h.ptr(rgb), rgb.numel(),
                                          out_desc.ctypes.data, base + layout["out_at"], _h.ptr(ws), ws.numel(), _h.stream()),
                 "decode_jpeg_batch")
        if meta is None or not meta[0].cpu().numpy().any():                       # the status: ONE small read
            break
        to_host_decoder()
    images = [rgb[int(o["src_offset"]):int(o["src_offset"]) + int(o["H"]) * int(o["W"]) * 3].view(int(o["H"]), int(o["W"]), 3)
              for o in out_desc]
    return JpegBatch(images, rgb, out_desc, base + layout["out_at"], packed, [int(k) for k in desc["kind"]])


def preprocess_jpeg_batch(blobs, final_height, final_width, out=None, fallback=_pillow_rgb):
    """``preprocess_ragged_batch`` of the decoded files without the pixels ever being on the host: ``decode_jpeg_batch``,
    then ``ssd_preprocess_ragged`` on the device-resident images.  Bitwise ``preprocess_ragged_batch([Pillow's decode of
    each], ...)``."""
    import torch
    import ssd_hip as _h
    fh, fw = int(final_height), int(final_width)
    B = len(blobs)
    out = _check_out(out, (B, fh, fw, 3), torch.float32, _h.device(), create=True)
    jb = decode_jpeg_batch(blobs, fallback=fallback)
    _h.check(_h.lib().ssd_preprocess_ragged(_h.ptr(jb.rgb), jb.rgb.numel(), jb.desc.ctypes.data, jb.desc_ptr, B, 3, fh, fw,
                                            _h.ptr(out), _h.stream()), "preprocess_jpeg_batch")
    return out


def resize_lanczos_jpeg_batch(blobs, final_height, final_width, out=None, out_u8=None, fallback=_pillow_rgb):
    """``resize_lanczos_batch`` of the decoded files: ``decode_jpeg_batch``, then ``ssd_resize_lanczos`` on the
    device-resident images (a second, small upload carries the coefficient tables).  Bitwise ``resize_lanczos_batch([Pillow's
    decode of each], ...)``."""
    import torch
    import ssd_hip as _h
    fh, fw = int(final_height), int(final_width)
    dev = _h.device()
    B = len(blobs)
    out = _check_out(out, (B, fh, fw, 3), torch.float32, dev, create=True)
    _check_out(out_u8, (B, fh, fw, 3), torch.uint8, dev, "out_u8")
    if _lanczos_nothing_to_pack(B, 3, fh, fw, out, out_u8, "resize_lanczos_jpeg_batch"):
        return out
    jb = decode_jpeg_batch(blobs, fallback=fallback)
    layout = _lanczos_layout([(int(o["H"]), int(o["W"])) for o in jb.desc], fh, fw, src_offsets=jb.desc["src_offset"])
    packed = _upload_packed(dev, layout["total"], lambda host: _lanczos_fill(host, [], layout))
    _lanczos_launch(packed, layout, out, out_u8, src=jb.rgb, what="resize_lanczos_jpeg_batch")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Baseline JPEGs encoded behind a GPU forward DCT (include/ssd_hip.h, "JPEG encoding"): the mirror
# image of the decoder.  Colour conversion, chroma downsampling, forward DCT and quantisation run on the device
# (``ssd_jpeg_forward``); the host writes the header and the Huffman stream (``ssd_jpeg_entropy_encode``: plain C++, the
# GIL is released around it) on the data pool's threads.  The bytes are ``PIL.Image.fromarray(a).save(f, "JPEG",
# quality=q, subsampling=s)``'s exactly.

JPEG_SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}                 # luma (h_samp, v_samp)
# On by default since the measurement (tests/bench_jpeg_encode.py; DESIGN.md section 7, profiles/HISTORY.md): 3.3x the
# images/s of the Pillow JPEG pool at 8 workers, spreads not overlapping, the same bytes.
JPEG_ENCODE_GPU_DEFAULT = "1"
_encode_pools = {}


def jpeg_encode_gpu_enabled():
    """Whether ``encode_jpeg_batch`` runs the forward DCT on the GPU: yes unless ``SSD_JPEG_ENCODE_GPU=0``, which routes
    to Pillow on downloaded pixels (the fallback and the A/B leg; the same bytes)."""
    import os
    return os.environ.get("SSD_JPEG_ENCODE_GPU", JPEG_ENCODE_GPU_DEFAULT) != "0"


def _encode_pool(workers):
    """The threads that write the streams: ``data_workers(workers)`` of them, kept between calls."""
    from concurrent.futures import ThreadPoolExecutor
    n = data_workers(workers)
    if n not in _encode_pools:
        _encode_pools[n] = ThreadPoolExecutor(max_workers=n, thread_name_prefix="ssd-jpeg")
    return _encode_pools[n]


def _per_image(value, B, name):
    if isinstance(value, (list, tuple, np.ndarray)):
        if len(value) != B:
            raise ValueError("%s: %d entries for %d images" % (name, len(value), B))
        return list(value)
    return [value] * B


def _jpeg_encode_layout(shapes, samplings):
    """Where one ``ssd_jpeg_forward`` call's input and output sit: descriptors | quantisation tables in ONE upload, the
    coefficient storage of the images one after the other (each rounded up to 16 bytes), the component planes likewise."""
    import ssd_hip as _h
    B = len(shapes)
    desc = np.zeros(B, _h.JPEG_ENC_DESC_DTYPE)
    (_, tables_at), total = _place([desc.nbytes, 256 * B])
    src = coef = planes = blocks = items = 0
    for b, ((H, W), (hs, vs)) in enumerate(zip(shapes, samplings)):
        d = desc[b]
        d["H"], d["W"], d["h_samp"], d["v_samp"] = H, W, hs, vs
        d["src_offset"], d["coef_offset"], d["quant_offset"], d["plane_offset"] = src, coef, tables_at + 256 * b, planes
        d["block_start"], d["item_start"] = blocks, items
        n1 = -(-W // (8 * hs)) * -(-H // (8 * vs))
        nb = n1 * (hs * vs + 2)
        src += H * W * 3
        coef += _round16(nb * 128)
        planes += _round16(nb * 64)
        blocks += nb
        items += n1 * 16
    return {"desc": desc, "tables_at": tables_at, "total": total, "coef_bytes": coef, "plane_bytes": planes}


def _jpeg_encode_fill(host, layout, tables):
    """Write the descriptors and the quantisation tables (uint16 ``[B,2,64]``) into ``host``."""
    _put(host, 0, layout["desc"])
    _put(host, layout["tables_at"], np.asarray(tables, np.uint16))


def jpeg_forward_batch(rgb, shapes, samplings, tables):
    """``ssd_jpeg_forward`` on packed device pixels: ``rgb`` a contiguous uint8 device tensor holding the images one after
    the other, ``shapes`` [(H, W)], ``samplings`` [(h_samp, v_samp)], ``tables`` uint16 [B,2,64].  Returns ``(coef, desc)``:
    the uint8 device buffer of the coefficient storages and the descriptors (``coef_offset`` says where each begins)."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    B = len(shapes)
    for H, W in shapes:
        if not _sizes_ok(H, W):
            raise _h.SsdHipUnsupported("encode_jpeg_batch: an image of %d x %d, outside 1..%d" % (H, W, _h.MAX_IMAGE_SIDE))
    layout = _jpeg_encode_layout(shapes, samplings)
    desc = layout["desc"]
    tables = np.asarray(tables, np.uint16).reshape(B, 128)
    packed = _upload_packed(dev, layout["total"], lambda host: _jpeg_encode_fill(host, layout, tables))
    assert layout["plane_bytes"] == _h.lib().ssd_jpeg_forward_workspace_bytes(desc.ctypes.data, B)
    coef = torch.empty(max(layout["coef_bytes"], 16), dtype=torch.uint8, device=dev)
    ws = _h.workspace(max(layout["plane_bytes"], 16))
    base = packed.data_ptr()
    _h.check(_h.lib().ssd_jpeg_forward(_h.ptr(rgb), rgb.numel(), base, layout["total"], desc.ctypes.data, base, B, _h.ptr(coef),
                                       coef.numel(), _h.ptr(ws), ws.numel(), _h.stream()), "encode_jpeg_batch")
    return coef, desc


def jpeg_host_encode(coef, H, W, sampling, tables):
    """The host half for one image, for a worker thread: int16 coefficient storage (a NumPy view, e.g. of the pinned
    download) -> the JPEG stream's ``bytes``."""
    import ctypes
    import ssd_hip as _h
    lib = _h.lib()
    info = _h.JpegInfo()
    tables = np.ascontiguousarray(tables, np.uint16)
    _h.check(lib.ssd_jpeg_encode_info(int(W), int(H), int(sampling[0]), int(sampling[1]), tables.ctypes.data, ctypes.byref(info)),
             "ssd_jpeg_encode_info")
    if coef.nbytes < info.coef_bytes:
        raise ValueError("jpeg_host_encode: %d bytes of coefficients, the image needs %d" % (coef.nbytes, info.coef_bytes))
    out = np.empty(int(lib.ssd_jpeg_encode_bound(ctypes.byref(info))), np.uint8)
    written = ctypes.c_size_t(0)
    _h.check(lib.ssd_jpeg_entropy_encode(coef.ctypes.data, ctypes.byref(info), out.ctypes.data, out.nbytes, ctypes.byref(written)),
             "ssd_jpeg_entropy_encode")
    return out[:written.value].tobytes()


def jpeg_entropy_gpu_enabled():
    """Whether ``encode_jpeg_batch`` also entropy-codes on the GPU (``ssd_jpeg_pack``): only with ``SSD_JPEG_ENTROPY_GPU=1``.
    Opt-in: the default stays the host pool (DESIGN.md section 7 has the measurement and the recommendation)."""
    import os
    return os.environ.get("SSD_JPEG_ENTROPY_GPU", "0") == "1"


def _jpeg_pack_layout(desc, shapes, samplings, tables):
    """Where one ``ssd_jpeg_pack`` call's input sits: its descriptors | every image's header in ONE upload (each part at a
    multiple of 16), taken from ``jpeg_forward_batch``'s descriptors; and ``out_bytes``, the sum of the images'
    ``ssd_jpeg_encode_bound``, each rounded up to 16."""
    import ctypes
    import ssd_hip as _h
    lib = _h.lib()
    B = len(shapes)
    pd = np.zeros(B, _h.JPEG_PACK_DESC_DTYPE)
    starts, total = _place([pd.nbytes] + [_h.JPEG_HEADER_BYTES] * B)
    infos, bound = [], 0
    for b, ((H, W), (hs, vs)) in enumerate(zip(shapes, samplings)):
        d = pd[b]
        d["H"], d["W"], d["h_samp"], d["v_samp"] = H, W, hs, vs
        d["coef_offset"], d["block_start"], d["header_offset"] = desc[b]["coef_offset"], desc[b]["block_start"], starts[1 + b]
        info = _h.JpegInfo()
        t = np.ascontiguousarray(tables[b], np.uint16)
        _h.check(lib.ssd_jpeg_encode_info(int(W), int(H), int(hs), int(vs), t.ctypes.data, ctypes.byref(info)), "ssd_jpeg_encode_info")
        infos.append(info)
        bound += _round16(int(lib.ssd_jpeg_encode_bound(ctypes.byref(info))))
    return {"desc": pd, "headers_at": starts[1:], "total": total, "out_bytes": bound, "infos": infos}


def _jpeg_pack_fill(host, layout):
    """Write the descriptors and every image's header (``ssd_jpeg_encode_header``) into ``host``."""
    import ctypes
    import ssd_hip as _h
    _put(host, 0, layout["desc"])
    header = np.empty(_h.JPEG_HEADER_BYTES, np.uint8)
    written = ctypes.c_size_t(0)
    for at, info in zip(layout["headers_at"], layout["infos"]):
        _h.check(_h.lib().ssd_jpeg_encode_header(ctypes.byref(info), header.ctypes.data, header.nbytes, ctypes.byref(written)),
                 "ssd_jpeg_encode_header")
        assert written.value == header.nbytes
        _put(host, at, header)


def _jpeg_pack(coef, desc, shapes, samplings, tables):
    """``jpeg_pack_batch`` with ``offsets`` and ``status`` still in the ONE int32 tensor that holds both (one download)."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    lib = _h.lib()
    B = len(shapes)
    meta = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
    if B == 0:
        _h.check(lib.ssd_jpeg_pack(None, 0, None, 0, None, None, 0, None, 0, None, None, None, 0, _h.stream()), "jpeg_pack_batch")
        return torch.empty(0, dtype=torch.uint8, device=dev), meta.zero_()
    tables = np.asarray(tables, np.uint16).reshape(B, 2, 64)
    layout = _jpeg_pack_layout(desc, shapes, samplings, tables)
    pd = layout["desc"]
    packed = _upload_packed(dev, layout["total"], lambda host: _jpeg_pack_fill(host, layout))
    out = torch.empty(layout["out_bytes"], dtype=torch.uint8, device=dev)
    ws = _h.workspace(max(int(lib.ssd_jpeg_pack_workspace_bytes(pd.ctypes.data, B)), 16))
    base = packed.data_ptr()
    _h.check(lib.ssd_jpeg_pack(_h.ptr(coef), coef.numel(), base, layout["total"], pd.ctypes.data, base, B, _h.ptr(out), out.numel(),
                               meta.data_ptr(), meta.data_ptr() + 4 * (B + 1), _h.ptr(ws), ws.numel(), _h.stream()), "jpeg_pack_batch")
    return out, meta


def jpeg_pack_batch(coef, desc, shapes, samplings, tables):
    """``ssd_jpeg_pack`` on what ``jpeg_forward_batch`` returns (``coef``, ``desc``) for the same ``shapes``, ``samplings`` and
    ``tables``: ONE packed upload (descriptors | headers), one call, no synchronisation.  Returns device tensors ``(out,
    offsets, status)``: stream b is ``out[offsets[b]:offsets[b + 1]]`` (int32 ``[B + 1]``), ``status`` int32 ``[B]`` is
    nonzero for an image whose coefficients the baseline cannot code (its region's content is then unspecified)."""
    out, meta = _jpeg_pack(coef, desc, shapes, samplings, tables)
    B = len(shapes)
    return out, meta[:B + 1], meta[B + 1:]


def _jpeg_pack_streams(coef, desc, shapes, samplings, tables):
    """The streams of a batch as ``bytes`` through the device coder: two downloads (offsets + status; the streams
    themselves, into pinned memory), sliced on the calling thread.  An image the baseline cannot code raises what the
    host coder raises for its coefficients."""
    import torch
    import ssd_hip as _h
    B = len(shapes)
    out, meta = _jpeg_pack(coef, desc, shapes, samplings, tables)
    meta = meta.cpu().numpy()
    offsets, status = meta[:B + 1], meta[B + 1:]
    bad = np.flatnonzero(status)
    if bad.size:
        b = int(bad[0])
        at = int(desc[b]["coef_offset"])
        end = int(desc[b + 1]["coef_offset"]) if b + 1 < B else coef.numel()
        jpeg_host_encode(coef[at:end].cpu().numpy().view(np.int16), shapes[b][0], shapes[b][1], samplings[b], tables[b])
        raise _h.SsdHipError("jpeg_pack_batch: image %d has status %d, yet the host coder takes its coefficients" % (b, status[b]))
    n = int(offsets[B])
    st = _pinned_staging("download", out.device, n)[0]
    st[:n].copy_(out[:n], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    host = st.numpy()
    return [host[offsets[b]:offsets[b + 1]].tobytes() for b in range(B)]


def _pillow_jpeg(args):
    import io
    from PIL import Image
    pixels, quality, subsampling = args
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def encode_jpeg_batch(images, quality=75, subsampling="4:2:0", workers=None):
    """Device uint8 images -> their JPEG files' ``bytes``, bitwise ``PIL.Image.fromarray(a).save(f, "JPEG", quality=quality,
    subsampling=subsampling)``'s.  ``images``: a device uint8 ``[B,H,W,3]`` tensor (what ``drawing_utils`` draws) or a list
    of device ``[H,W,3]`` tensors of any sizes; ``quality`` and ``subsampling`` ("4:4:4", "4:2:2", "4:2:0") may be one
    value or one per image.  Per batch: ONE descriptor upload, ONE ``ssd_jpeg_forward`` call (two launches), ONE download
    of the int16 coefficients into pinned memory; then ``ssd_jpeg_entropy_encode`` per image on ``data_workers(workers)``
    threads.  ``SSD_JPEG_ENCODE_GPU=0``: the pixels are downloaded and Pillow encodes them on the same threads.
    ``SSD_JPEG_ENTROPY_GPU=1`` (opt-in): the Huffman coding, the stuffing and the header run on the GPU as well
    (``jpeg_pack_batch``); the downloads shrink to offsets + status and the finished streams, which the calling thread
    slices into ``bytes`` -- no thread pool is used.  A batch outside ``ssd_jpeg_pack``'s limits takes the host pool."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError("images must be uint8 [B,H,W,3] or a list of [H,W,3], got %s" % (tuple(images.shape),))
        seq = list(images)
    else:
        seq = list(images)
    for t in seq:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.device != dev:
            raise ValueError("images must be device uint8 [H,W,3] tensors")
    B = len(seq)
    qualities = [int(q) for q in _per_image(quality, B, "quality")]
    subs = _per_image(subsampling, B, "subsampling")
    for s in subs:
        if s not in JPEG_SAMPLING:
            raise ValueError("subsampling must be one of %s, got %r" % (sorted(JPEG_SAMPLING), s))
    if B == 0:
        _h.check(_h.lib().ssd_jpeg_forward(None, 0, None, 0, None, None, 0, None, 0, None, 0, _h.stream()), "encode_jpeg_batch")
        return []
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in seq]
    if isinstance(images, torch.Tensor) and images.is_contiguous():
        rgb = images.reshape(-1)
    else:
        rgb = torch.cat([t.reshape(-1) for t in seq])
    if not jpeg_encode_gpu_enabled():
        host = rgb.cpu().numpy()
        ends = np.cumsum([h * w * 3 for h, w in shapes])
        jobs = [(host[e - h * w * 3:e].reshape(h, w, 3), q, s) for e, (h, w), q, s in zip(ends, shapes, qualities, subs)]
        return list(_encode_pool(workers).map(_pillow_jpeg, jobs))
    samplings = [JPEG_SAMPLING[s] for s in subs]
    known = {}
    tables = np.empty((B, 2, 64), np.uint16)
    for b, q in enumerate(qualities):
        if q not in known:
            known[q] = np.empty((2, 64), np.uint16)
            _h.check(_h.lib().ssd_jpeg_quality_tables(q, known[q].ctypes.data), "ssd_jpeg_quality_tables")
        tables[b] = known[q]
    coef, desc = jpeg_forward_batch(rgb, shapes, samplings, tables)
    if jpeg_entropy_gpu_enabled():
        try:
            return _jpeg_pack_streams(coef, desc, shapes, samplings, tables)
        except _h.SsdHipUnsupported:
            pass                                                                  # outside the device coder's limits: the host pool
    st = _pinned_staging("download", dev, coef.numel())[0]
    st[:coef.numel()].copy_(coef, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    host = st.numpy()
    ends = [int(d["coef_offset"]) for d in desc[1:]] + [coef.numel()]
    jobs = [(host[int(d["coef_offset"]):e].view(np.int16), h, w, hv, t)
            for d, e, (h, w), hv, t in zip(desc, ends, shapes, samplings, tables)]
    return list(_encode_pool(workers).map(lambda a: jpeg_host_encode(*a), jobs))


# --- PNG output: the files themselves are made on the GPU (ssd_png_encode; include/ssd_hip.h "PNG ENCODER") -----------------------------
# PNG is lossless, so the bytes are not Pillow's (zlib's matcher is a serial heuristic): every decoder returns the input
# pixels, and ``ssd_png_encode_host`` writes the same bytes on the host.

def png_gpu_enabled():
    """Whether ``drawing_utils`` writes ``out_format="png"`` through ``encode_png_batch``: only with ``SSD_PNG_GPU=1``.
    Opt-in: unset or anything else is Pillow's ``save`` on downloaded pixels (DESIGN.md section 7 has the measurement)."""
    import os
    return os.environ.get("SSD_PNG_GPU", "0") == "1"


def _png_filters(filter, B):
    import ssd_hip as _h
    out = []
    for f in _per_image(filter, B, "filter"):
        if f not in _h.PNG_FILTERS:
            raise ValueError("filter must be one of %s, got %r" % (sorted(_h.PNG_FILTERS), f))
        out.append(_h.PNG_FILTERS[f])
    return out


def _png_layout(shapes, filters):
    """Where one ``ssd_png_encode`` call's input and output sit: the descriptors are the ONE upload (pixels stay where they
    are: ``src_offset`` counts the images one after the other), ``seg_start`` / ``row_start`` the running sums of the IDAT
    chunks (one per 16384 bytes of ``H * (1 + 3W)``) and of the rows; ``out_bytes`` the sum of the images'
    ``ssd_png_encode_bound``."""
    import ssd_hip as _h
    B = len(shapes)
    desc = np.zeros(B, _h.PNG_DESC_DTYPE)
    src = segs = rows = bound = 0
    for b, ((H, W), f) in enumerate(zip(shapes, filters)):
        d = desc[b]
        d["src_offset"], d["H"], d["W"], d["filter"], d["seg_start"], d["row_start"] = src, H, W, f, segs, rows
        n = -(-(H * (1 + 3 * W)) // _h.PNG_SEGMENT_BYTES)
        src += H * W * 3
        segs += n
        rows += H
        bound += 45 + 17 * n + H * (1 + 3 * W) + 6
    return {"desc": desc, "total": _round16(desc.nbytes), "out_bytes": bound, "segments": segs}


def png_pack_batch(rgb, shapes, filter="adaptive"):
    """``ssd_png_encode`` on packed device pixels: ``rgb`` a contiguous uint8 device tensor holding the images one after
    the other, ``shapes`` [(H, W)], ``filter`` one of "none" | "sub" | "up" | "average" | "paeth" | "adaptive" or one per
    image (integers 0..5 are passed through to the library).  ONE descriptor upload, one call (four launches), no
    synchronisation.  Returns device tensors ``(out, offsets)``: file b is ``out[offsets[b]:offsets[b + 1]]`` (int32
    ``[B + 1]``).  ``SsdHipUnsupported`` for a batch outside the kernel's limits."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    lib = _h.lib()
    B = len(shapes)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    if B == 0:
        _h.check(lib.ssd_png_encode(None, 0, None, None, 0, None, 0, None, None, 0, _h.stream()), "png_pack_batch")
        return torch.empty(0, dtype=torch.uint8, device=dev), offsets.zero_()
    filters = [f if isinstance(f, (int, np.integer)) else _png_filters(f, 1)[0] for f in _per_image(filter, B, "filter")]
    layout = _png_layout(shapes, filters)
    desc = layout["desc"]
    packed = _upload_packed(dev, layout["total"], lambda host: _put(host, 0, desc))
    if layout["out_bytes"] > 2 ** 31 - 1:
        raise _h.SsdHipUnsupported("png_pack_batch: the files may need more than 2^31 - 1 bytes")
    out = torch.empty(layout["out_bytes"], dtype=torch.uint8, device=dev)
    ws = _h.workspace(max(int(lib.ssd_png_encode_workspace_bytes(desc.ctypes.data, B)), 16))
    _h.check(lib.ssd_png_encode(_h.ptr(rgb), rgb.numel(), desc.ctypes.data, packed.data_ptr(), B, _h.ptr(out), out.numel(),
                                _h.ptr(offsets), _h.ptr(ws), ws.numel(), _h.stream()), "png_pack_batch")
    return out, offsets


def _pillow_png(pixels):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "PNG")
    return buf.getvalue()


def encode_png_batch(images, filter="adaptive"):
    """Device uint8 images -> their PNG files' ``bytes``, made on the GPU.  ``images``: a device uint8 ``[B,H,W,3]`` tensor
    (what ``drawing_utils`` draws) or a list of device ``[H,W,3]`` tensors of any sizes; ``filter`` ("none", "sub", "up",
    "average", "paeth", "adaptive") may be one value or one per image.  Per batch: ONE descriptor upload, ONE
    ``ssd_png_encode`` call, the download of the offsets, then ONE download of the files into pinned memory, which the
    calling thread slices into ``bytes``.  A batch outside the kernel's limits (``SsdHipUnsupported``) is downloaded as
    pixels and encoded by Pillow."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError("images must be uint8 [B,H,W,3] or a list of [H,W,3], got %s" % (tuple(images.shape),))
        seq = list(images)
    else:
        seq = list(images)
    for t in seq:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.device != dev:
            raise ValueError("images must be device uint8 [H,W,3] tensors")
    B = len(seq)
    filters = _png_filters(filter, B)
    if B == 0:
        png_pack_batch(None, [])
        return []
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in seq]
    if isinstance(images, torch.Tensor) and images.is_contiguous():
        rgb = images.reshape(-1)
    else:
        rgb = torch.cat([t.reshape(-1) for t in seq])
    try:
        out, offsets = png_pack_batch(rgb, shapes, filters)
    except _h.SsdHipUnsupported:
        host = rgb.cpu().numpy()
        ends = np.cumsum([h * w * 3 for h, w in shapes])
        return [_pillow_png(host[e - h * w * 3:e].reshape(h, w, 3)) for e, (h, w) in zip(ends, shapes)]
    offsets = offsets.cpu().numpy()
    n = int(offsets[B])
    st = _pinned_staging("download", dev, n)[0]
    st[:n].copy_(out[:n], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    host = st.numpy()
    return [host[offsets[b]:offsets[b + 1]].tobytes() for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------------
# PNG files decoded on the GPU behind a host inflate (include/ssd_hip.h, "PNG DECODER").  The host
# walks the chunks and verifies the CRCs (``ssd_png_parse``: plain C++, the GIL is released around it) and inflates the
# zlib stream (Python's ``zlib``, which releases the GIL too); un-filtering the scanlines and converting the samples to
# packed RGB run on the device (``ssd_png_decode``), Pillow's pixels exactly, and the pixels never exist in host memory.

def png_decode_gpu_enabled():
    """Whether the custom-image generators decode PNG files this way: only with ``SSD_PNG_DECODE_GPU=1``.  Opt-in
    (DESIGN.md section 7 has the measurement); the pixels are the same either way."""
    import os
    return os.environ.get("SSD_PNG_DECODE_GPU", "0") == "1"


class PngScanlines(object):
    """One PNG file after the host half: ``info`` (``ssd_hip.PngInfo``) and ``filtered`` (uint8, what inflate returned:
    ``height`` rows of one filter byte and ``row_bytes`` filtered bytes)."""
    __slots__ = ("info", "filtered")

    def __init__(self, info, filtered):
        self.info, self.filtered = info, filtered


def _png_parse(blob):
    """``ssd_hip.PngInfo`` of a file the library decodes, else None (no PNG at all, unsupported or malformed: Pillow's
    business)."""
    import ctypes
    import ssd_hip as _h
    if blob[:8] != _h.PNG_SIGNATURE:
        return None
    info = _h.PngInfo()
    rc = _h.lib().ssd_png_parse(blob, len(blob), ctypes.byref(info))
    return info if rc == 0 else None


def _png_inflate(blob, info):
    """The file's filtered scanlines (uint8), or None: a zlib error, a stream that does not end where the image does
    (never more than one byte beyond the image is decompressed), bytes behind the stream's end, a filter byte above 4,
    or more pixels than Pillow opens without a warning."""
    import ctypes
    import zlib
    import ssd_hip as _h
    from PIL import Image
    if Image.MAX_IMAGE_PIXELS is not None and info.width * info.height > Image.MAX_IMAGE_PIXELS:
        return None
    stream = np.empty(int(info.idat_bytes), np.uint8)
    if _h.lib().ssd_png_idat(blob, len(blob), ctypes.byref(info), stream.ctypes.data, stream.nbytes) != 0:
        return None
    expected = int(info.stream_bytes)
    z = zlib.decompressobj()
    try:
        data = z.decompress(stream, expected + 1)
    except zlib.error:
        return None
    if len(data) != expected or not z.eof or z.unused_data or z.unconsumed_tail:
        return None
    filtered = np.frombuffer(data, np.uint8)
    if int(filtered[::1 + int(info.row_bytes)].max()) > 4:
        return None
    return filtered


def png_host_inflate(blob, fallback=_pillow_rgb):
    """The host half for one file's bytes, for a worker thread: ``PngScanlines``, or -- a file the library calls
    unsupported or invalid, a stream inflate refuses, or no PNG at all -- ``fallback(blob)``'s uint8 ``[H,W,3]`` pixels."""
    blob = bytes(blob)
    info = _png_parse(blob)
    filtered = _png_inflate(blob, info) if info is not None else None
    return PngScanlines(info, filtered) if filtered is not None else fallback(blob)


def png_inflate_gpu_enabled():
    """Whether PNG files are inflated on the device too (``ssd_png_inflate``): only with ``SSD_PNG_INFLATE_GPU=1``, and in
    the generators only beside ``SSD_PNG_DECODE_GPU=1``.  Opt-in ("PNG inflate on the device", has
    the measurement); the pixels are the same either way."""
    import os
    return os.environ.get("SSD_PNG_INFLATE_GPU", "0") == "1"


class PngStream(object):
    """One PNG file after parse only: ``info`` (``ssd_hip.PngInfo``) and ``blob``, the file's bytes.  Its zlib stream is
    inflated on the device (``ssd_png_inflate``); the host never sees a pixel of it."""
    __slots__ = ("info", "blob")

    def __init__(self, info, blob):
        self.info, self.blob = info, blob


def png_host_parse(blob, fallback=_pillow_rgb):
    """The host half for one file's bytes when inflate runs on the device, for a worker thread: parse and CRCs only.
    ``PngStream``; for a file the library calls unsupported or invalid, no PNG at all, or more pixels than Pillow opens
    without a warning, ``fallback(blob)``'s uint8 ``[H,W,3]`` pixels; for a stream longer than ``ssd_png_inflate`` takes
    (``ssd_hip.PNG_INFLATE_MAX_STREAM``), what ``png_host_inflate`` returns."""
    import ssd_hip as _h
    from PIL import Image
    blob = bytes(blob)
    info = _png_parse(blob)
    if info is None or (Image.MAX_IMAGE_PIXELS is not None and info.width * info.height > Image.MAX_IMAGE_PIXELS):
        return fallback(blob)
    if info.stream_bytes > _h.PNG_INFLATE_MAX_STREAM:
        return png_host_inflate(blob, fallback)
    return PngStream(info, blob)


def _png_items(blobs, fallback):
    """Every entry as ``PngScanlines``, ``PngStream`` (files' bytes only with ``SSD_PNG_INFLATE_GPU=1``) or a uint8
    ``[H,W,3]`` array (raw pixels)."""
    items = []
    host_half = png_host_parse if png_inflate_gpu_enabled() else png_host_inflate
    for x in blobs:
        if isinstance(x, (bytes, bytearray, memoryview)):
            x = host_half(x, fallback)
        if not isinstance(x, (PngScanlines, PngStream)):
            x = np.asarray(x)
            if x.dtype != np.uint8 or x.ndim != 3 or x.shape[2] != 3:
                raise ValueError("raw images must be uint8 [H,W,3], got %s %s" % (x.dtype, tuple(x.shape)))
        items.append(x)
    return items


def _png_decode_layout(items):
    """Where one ``ssd_png_decode`` call's input sits in ONE buffer: descriptors | output descriptors | 768-byte palettes |
    chain lists | per image its filtered scanlines, each part at a multiple of 16 bytes; and where the output images go.
    A raw image travels as 8-bit RGB scanlines with filter byte 0: every row a chain of its own."""
    import ssd_hip as _h
    B = len(items)
    desc = np.zeros(B, _h.PNG_DEC_DESC_DTYPE)
    out_desc = np.zeros(B, _h.IMAGE_DESC_DTYPE)
    chains, kinds, streams = [], [], []
    for b, x in enumerate(items):
        d = desc[b]
        if isinstance(x, PngScanlines):
            i = x.info
            d["H"], d["W"], d["depth"], d["color_type"] = i.height, i.width, i.depth, i.color_type
            types = x.filtered[::1 + int(i.row_bytes)]
            starts = np.flatnonzero(types <= 1).astype(np.int32)
            chains.append(starts if len(starts) and starts[0] == 0 else np.concatenate([np.zeros(1, np.int32), starts]))
            kinds.append(_h.PNG_SCANLINES)
            streams.append(int(i.stream_bytes))
        else:
            d["H"], d["W"], d["depth"], d["color_type"] = x.shape[0], x.shape[1], 8, 2
            chains.append(np.arange(x.shape[0], dtype=np.int32))
            kinds.append(_h.JPEG_RAW)
            streams.append(x.shape[0] * (1 + 3 * x.shape[1]))
    palettes = [b for b, x in enumerate(items) if isinstance(x, PngScanlines) and x.info.color_type == 3]
    starts, total = _place([desc.nbytes, out_desc.nbytes] + [768] * len(palettes) + [4 * len(c) for c in chains] + streams)
    out_at = starts[1]
    for b, at in zip(palettes, starts[2:]):
        desc[b]["palette_offset"] = at
    desc["chain_offset"] = starts[2 + len(palettes):2 + len(palettes) + B]
    desc["src_offset"] = starts[2 + len(palettes) + B:]
    rgb_bytes = raw = n_chains = rows = 0
    for b in range(B):
        d = desc[b]
        H, W = int(d["H"]), int(d["W"])
        d["chains"], d["chain_start"], d["row_start"], d["raw_offset"], d["dst_offset"] = len(chains[b]), n_chains, rows, raw, rgb_bytes
        out_desc[b]["H"], out_desc[b]["W"], out_desc[b]["src_offset"] = H, W, rgb_bytes
        n_chains += len(chains[b])
        rows += H
        raw += _round16(streams[b] - H)
        rgb_bytes += _round16(H * W * 3)
    return {"desc": desc, "out_desc": out_desc, "out_at": out_at, "total": total, "rgb_bytes": rgb_bytes, "raw_bytes": raw,
            "chains": chains, "kinds": kinds}


def _png_decode_fill(host, items, layout):
    import ssd_hip as _h
    desc, palette = layout["desc"], _h.PngInfo.palette
    _put(host, 0, desc)
    _put(host, layout["out_at"], layout["out_desc"])
    for b, x in enumerate(items):
        d = desc[b]
        _put(host, int(d["chain_offset"]), layout["chains"][b])
        at = int(d["src_offset"])
        if isinstance(x, PngScanlines):
            if x.info.color_type == 3:
                _put(host, int(d["palette_offset"]), np.frombuffer(x.info, np.uint8)[palette.offset:palette.offset + palette.size])
            _put(host, at, x.filtered)
        else:
            H, n = x.shape[0], 3 * x.shape[1]
            rows = host[at:at + H * (1 + n)].reshape(H, 1 + n)
            rows[:, 0] = 0
            rows[:, 1:] = x.reshape(H, n)


def _png_stream_layout(items):
    """``_png_decode_layout`` for a batch with at least one ``PngStream``.  The UPLOAD holds descriptors | output
    descriptors | inflate descriptors | 768-byte palettes | the host-built chain lists and scanlines of ``PngScanlines`` and
    raw entries | per ``PngStream`` its joined IDAT payload.  BEHIND the upload, device memory only: per ``PngStream`` the
    scanlines ``ssd_png_inflate`` writes and its H-slot chain list.  ``ssd_png_decode`` wants its images' scanlines in
    ascending order, so its descriptors run over the host-built entries first and the streams after them (``order``); the
    output descriptors stay in the list's order."""
    import ssd_hip as _h
    B = len(items)
    order = [b for b, x in enumerate(items) if not isinstance(x, PngStream)] + [b for b, x in enumerate(items) if isinstance(x, PngStream)]
    n_host = sum(1 for x in items if not isinstance(x, PngStream))
    desc = np.zeros(B, _h.PNG_DEC_DESC_DTYPE)
    out_desc = np.zeros(B, _h.IMAGE_DESC_DTYPE)
    inflate = np.zeros(B - n_host, _h.PNG_INFLATE_DESC_DTYPE)
    chains, kinds, streams = {}, [0] * B, []
    for k, b in enumerate(order):
        x, d = items[b], desc[k]
        if isinstance(x, np.ndarray):
            d["H"], d["W"], d["depth"], d["color_type"] = x.shape[0], x.shape[1], 8, 2
            chains[k] = np.arange(x.shape[0], dtype=np.int32)
            kinds[b] = _h.JPEG_RAW
            streams.append(x.shape[0] * (1 + 3 * x.shape[1]))
            continue
        i = x.info
        d["H"], d["W"], d["depth"], d["color_type"] = i.height, i.width, i.depth, i.color_type
        kinds[b] = _h.PNG_SCANLINES
        streams.append(int(i.stream_bytes))
        if isinstance(x, PngScanlines):
            starts = np.flatnonzero(x.filtered[::1 + int(i.row_bytes)] <= 1).astype(np.int32)
            chains[k] = starts if len(starts) and starts[0] == 0 else np.concatenate([np.zeros(1, np.int32), starts])
    palettes = [k for k, b in enumerate(order) if not isinstance(items[b], np.ndarray) and items[b].info.color_type == 3]
    heights = [int(desc[k]["H"]) for k in range(B)]
    upload = ([desc.nbytes, out_desc.nbytes, inflate.nbytes] + [768] * len(palettes) + [4 * len(chains[k]) for k in range(n_host)]
              + streams[:n_host] + [int(items[b].info.idat_bytes) for b in order[n_host:]])
    starts, total = _place(upload)
    behind, device_total = _place(streams[n_host:] + [4 * heights[k] for k in range(n_host, B)], total)
    out_at, inflate_at = starts[1], starts[2]
    at = 3
    for k, where in zip(palettes, starts[at:]):
        desc[k]["palette_offset"] = where
    at += len(palettes)
    desc["chain_offset"] = starts[at:at + n_host] + behind[B - n_host:]
    desc["src_offset"] = starts[at + n_host:at + 2 * n_host] + behind[:B - n_host]
    inflate["zlib_offset"] = starts[at + 2 * n_host:]
    rgb_bytes = raw = n_chains = rows = 0
    for k, b in enumerate(order):
        d = desc[k]
        H, W = int(d["H"]), int(d["W"])
        d["chains"] = len(chains[k]) if k < n_host else H
        d["chain_start"], d["row_start"], d["raw_offset"], d["dst_offset"] = n_chains, rows, raw, rgb_bytes
        out_desc[b]["H"], out_desc[b]["W"], out_desc[b]["src_offset"] = H, W, rgb_bytes
        if k >= n_host:
            f, i = inflate[k - n_host], items[b].info
            f["zlib_bytes"], f["dst_offset"], f["chain_offset"], f["row_bytes"], f["H"] = i.idat_bytes, d["src_offset"], d["chain_offset"], i.row_bytes, H
        n_chains += int(d["chains"])
        rows += H
        raw += _round16(streams[k] - H)
        rgb_bytes += _round16(H * W * 3)
    return {"desc": desc, "out_desc": out_desc, "out_at": out_at, "inflate": inflate, "inflate_at": inflate_at, "total": total,
            "device_total": device_total, "rgb_bytes": rgb_bytes, "raw_bytes": raw, "chains": chains, "kinds": kinds, "order": order,
            "n_host": n_host}


def _png_stream_fill(host, items, layout):
    """The upload of ``_png_stream_layout``: ``ssd_png_idat`` writes each ``PngStream``'s payload straight into the staging
    buffer."""
    import ctypes
    import ssd_hip as _h
    desc, inflate, palette, n_host = layout["desc"], layout["inflate"], _h.PngInfo.palette, layout["n_host"]
    _put(host, 0, desc)
    _put(host, layout["out_at"], layout["out_desc"])
    _put(host, layout["inflate_at"], inflate)
    for k, b in enumerate(layout["order"]):
        x, d = items[b], desc[k]
        if not isinstance(x, np.ndarray) and x.info.color_type == 3:
            _put(host, int(d["palette_offset"]), np.frombuffer(x.info, np.uint8)[palette.offset:palette.offset + palette.size])
        if k >= n_host:
            f = inflate[k - n_host]
            rc = _h.lib().ssd_png_idat(x.blob, len(x.blob), ctypes.byref(x.info), host.ctypes.data + int(f["zlib_offset"]), int(f["zlib_bytes"]))
            _h.check(rc, "ssd_png_idat")
            continue
        _put(host, int(d["chain_offset"]), layout["chains"][k])
        at = int(d["src_offset"])
        if isinstance(x, PngScanlines):
            _put(host, at, x.filtered)
        else:
            H, n = x.shape[0], 3 * x.shape[1]
            rows = host[at:at + H * (1 + n)].reshape(H, 1 + n)
            rows[:, 0] = 0
            rows[:, 1:] = x.reshape(H, n)


def _check_out_u8(out_u8, nbytes, dev):
    """``out_u8`` of the decode functions: a contiguous 1-D uint8 device tensor, 16-byte aligned and long enough."""
    import torch
    if (not isinstance(out_u8, torch.Tensor) or out_u8.dtype != torch.uint8 or out_u8.device != dev or out_u8.dim() != 1
            or not out_u8.is_contiguous() or out_u8.numel() < nbytes or out_u8.data_ptr() % 16):
        raise ValueError("out_u8 must be a contiguous 1-D uint8 device tensor of at least %d bytes, 16-byte aligned" % nbytes)
    return out_u8


def decode_png_batch(blobs, out_u8=None, fallback=_pillow_rgb):
    """A list of PNG files' ``bytes`` -> their pixels on the GPU, bitwise ``PIL.Image.open(...).convert("RGB")``'s, as a
    ``JpegBatch`` (the same object ``decode_jpeg_batch`` returns).  Per batch: parse and inflate on the host, ONE upload
    of the filtered scanlines, ONE ``ssd_png_decode`` call (two launches).  A file the library refuses (16-bit grey,
    interlaced, malformed, ...) is decoded by ``fallback`` -- Pillow, exactly as before, raising what it raised before --
    and travels as raw pixels in the same upload; entries may also be ``PngScanlines`` from ``png_host_inflate`` (the
    data pool's threads) or uint8 ``[H,W,3]`` arrays.  ``kinds``: per image ``ssd_hip.PNG_SCANLINES`` or
    ``ssd_hip.JPEG_RAW``.  ``out_u8`` as ``decode_jpeg_batch``'s; nothing outside the images is written.
    With ``SSD_PNG_INFLATE_GPU=1`` the files' bytes become ``PngStream`` entries (``png_host_parse``; such entries are taken
    either way): the upload carries their IDAT payloads instead of scanlines, ``ssd_png_inflate`` writes the scanlines and
    the chain lists behind the upload, ``ssd_png_decode`` follows, then ONE small read of the status words.  If any is
    nonzero, every ``PngStream`` of the batch goes through ``png_host_inflate`` (a bad stream ends at ``fallback``, raising
    what it raised before) and the batch runs again on the host-inflate road; ``kinds`` stays ``PNG_SCANLINES``."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    lib = _h.lib()
    items = _png_items(blobs, fallback)
    B = len(items)
    if B == 0:
        _h.check(lib.ssd_png_decode(None, 0, None, None, 0, None, 0, None, 0, _h.stream()), "decode_png_batch")
        return JpegBatch([], torch.empty(0, dtype=torch.uint8, device=dev), np.zeros(0, _h.IMAGE_DESC_DTYPE), 0, None, [])
    on_device = any(isinstance(x, PngStream) for x in items)
    if on_device:
        layout = _png_stream_layout(items)
        packed = _upload_packed(dev, layout["total"], lambda host: _png_stream_fill(host, items, layout), device_total=layout["device_total"])
    else:
        layout = _png_decode_layout(items)
        packed = _upload_packed(dev, layout["total"], lambda host: _png_decode_fill(host, items, layout))
    if out_u8 is None or out_u8 is False:
        rgb = torch.empty(max(layout["rgb_bytes"], 16), dtype=torch.uint8, device=dev)
    else:
        rgb = _check_out_u8(out_u8, layout["rgb_bytes"], dev)
    desc, out_desc = layout["desc"], layout["out_desc"]
    assert layout["raw_bytes"] == lib.ssd_png_decode_workspace_bytes(desc.ctypes.data, B)
    ws = _h.workspace(max(layout["raw_bytes"], 16))
    base = packed.data_ptr()
    if on_device:
        inflate = layout["inflate"]
        status = torch.empty(len(inflate), dtype=torch.int32, device=dev)
        _h.check(lib.ssd_png_inflate(base, packed.numel(), inflate.ctypes.data, base + layout["inflate_at"], len(inflate), _h.ptr(status),
                                     _h.stream()), "decode_png_batch")
    _h.check(lib.ssd_png_decode(base, packed.numel(), desc.ctypes.data, base, B, _h.ptr(rgb), rgb.numel(), _h.ptr(ws), ws.numel(),
                                _h.stream()), "decode_png_batch")
    if on_device and bool(status.cpu().any()):                                    # ONE small read; the host road decides, for every stream
        redone = [png_host_inflate(x.blob, fallback) if isinstance(x, PngStream) else x for x in items]
        return decode_png_batch(redone, out_u8=out_u8, fallback=fallback)
    images = [rgb[int(o["src_offset"]):int(o["src_offset"]) + int(o["H"]) * int(o["W"]) * 3].view(int(o["H"]), int(o["W"]), 3)
              for o in out_desc]
    return JpegBatch(images, rgb, out_desc, base + layout["out_at"], packed, layout["kinds"])


def _is_png(x):
    import ssd_hip as _h
    return isinstance(x, (PngScanlines, PngStream)) or (isinstance(x, (bytes, bytearray, memoryview)) and bytes(x[:8]) == _h.PNG_SIGNATURE)


def decode_image_batch(blobs, out_u8=None, fallback=_pillow_rgb):
    """A mixed list -- JPEG files' bytes, PNG files' bytes, host-half items of either codec (``JpegCoefficients``,
    ``PngScanlines``), uint8 ``[H,W,3]`` arrays -- -> ONE packed ``rgb`` buffer and ONE descriptor array in the list's
    order, as a ``JpegBatch``.  The JPEG and raw entries go through ``decode_jpeg_batch`` into the front of the buffer, the
    PNG entries through ``decode_png_batch`` (``ssd_png_decode``) into the rest; a list without PNG entries calls nothing
    of the PNG road.  ``kinds``: per image ``JPEG_COEFFICIENTS``, ``JPEG_RAW`` or ``PNG_SCANLINES``."""
    import torch
    import ssd_hip as _h
    dev = _h.device()
    blobs = list(blobs)
    png = [b for b, x in enumerate(blobs) if _is_png(x)]
    if not png:
        return decode_jpeg_batch(blobs, out_u8=out_u8, fallback=fallback)
    taken = set(png)
    rest = [b for b in range(len(blobs)) if b not in taken]
    png_items = _png_items([blobs[b] for b in png], fallback)
    rest_items = _jpeg_items([blobs[b] for b in rest], fallback)

    def size(x):
        H, W = (x.info.height, x.info.width) if hasattr(x, "info") else x.shape[:2]
        return _round16(int(H) * int(W) * 3)
    front = sum(size(x) for x in rest_items)
    total = front + sum(size(x) for x in png_items)
    rgb = torch.empty(max(total, 16), dtype=torch.uint8, device=dev) if out_u8 is None or out_u8 is False else _check_out_u8(out_u8, total, dev)
    parts = [(png, decode_png_batch(png_items, out_u8=rgb[front:], fallback=fallback), front)]
    if rest:
        parts.append((rest, decode_jpeg_batch(rest_items, out_u8=rgb[:max(front, 16)], fallback=fallback), 0))
    desc = np.zeros(len(blobs), _h.IMAGE_DESC_DTYPE)
    kinds = [0] * len(blobs)
    for where, batch, at in parts:
        for b, o, k in zip(where, batch.desc, batch.kinds):
            desc[b]["H"], desc[b]["W"], desc[b]["src_offset"] = o["H"], o["W"], int(o["src_offset"]) + at
            kinds[b] = k
    desc_dev = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    images = [rgb[int(o["src_offset"]):int(o["src_offset"]) + int(o["H"]) * int(o["W"]) * 3].view(int(o["H"]), int(o["W"]), 3)
              for o in desc]
    return JpegBatch(images, rgb, desc, desc_dev.data_ptr(), (desc_dev, [p[1].packed for p in parts]), kinds)


def preprocess_image_batch(blobs, final_height, final_width, out=None, fallback=_pillow_rgb):
    """``preprocess_jpeg_batch`` for a mixed list (``decode_image_batch``): bitwise ``preprocess_ragged_batch([Pillow's
    decode of each], ...)``."""
    import torch
    import ssd_hip as _h
    fh, fw = int(final_height), int(final_width)
    B = len(blobs)
    out = _check_out(out, (B, fh, fw, 3), torch.float32, _h.device(), create=True)
    jb = decode_image_batch(blobs, fallback=fallback)
    _h.check(_h.lib().ssd_preprocess_ragged(_h.ptr(jb.rgb), jb.rgb.numel(), jb.desc.ctypes.data, jb.desc_ptr, B, 3, fh, fw,
                                            _h.ptr(out), _h.stream()), "preprocess_image_batch")
    return out


def resize_lanczos_image_batch(blobs, final_height, final_width, out=None, out_u8=None, fallback=_pillow_rgb):
    """``resize_lanczos_jpeg_batch`` for a mixed list (``decode_image_batch``): bitwise ``resize_lanczos_batch([Pillow's
    decode of each], ...)``."""
    import torch
    import ssd_hip as _h
    fh, fw = int(final_height), int(final_width)
    dev = _h.device()
    B = len(blobs)
    out = _check_out(out, (B, fh, fw, 3), torch.float32, dev, create=True)
    _check_out(out_u8, (B, fh, fw, 3), torch.uint8, dev, "out_u8")
    if _lanczos_nothing_to_pack(B, 3, fh, fw, out, out_u8, "resize_lanczos_image_batch"):
        return out
    jb = decode_image_batch(blobs, fallback=fallback)
    layout = _lanczos_layout([(int(o["H"]), int(o["W"])) for o in jb.desc], fh, fw, src_offsets=jb.desc["src_offset"])
    packed = _upload_packed(dev, layout["total"], lambda host: _lanczos_fill(host, [], layout))
    _lanczos_launch(packed, layout, out, out_u8, src=jb.rgb, what="resize_lanczos_image_batch")
    return out


def data_workers(workers=None):
    """Size of the decoding pool: ``workers``, else ``SSD_DATA_WORKERS``, else 8; always within 1..16 (never the
    machine's CPU count: the pool shares the host with the training loop and with other jobs)."""
    import os
    n = int(workers) if workers else int(os.environ.get("SSD_DATA_WORKERS", "0") or 0) or 8
    return max(1, min(n, 16))


class voc_batches(object):
    """The reference's ``dataset.map(preprocessing).padded_batch(batch_size)`` (trainer.py:42-48, predictor.py:40-43) with
    one upload and one launch per batch: iterating yields ``(imgs device float32 [b,h,w,3], gt_boxes [b,G,4], gt_labels
    [b,G])``, bitwise what ``padded_batch(preprocessing(item, h, w, evaluate=evaluate) for item in dataset)`` yields.
    ``dataset``: a ``voc_utils.VocDataset`` (its images are decoded by a pool of ``data_workers(workers)`` threads --
    Pillow releases the GIL while it decodes -- at most ``prefetch`` batches ahead of the one the consumer is about to
    get, so up to ``prefetch + 1`` batches of decoded images are held) or any iterable of tfds-shaped dicts (already
    decoded).  A pass that is abandoned half-way (``train_utils.generator`` after the last step) shuts its pool down
    when the generator is closed or collected: decodes not yet started are cancelled, the few in flight are waited
    for.  The order is the dataset's whatever the worker count.  ``augmentation_fn``: the batched
    ``augmentation.apply_batch``, applied after the resize as the reference does.  Every ``iter()`` is a fresh pass (a
    shuffled dataset draws a new order), so ``train_utils.generator`` can cycle it.  ``keep_difficult``: as in
    ``preprocessing`` -- no object is dropped and a fourth item ``gt_difficult`` (uint8 [b,G], padding 0) is yielded."""

    def __init__(self, dataset, batch_size, final_height, final_width, evaluate=False, augmentation_fn=None, workers=None,
                 prefetch=2, keep_difficult=False):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.size = (int(final_height), int(final_width))
        self.evaluate, self.augmentation_fn = bool(evaluate), augmentation_fn
        self.keep_difficult = bool(keep_difficult)
        self.workers, self.prefetch = data_workers(workers), max(int(prefetch), 0)

    def _decode_jobs(self):
        """``(callable, argument)`` per item, in order: calling it gives the decoded tfds-shaped dict."""
        if hasattr(self.dataset, "iter_records"):
            load = self._load_encoded if jpeg_gpu_enabled() and hasattr(self.dataset, "load_encoded") else self.dataset.load
            return ((load, r) for r in self.dataset.iter_records())
        return ((_identity, item) for item in self.dataset)

    def __iter__(self):
        import collections
        import itertools
        from concurrent.futures import ThreadPoolExecutor
        jobs = self._decode_jobs()
        pending = collections.deque()
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="ssd-data")
        try:
            def submit_next():
                chunk = list(itertools.islice(jobs, self.batch_size))
                if chunk:
                    pending.append([pool.submit(fn, arg) for fn, arg in chunk])
                return bool(chunk)
            more = submit_next()
            while pending:
                while more and len(pending) <= self.prefetch:
                    more = submit_next()
                items = [f.result() for f in pending.popleft()]
                yield self._batch(items)
        finally:
            pool.shutdown(wait=True, cancel_futures=True)

    def _load_encoded(self, record):
        """The pool's job unless ``SSD_JPEG_GPU=0``: read the file, parse it, entropy-decode it (no pixels yet) -- or, with
        ``SSD_JPEG_ENTROPY_DECODE_GPU=1``, only plan its scan."""
        item = self.dataset.load_encoded(record)
        if "image" not in item:
            decode = jpeg_host_plan if jpeg_entropy_decode_gpu_enabled() else jpeg_host_decode
            item["image"] = decode(item.pop("image_bytes"))
        return item

    def _batch(self, items):
        images = [it["image"] for it in items]
        if any(isinstance(im, JpegCoefficients) for im in images):
            imgs = preprocess_jpeg_batch(images, self.size[0], self.size[1])
        else:
            imgs = preprocess_ragged_batch(images, self.size[0], self.size[1])
        drop = self.evaluate and not self.keep_difficult
        gt_boxes, gt_labels = _pad_ground_truth([_ground_truth(it, drop) for it in items], get_padding_values())
        if self.augmentation_fn:
            imgs, gt_boxes = self.augmentation_fn(imgs, gt_boxes, gt_labels)
        if self.keep_difficult:
            return imgs, gt_boxes, gt_labels, _pad_flags([_difficult(it) for it in items], gt_labels.shape[1])
        return imgs, gt_boxes, gt_labels


def _identity(x):
    return x


def _pad_ground_truth(pairs, pv):
    """``padded_batch``'s ground truth: ``(boxes [g,4], labels [g])`` pairs padded to the longest (at least 1) with
    ``pv[1]`` / ``pv[2]``."""
    g = max([len(bb) for bb, _ in pairs] + [1])
    gt = np.full((len(pairs), g, 4), pv[1], np.float32)
    gl = np.full((len(pairs), g), pv[2], np.int32)
    for i, (bb, ll) in enumerate(pairs):
        gt[i, :len(bb)] = np.asarray(bb, np.float32).reshape(-1, 4)
        gl[i, :len(ll)] = np.asarray(ll, np.int32)
    return gt, gl


def _decode_custom_image(img_path):
    """One custom image as uint8 [H,W,3]: PIL decodes (``.convert("RGB")``); ``*.npy`` files hold the array itself."""
    if img_path.endswith(".npy"):
        return np.ascontiguousarray(np.load(img_path))
    from PIL import Image
    return np.asarray(Image.open(img_path).convert("RGB"), dtype=np.uint8)


def _encoded_custom_image(img_path):
    """Unless ``SSD_JPEG_GPU=0``: a JPEG file's bytes (decoded on the GPU); ``*.npy`` and every other format as before."""
    if not img_path.endswith(".npy"):
        with open(img_path, "rb") as f:
            blob = f.read()
        if blob[:2] == _JPEG_SOI:
            return blob
    return _decode_custom_image(img_path)


def _custom_image_item(img_path):
    """With ``SSD_PNG_DECODE_GPU=1``, for a worker thread: the file after its host half -- a PNG parsed and inflated
    (``png_host_inflate``) or, with ``SSD_PNG_INFLATE_GPU=1`` too, parsed only (``png_host_parse``), a JPEG entropy-decoded or planned unless ``SSD_JPEG_GPU=0`` -- or, for ``*.npy`` and every other
    format, its pixels as before."""
    if not img_path.endswith(".npy"):
        import ssd_hip as _h
        with open(img_path, "rb") as f:
            blob = f.read()
        if blob[:8] == _h.PNG_SIGNATURE:
            return (png_host_parse if png_inflate_gpu_enabled() else png_host_inflate)(blob)
        if blob[:2] == _JPEG_SOI and jpeg_gpu_enabled():
            return (jpeg_host_plan if jpeg_entropy_decode_gpu_enabled() else jpeg_host_decode)(blob)
    return _decode_custom_image(img_path)


def _custom_images_resized(img_paths, final_height, final_width, pool=None):
    """The files as one resized batch: JPEG files decoded on the GPU unless ``SSD_JPEG_GPU=0``, PNG files only with
    ``SSD_PNG_DECODE_GPU=1`` (their host halves on ``pool``'s threads when there is one; with ``SSD_PNG_INFLATE_GPU=1`` as
    well that half is parse and CRCs only and inflate runs on the device), the rest by PIL."""
    if png_decode_gpu_enabled():
        items = list(pool.map(_custom_image_item, img_paths)) if pool is not None else [_custom_image_item(p) for p in img_paths]
        return resize_lanczos_image_batch(items, final_height, final_width)
    if jpeg_gpu_enabled():
        return resize_lanczos_jpeg_batch([_encoded_custom_image(p) for p in img_paths], final_height, final_width)
    return resize_lanczos_batch([_decode_custom_image(p) for p in img_paths], final_height, final_width)


def custom_data_generator(img_paths, final_height, final_width):
    """reference utils/data_utils.py:93-108: every image opened with PIL, resized with LANCZOS, then uint8 -> float32
    [0,1] (``tf.image.convert_image_dtype``).  PIL only decodes here: the resize (Pillow's, bit for bit) and the
    conversion run on the GPU (``resize_lanczos_batch``); there is no host resize path.  ``*.npy`` files (uint8 [H,W,3])
    are accepted as well.  Yields ``(img [final_height, final_width, 3] device tensor, gt_boxes [0,4], gt_labels [0])``;
    ``custom_data_batches`` resizes a whole batch per call."""
    for img_path in img_paths:
        yield _custom_images_resized([img_path], final_height, final_width)[0], np.zeros((0, 4), np.float32), np.zeros((0,), np.int32)


def custom_data_batches(img_paths, final_height, final_width, batch_size):
    """``custom_data_generator`` + ``padded_batch`` with one upload and one resize call per batch: yields ``(imgs
    [b,final_height,final_width,3] device tensor, gt_boxes [b,1,4] zeros, gt_labels [b,1] of -1)``, what
    ``padded_batch`` makes of the generator's items (no ground truth: one padding row).  With ``SSD_PNG_DECODE_GPU=1`` the
    files' host halves run on ``data_workers()`` threads; ``SSD_PNG_INFLATE_GPU=1`` beside it moves inflate to the device."""
    pv = get_padding_values()
    img_paths = list(img_paths)
    pool = None
    if png_decode_gpu_enabled():                                                  # the host halves: read, parse, inflate (or not)
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=data_workers(), thread_name_prefix="ssd-data")
    try:
        for i in range(0, len(img_paths), int(batch_size)):
            imgs = _custom_images_resized(img_paths[i:i + int(batch_size)], final_height, final_width, pool)
            yield imgs, np.full((len(imgs), 1, 4), pv[1], np.float32), np.full((len(imgs), 1), pv[2], np.int32)
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)


def padded_batch(items, batch_size, padding_values=None):
    """``Dataset.padded_batch(batch_size, padded_shapes=data_shapes, padding_values=...)`` of the reference
    scripts (predictor.py:43, trainer.py:33-34): consecutive ``(img, gt_boxes, gt_labels)`` items are stacked,
    ground truth padded to the longest of the batch with 0 / -1.  Images stay where they are (device tensors
    are stacked on the device).  Items with a fourth element (``preprocessing(keep_difficult=True)``) give batches
    with a fourth element: the flags as uint8 [b,G], padded with 0."""
    import torch
    pv = padding_values or get_padding_values()
    batch = []

    def flush():
        gt, gl = _pad_ground_truth([(b[1], b[2]) for b in batch], pv)
        imgs = [b[0] for b in batch]
        x = torch.stack(imgs) if isinstance(imgs[0], torch.Tensor) else np.stack(imgs)
        if len(batch[0]) > 3:
            return x, gt, gl, _pad_flags([b[3] for b in batch], gl.shape[1])
        return x, gt, gl

    for it in items:
        batch.append(it)
        if len(batch) == batch_size:
            yield flush()
            batch = []
    if batch:
        yield flush()


def synthetic_voc_items(total_items, total_labels=21, seed=0):
    """Seeded stand-in for ``tfds.load("voc/2007")`` items: dicts ``{"image": uint8 [H,W,3] (VOC-like sizes, H / W
    in 300..500), "objects": {"bbox" [G,4] normalised, "label" [G] in 0..total_labels-2 (``preprocessing`` adds
    1), "is_difficult" [G]}}`` -- what ``preprocessing`` consumes (utils/data_utils.py:7-30)."""
    rng = np.random.default_rng(seed)
    for _ in range(total_items):
        h, w = int(rng.integers(300, 501)), int(rng.integers(300, 501))
        g = int(rng.integers(1, 9))
        c = rng.uniform(0.15, 0.85, (g, 2))
        sz = rng.uniform(0.08, 0.5, (g, 2))
        yield {"image": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
               "objects": {"bbox": np.clip(np.concatenate([c - sz / 2, c + sz / 2], -1), 0, 1).astype(np.float32),
                           "label": rng.integers(0, total_labels - 1, g).astype(np.int64),
                           "is_difficult": rng.random(g) < 0.2}}


def get_padding_values():
    """reference utils/data_utils.py:117-122: image 0, gt boxes 0, gt labels -1."""
    return (np.float32(0), np.float32(0), np.int32(-1))


def synthetic_images(batch, img_size=300, seed=0):
    """uint8->float32 [0,1] images like ``preprocessing`` yields (utils/data_utils.py:22)."""
    return np.random.default_rng(seed).random((batch, img_size, img_size, 3), dtype=np.float32)


def synthetic_gt(batch, max_boxes=16, total_labels=21, seed=3):
    rng = np.random.default_rng(seed)
    gt = np.zeros((batch, max_boxes, 4), np.float32)
    gl = -np.ones((batch, max_boxes), np.int32)
    for b in range(batch):
        g = int(rng.integers(1, max_boxes + 1))
        c = rng.uniform(0.1, 0.9, (g, 2))
        s = rng.uniform(0.05, 0.5, (g, 2))
        gt[b, :g] = np.clip(np.concatenate([c - s / 2, c + s / 2], -1), 0, 1).astype(np.float32)
        gl[b, :g] = rng.integers(1, total_labels, g)
    return gt, gl


def synthetic_dataset(total_items, batch_size, img_size=300, total_labels=21, seed=0):
    """Finite iterable of (img, gt_boxes, gt_labels) padded batches."""
    for i in range(0, total_items, batch_size):
        b = min(batch_size, total_items - i)
        gt, gl = synthetic_gt(b, total_labels=total_labels, seed=seed + 1000 + i)
        yield synthetic_images(b, img_size, seed + i), gt, gl


def synthetic_weights(model, seed=1, target_frac=0.05):
    """Seeded random weights for benchmarks (no pretrained weights offline): He-normal conv
    kernels, BatchNorm gamma 1+-0.1 / beta,mean +-0.1 / var in [0.5,1.5].  The label-head
    background bias is then calibrated ON THE DEVICE (bisection on the model's own output
    for one image) so that ~target_frac of the anchors carry a non-background probability
    above 0.5 -- with purely random weights NMS would have nothing to do."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in model.param_specs:
        var = name.rsplit("/", 1)[1]
        if var == "kernel":
            scale = 0.5 if "label_output" in name else (0.25 if "boxes_output" in name else 1.0)
            w[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2])) * scale).astype(np.float32)
        elif var == "depthwise_kernel":
            w[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / 9.0)).astype(np.float32)
        elif var == "gamma":
            w[name] = rng.uniform(0.9, 1.1, shape).astype(np.float32)
        elif var in ("beta", "moving_mean"):
            w[name] = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
        elif var == "moving_variance":
            w[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif var == "scale":
            w[name] = np.full(shape, 20.0, np.float32)
        else:
            w[name] = rng.uniform(-0.05, 0.05, shape).astype(np.float32)
    model.set_weights(w)
    _, probs = model(synthetic_images(1, model.img_size, seed=0))
    logp = np.log(np.maximum(probs[0].double().cpu().numpy(), 1e-300))

    def frac(t, g=1.0):
        lg = logp * g
        lg[:, 0] += t
        e = np.exp(lg - lg.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        return float(((p.argmax(-1) != 0) & (p.max(-1) > 0.5)).mean())
    # log-probabilities are the logits up to a per-row constant (valid while the softmax is not
    # saturated, which holds for the un-gained random heads).  If the class spread is too small
    # for any class to pass 0.5 (VGG16), scale the label kernels and biases by g first: the
    # logits scale by g exactly.
    g = 1.0
    while frac(-1e4, g) < 3 * target_frac and g < 64:
        g *= 2.0
    lo, hi = -50.0 * g, 50.0 * g
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if frac(mid, g) > target_frac:
            lo = mid
        else:
            hi = mid
    L = model.total_labels
    upd = {}
    for i in range(1, 7):
        b = w["%d_conv_label_output/bias" % i] * np.float32(g)
        b[0::L] += np.float32(0.5 * (lo + hi))
        w["%d_conv_label_output/bias" % i] = b
        upd["%d_conv_label_output/bias" % i] = b
        if g != 1.0:
            k = w["%d_conv_label_output/kernel" % i] * np.float32(g)
            w["%d_conv_label_output/kernel" % i] = k
            upd["%d_conv_label_output/kernel" % i] = k
    model.set_weights(upd)
    return w
