"""Drop-in for the reference's ``utils/drawing_utils.py`` (same names and argument order) with the pixels produced on
the GPU: ``ssd_image_minmax`` + ``ssd_draw_detections`` reproduce ``array_to_img`` and the per-box PIL loop
(``ImageDraw.text`` in the legacy bitmap font, ``ImageDraw.rectangle(outline, width=3)``) to the byte in one pass over
the batch, ``ssd_draw_bounding_boxes`` is ``tf.image.draw_bounding_boxes``.

Differences from the reference, all additions:
  * nothing calls ``plt.show()`` unless ``show=True``; every function RETURNS the annotated images (device tensors),
    ``out=`` receives them, ``out_dir=`` also saves PNGs through PIL;
  * the colours the reference draws afresh on every call (``tf.random.uniform((len(labels), 4), maxval=256)``) come from a
    module generator (``seed(s)``), or from ``colors=``;
  * ``draw_detections_batch`` is the batched entry point: one upload of boxes and text and one call per batch.

Text: ``"{0} {1:0.3f}".format(labels[i], prob)`` is formatted on the host.  Characters outside printable ASCII
(32..126) raise ``ValueError`` (Pillow would draw Latin-1 glyphs for 160..255 and nothing for the rest; no label of the
reference needs them).  Pillow is needed once per process, to read the glyphs of its bitmap font; no font data lives here.
"""
import os

import numpy as np
import torch

import ssd_hip as _h
from utils import bbox_utils

OUTLINE_WIDTH = 3              # drawing_utils.py:69
TEXT_OFFSET = (4, 2)           # drawing_utils.py:68: text at (x1 + 4, y1 + 2)
GLYPH_ADVANCE, GLYPH_HEIGHT = 6, 11
MAX_TEXT = 64                  # ssd_draw_detections: maxlen cap
MAX_BOXES = 4096               # ssd_draw_detections: T cap
_COORD_LIMIT = 1 << 30

_rng = np.random.default_rng()
_atlas_host = None
_atlas_dev = {}


def seed(s):
    """Reseed the generator the default colours are drawn from (the reference uses TF's global generator)."""
    global _rng
    _rng = np.random.default_rng(s)


def random_colors(total_labels):
    """drawing_utils.py:55: ``tf.random.uniform((len(labels), 4), maxval=256, dtype=tf.int32)`` from the module generator."""
    return _rng.integers(0, 256, size=(int(total_labels), 4), dtype=np.int64)


def bitmap_font():
    """The font ``ImageDraw.text`` used without ``font=`` in the reference's Pillow: the legacy bitmap font."""
    from PIL import ImageFont
    load = getattr(ImageFont, "load_default_imagefont", None) or ImageFont.load_default
    return load()


def _render(font, s):
    from PIL import Image, ImageDraw
    im = Image.new("L", (GLYPH_ADVANCE * len(s), GLYPH_HEIGHT), 0)
    ImageDraw.Draw(im).text((0, 0), s, fill=255, font=font)
    return np.asarray(im) != 0


def glyph_atlas():
    """uint32 ``[96,4]`` (read-only, cached): what ``ssd_draw_detections`` needs of Pillow's bitmap font, read out of Pillow
    through its public drawing calls.  Per glyph (95 printable ASCII characters, then a blank one): 11 row bytes, bit k =
    column k - 1 of the 6-wide cell (column -1 is the overhang into the previous cell), and a word
    ``first box row | end box row << 8 | has column -1 << 16``.  Pillow pastes each glyph's box opaquely in string order and
    the font's boxes are the tight boxes of the ink (tests/test_drawing_cpu.py holds the atlas to ``font.getmask`` on
    every label string and on random strings), so the box is recovered from the ink of ``" " + character``."""
    global _atlas_host
    if _atlas_host is not None:
        return _atlas_host
    font = bitmap_font()
    if _render(font, "Ag").shape != (GLYPH_HEIGHT, 2 * GLYPH_ADVANCE) or tuple(font.getbbox("Ag")[2:]) != (2 * GLYPH_ADVANCE, GLYPH_HEIGHT):
        raise RuntimeError("Pillow's default bitmap font is not the 6 x 11 monospace font the drawing kernel reproduces")
    atlas = np.zeros((96, 4), np.uint32)
    rows = atlas.view(np.uint8).reshape(96, 16)
    for g in range(95):
        ink = _render(font, " " + chr(32 + g))[:, GLYPH_ADVANCE - 1:]          # columns -1 .. 5 of the glyph
        for y in range(GLYPH_HEIGHT):
            rows[g, y] = sum(1 << k for k in range(7) if ink[y, k])
        ys = np.nonzero(ink.any(1))[0]
        if len(ys):
            atlas[g, 3] = int(ys[0]) | (int(ys[-1]) + 1) << 8 | int(ink[:, 0].any()) << 16
    atlas.setflags(write=False)
    _atlas_host = atlas
    return atlas


def format_label(name, prob):
    """drawing_utils.py:67."""
    return "{0} {1:0.3f}".format(name, prob)


def encode_texts(texts, maxlen=None):
    """A list of strings -> (uint8 ``[N,maxlen]``, int32 ``[N]``); ``ValueError`` for a character outside 32..126 and for a
    string longer than ``MAX_TEXT``."""
    raw = []
    for s in texts:
        if any(ord(c) < 32 or ord(c) > 126 for c in s):
            raise ValueError("label text %r has characters outside printable ASCII (32..126)" % (s,))
        if len(s) > MAX_TEXT:
            raise ValueError("label text %r is longer than %d characters" % (s, MAX_TEXT))
        raw.append(s.encode("ascii"))
    longest = max([len(r) for r in raw] + [0])
    if maxlen is None:
        maxlen = longest
    if longest > maxlen or maxlen > MAX_TEXT:
        raise ValueError("maxlen %d does not hold the longest text (%d) or exceeds %d" % (maxlen, longest, MAX_TEXT))
    out = np.zeros((len(raw), maxlen), np.uint8)
    for i, r in enumerate(raw):
        out[i, :len(r)] = np.frombuffer(r, np.uint8)
    return out, np.asarray([len(r) for r in raw], np.int32)


def _host(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype, copy=False)


def _int_boxes(boxes):
    """integer-valued float boxes -> int32; a box with a NaN corner becomes (0,0,0,0), which is skipped"""
    b = _host(boxes, np.float64)
    b = np.where(np.isnan(b).any(-1, keepdims=True), 0.0, b)
    return np.clip(b, -_COORD_LIMIT, _COORD_LIMIT).astype(np.int32)


def _colors_u8(colors, total_labels):
    c = random_colors(total_labels) if colors is None else _host(colors, np.int64)
    if c.ndim != 2 or c.shape[1] not in (3, 4) or c.shape[0] < total_labels:
        raise ValueError("colors must be [>= %d, 3 or 4], got %s" % (total_labels, tuple(c.shape)))
    if c.size and (c.min() < 0 or c.max() > 255):
        raise ValueError("colors must lie in 0..255")
    return np.ascontiguousarray(c[:, :3]).astype(np.uint8)            # an RGB image drops the alpha of a 4-tuple


def _atlas_on(dev):
    t = _atlas_dev.get(dev.index)
    if t is None:
        t = _atlas_dev[dev.index] = torch.from_numpy(glyph_atlas().view(np.int32).copy()).to(dev)
    return t


def _check_out(out, shape, dtype, dev):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s device tensor %s" % (dtype, tuple(shape)))
    return out


def _images(imgs):
    if not isinstance(imgs, torch.Tensor):
        imgs = np.asarray(imgs)
    if imgs.ndim != 4:
        raise ValueError("images must be [B,H,W,C], got %s" % (tuple(imgs.shape),))
    return imgs


def draw_pixel_boxes(imgs, boxes, label_indices, texts, colors, out=None, scale=True, fill=False, width=OUTLINE_WIDTH):
    """The kernel call under every function here.  ``imgs`` float ``[B,H,W,3]``; ``boxes`` ``[B,T,4]`` integer-valued
    pixel corners (y1, x1, y2, x2); ``label_indices`` ``[B,T]`` rows of ``colors`` (uint8 ``[L,3]``); ``texts`` a list of B
    lists of T strings ('' draws nothing) or None.  ``scale``: ``array_to_img``'s min/max scaling (False: the floats
    already hold bytes).  One host buffer, one upload, then ``ssd_image_minmax`` and ``ssd_draw_detections``.  Returns the
    uint8 device tensor ``[B,H,W,3]``."""
    imgs = _images(imgs)
    B, H, W, C = (int(v) for v in imgs.shape)
    ib = _int_boxes(boxes)
    T = int(ib.shape[-2]) if ib.ndim >= 2 else 0
    ib = ib.reshape(B, T, 4)
    lab = _host(label_indices, np.int64).reshape(B, T).clip(-1, 1 << 30).astype(np.int32)
    col = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    if texts is not None and not fill:
        flat = [s for row in texts for s in row]
        if len(flat) != B * T:
            raise ValueError("texts must hold B lists of T strings")
        tb, tl = encode_texts(flat)
    else:
        tb, tl = np.zeros((B * T, 0), np.uint8), np.zeros(B * T, np.int32)
    maxlen = tb.shape[1]
    dev = _h.device()
    x = _h.to_dev(imgs)
    out = _check_out(out, (B, H, W, C), torch.uint8, dev)
    return _launch(x, _upload(ib, lab, tl, col, tb, dev), out, scale, fill, width)


def _upload(ib, lab, tl, col, tb, dev):
    """boxes | labels | lengths | colours | text in one host buffer (boxes first: 16-byte aligned), one copy"""
    parts = [ib.tobytes(), lab.tobytes(), tl.tobytes(), col.tobytes() + b"\0" * (-col.size % 4), tb.tobytes()]
    offs = np.cumsum([0] + [len(p) for p in parts])
    packed = torch.from_numpy(np.frombuffer(b"".join(parts) + b"\0" * 16, np.uint8).copy()).to(dev)
    return {"packed": packed, "offsets": [int(o) for o in offs[:5]], "T": int(ib.shape[1]), "maxlen": int(tb.shape[1]),
            "L": int(col.shape[0])}


def _launch(x, up, out, scale=True, fill=False, width=OUTLINE_WIDTH):
    """``ssd_image_minmax`` (when scaling) and ``ssd_draw_detections`` on resident inputs"""
    B, H, W, C = (int(v) for v in x.shape)
    lib = _h.lib()
    base = up["packed"].data_ptr()
    p_box, p_lab, p_len, p_col, p_txt = (_h.vp(base + o) for o in up["offsets"])
    maxlen = up["maxlen"]
    atlas = _atlas_on(x.device) if (maxlen > 0 and not fill) else None
    mm = None
    if scale and B > 0 and C == 3 and 1 <= H <= _h.MAX_IMAGE_SIDE and 1 <= W <= _h.MAX_IMAGE_SIDE:         # otherwise the library answers below
        mm = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        ws = _h.workspace(lib.ssd_image_minmax_workspace_bytes(B))
        _h.check(lib.ssd_image_minmax(_h.ptr(x), B, H, W, C, _h.ptr(mm), _h.ptr(ws), ws.numel(), _h.stream()), "ssd_image_minmax")
    _h.check(lib.ssd_draw_detections(_h.ptr(x), _h.ptr(mm), B, H, W, C, p_box, p_lab, p_txt if maxlen else None,
                                     p_len if maxlen else None, up["T"], maxlen, p_col, up["L"], _h.ptr(atlas), int(width),
                                     int(bool(fill)), _h.ptr(out), _h.stream()), "ssd_draw_detections")
    return out


def label_texts(int_boxes, label_indices, probs, labels):
    """The reference's loop body on the host (drawing_utils.py:59-67): per box the text it would draw, '' for a box it
    skips.  ``IndexError`` for a drawn box whose label is not in ``labels``."""
    B, T = int_boxes.shape[:2]
    drawn = (int_boxes[..., 3].astype(np.int64) - int_boxes[..., 1] > 0) & (int_boxes[..., 2].astype(np.int64) - int_boxes[..., 0] > 0)
    texts = [[""] * T for _ in range(B)]
    for b, t in zip(*np.nonzero(drawn)):
        li = int(label_indices[b, t])
        if not 0 <= li < len(labels):
            raise IndexError("label index %d of image %d box %d is outside the %d labels" % (li, b, t, len(labels)))
        texts[b][t] = format_label(labels[li], probs[b, t])
    return texts


def draw_detections_batch(imgs, boxes, label_indices, probs, labels, colors=None, out=None):
    """``draw_bboxes_with_labels`` for a whole batch: ``imgs`` float ``[B,H,W,3]``, ``boxes`` NORMALISED ``[B,T,4]``
    (denormalised here with ``bbox_utils.denormalize_bboxes``, which rounds half to even), ``label_indices`` / ``probs``
    ``[B,T]``, ``labels`` the list of names, ``colors`` ``[len(labels), 3 or 4]`` in 0..255 (default: drawn from the module
    generator).  Returns the uint8 device tensor ``[B,H,W,3]`` (``out`` when given)."""
    imgs = _images(imgs)
    B, H, W = int(imgs.shape[0]), int(imgs.shape[1]), int(imgs.shape[2])
    nb = _host(boxes, np.float32)
    T = int(nb.shape[-2]) if nb.ndim >= 2 else 0
    ib = _int_boxes(bbox_utils.denormalize_bboxes(torch.as_tensor(nb).reshape(B, T, 4), H, W))
    li = _host(label_indices, np.float64).reshape(B, T).astype(np.int64)          # int(label_indices[index])
    pr = _host(probs, np.float32).reshape(B, T)
    col = _colors_u8(colors, len(labels))
    return draw_pixel_boxes(imgs, ib, li, label_texts(ib, li, pr, labels), col, out=out)


def draw_bboxes_with_labels(img, bboxes, label_indices, probs, labels, colors=None, out=None, out_dir=None, show=False,
                            out_format="png", out_quality=75):
    """drawing_utils.py:45-73: ``img`` ``[H,W,3]`` float, ``bboxes`` ``[T,4]`` DENORMALISED, ``label_indices`` / ``probs``
    ``[T]``.  The B = 1 case of the batched call; returns the uint8 device tensor ``[H,W,3]``."""
    x = img.unsqueeze(0) if isinstance(img, torch.Tensor) else np.asarray(img)[None]
    _images(x)
    ib = _int_boxes(bboxes).reshape(1, -1, 4)
    T = ib.shape[1]
    li = _host(label_indices, np.float64).reshape(1, T).astype(np.int64)
    pr = _host(probs, np.float32).reshape(1, T)
    col = _colors_u8(colors, len(labels))
    o = draw_pixel_boxes(x, ib, li, label_texts(ib, li, pr, labels), col, out=None if out is None else out.unsqueeze(0))
    _present(o, out_dir, 0, show, out_format, out_quality)
    return o[0]


def draw_predictions(dataset, pred_bboxes, pred_labels, pred_scores, labels, batch_size, colors=None, out_dir=None,
                     show=False, out_format="png", out_quality=75):
    """drawing_utils.py:75-84 as a generator: one uint8 device tensor ``[B,H,W,3]`` per batch of ``dataset`` (items
    ``(imgs, _, _)``), drawn with ONE colour table for the whole run.  ``out_dir``: also writes ``img_%05d.png``, or, with
    ``out_format="jpeg"``, ``img_%05d.jpg`` at ``out_quality`` (encoded from the device tensor: ``_present``)."""
    col = _colors_u8(colors, len(labels))
    for batch_id, image_data in enumerate(dataset):
        imgs = image_data[0]
        start = batch_id * batch_size
        end = start + int(imgs.shape[0])
        o = draw_detections_batch(imgs, pred_bboxes[start:end], pred_labels[start:end], pred_scores[start:end], labels, colors=col)
        _present(o, out_dir, start, show, out_format, out_quality)
        yield o


def draw_bboxes(imgs, bboxes, colors=None, out=None, out_dir=None, show=False, out_format="png", out_quality=75):
    """drawing_utils.py:31-43 -> ``tf.image.draw_bounding_boxes(imgs, bboxes, colors)``: float images ``[B,H,W,3]``,
    normalised boxes ``[B,T,4]``, ``colors`` float ``[L, 3 or 4]`` cycled by box index (default: the reference's red).
    Returns the float32 device tensor ``[B,H,W,3]``."""
    imgs = _images(imgs)
    B, H, W, C = (int(v) for v in imgs.shape)
    dev = _h.device()
    x = _h.to_dev(imgs)
    bx = _h.to_dev(_host(bboxes, np.float32).reshape(B, -1, 4))
    T = int(bx.shape[1])
    c = np.asarray([[1, 0, 0, 1]] if colors is None else _host(colors, np.float32), np.float32)
    if c.ndim != 2 or c.shape[1] not in (3, 4) or c.shape[0] < 1:
        raise ValueError("colors must be [L, 3 or 4]")
    cd = _h.to_dev(np.ascontiguousarray(c[:, :3]))
    out = _check_out(out, (B, H, W, C), torch.float32, dev)
    _h.check(_h.lib().ssd_draw_bounding_boxes(_h.ptr(x), B, H, W, C, _h.ptr(bx), T, _h.ptr(cd), int(cd.shape[0]), _h.ptr(out),
                                              _h.stream()), "ssd_draw_bounding_boxes")
    if out_dir is not None or show:
        _present((out.clamp(0, 1) * 255).to(torch.uint8), out_dir, 0, show, out_format, out_quality)
    return out


def draw_grid_map(img, grid_map, stride, out=None, out_dir=None, show=False, out_format="png", out_quality=75):
    """drawing_utils.py:6-29: a filled white 5 x 5 square at ``grid + stride // 2`` for every row of ``grid_map``
    (``[N,4]``; the reference hands rows (0, 1, 2, 3) to PIL as (x0, y0, x1, y1)).  ``img`` uint8 ``[H,W,3]``.  Returns the
    uint8 device tensor ``[H,W,3]``."""
    a = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img))
    if a.dtype != torch.uint8 or a.dim() != 3:
        raise ValueError("img must be uint8 [H,W,3]")
    g = _host(grid_map, np.int64).reshape(-1, 4)
    h = int(stride) // 2
    x0, y0, x1, y1 = g[:, 0] + h - 2, g[:, 1] + h - 2, g[:, 2] + h + 2, g[:, 3] + h + 2
    if (x1 < x0).any() or (y1 < y0).any():
        raise ValueError("x1 must be greater than or equal to x0, y1 than y0")         # Pillow's own check
    boxes = np.stack([y0, x0, y1, x1], -1)
    white = np.full((1, 3), 255, np.uint8)
    dev = _h.device()
    cur = a.to(dev).unsqueeze(0)
    res = None
    for s in range(0, max(len(boxes), 1), MAX_BOXES):                                  # later squares over earlier ones
        part = boxes[s:s + MAX_BOXES][None]
        last = s + MAX_BOXES >= len(boxes)
        res = draw_pixel_boxes(cur.float(), part, np.zeros(part.shape[:2], np.int64), None, white,
                               out=None if (out is None or not last) else out.unsqueeze(0), scale=False, fill=True)
        cur = res
    _present(res, out_dir, 0, show, out_format, out_quality)
    return res[0]


def _present(images_u8, out_dir, start, show, out_format="png", out_quality=75):
    """``out_dir``: ``img_%05d.png`` from index ``start`` on, through PIL (with ``SSD_PNG_GPU=1``: encoded on the GPU from
    the device tensor by ``data_utils.encode_png_batch`` -- other bytes, the same pixels); with ``out_format="jpeg"``, ``img_%05d.jpg`` at
    quality ``out_quality`` through ``data_utils.encode_jpeg_batch`` -- the drawn tensor is already on the device, so the
    whole batch is one forward-DCT call and the files are Pillow's ``save(f, "JPEG", quality=out_quality)`` bytes.
    ``show``: the reference's matplotlib figures."""
    if out_format not in ("png", "jpeg"):
        raise ValueError('out_format must be "png" or "jpeg", got %r' % (out_format,))
    if out_dir is None and not show:
        return
    if out_dir is not None and out_format == "jpeg":
        from utils import data_utils
        os.makedirs(out_dir, exist_ok=True)
        blobs = data_utils.encode_jpeg_batch(images_u8.detach().contiguous(), quality=out_quality)
        for i, blob in enumerate(blobs):
            with open(os.path.join(out_dir, "img_%05d.jpg" % (start + i)), "wb") as f:
                f.write(blob)
        if not show:
            return
    if out_dir is not None and out_format == "png":
        from utils import data_utils
        if data_utils.png_gpu_enabled():                                               # opt-in (SSD_PNG_GPU=1): the files are made on the GPU
            os.makedirs(out_dir, exist_ok=True)
            for i, blob in enumerate(data_utils.encode_png_batch(images_u8.detach().contiguous())):
                with open(os.path.join(out_dir, "img_%05d.png" % (start + i)), "wb") as f:
                    f.write(blob)
            if not show:
                return
            out_dir = None
    host = images_u8.detach().cpu().numpy()
    if out_dir is not None and out_format == "png":
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        for i, a in enumerate(host):
            Image.fromarray(a).save(os.path.join(out_dir, "img_%05d.png" % (start + i)))
    if show:
        import matplotlib.pyplot as plt
        for a in host:
            plt.figure()
            plt.imshow(a)
            plt.show()
