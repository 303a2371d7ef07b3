"""Diagnostics script (not a test): what encoding annotated detections as JPEG behind the GPU forward DCT
(``ssd_jpeg_forward`` + ``ssd_jpeg_entropy_encode``) buys for the output path.

64 device-resident uint8 images -- 32 drawn 300x300 images (``draw_detections_batch`` on noise-free synthetic pixels with
up to 200 boxes each) and 32 VOC-sized images (H and W in 300..500) -- to ``bytes`` in host memory, quality 75, 4:2:0, the
paths alternating inside this process, every timed window >= 1 s and closed by a device synchronise:
  (a) today's path: one download, then ``PIL.Image.save(..., "PNG")`` per image on the calling thread;
  (b) one download, then a pool of N threads runs Pillow's JPEG encoder (``encode_jpeg_batch`` with
      ``SSD_JPEG_ENCODE_GPU=0``);
  (c) the new path at the same N: ``ssd_jpeg_forward``, one download of the int16 coefficients into pinned memory, the
      pool runs ``ssd_jpeg_entropy_encode``; (b) and (c) for N = 1, 8 and 16;
  (d) ``ssd_jpeg_forward`` alone (its two kernels), device events around K back-to-back calls on resident buffers.
Every figure is the median of --rounds windows with their spread (min .. max).  The outputs of (b) and (c) are compared
byte for byte first.  Usage: python tests/bench_jpeg_encode.py [--rounds 5]"""
import argparse
import io
import os
import statistics
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
from utils import data_utils, drawing_utils
import drawing_cases as dc
import voc_cases as vc
from bench_jpeg import events, spread, window

B, QUALITY, SUBSAMPLING = 32, 75, "4:2:0"
WORKERS = (1, 8, 16)


def images():
    dev = h.device()
    imgs, boxes, labels, scores = dc.ragged_batch(B=B)
    drawn = drawing_utils.draw_detections_batch(h.to_dev(imgs), boxes, labels, scores, dc.LABELS, colors=dc.colors(9))
    rng = np.random.default_rng(0)
    voc = [torch.as_tensor(vc.pixels(int(rng.integers(300, 501)), int(rng.integers(300, 501)), "RGB", seed=i)).to(dev)
           for i in range(B)]
    return list(drawn) + voc


def png_serial(batch):
    from PIL import Image
    out = []
    for t in batch:
        buf = io.BytesIO()
        Image.fromarray(t.cpu().numpy()).save(buf, "PNG")
        out.append(buf.getvalue())
    return out


def encode(batch, gpu, workers):
    os.environ["SSD_JPEG_ENCODE_GPU"] = "1" if gpu else "0"
    return data_utils.encode_jpeg_batch(batch, quality=QUALITY, subsampling=SUBSAMPLING, workers=workers)


def main(rounds):
    assert torch.cuda.is_available(), "bench_jpeg_encode.py measures on the GPU"
    batch = images()
    n_img = len(batch)
    pixels = sum(int(t.shape[0]) * int(t.shape[1]) for t in batch)
    a, b = encode(batch, False, 8), encode(batch, True, 8)
    assert a == b, "the GPU encode differs from Pillow's"
    png = png_serial(batch)
    for n in WORKERS:
        encode(batch, False, n); encode(batch, True, n)
    tp, tb, tc = [], {n: [] for n in WORKERS}, {n: [] for n in WORKERS}
    for _ in range(rounds):
        tp.append(window(lambda: png_serial(batch)))
        for n in WORKERS:
            tb[n].append(window(lambda: encode(batch, False, n)))
            tc[n].append(window(lambda: encode(batch, True, n)))
    print("%d device images (%d drawn 300x300 + %d VOC-sized; %.1f MB of pixels) -> bytes on the host; JPEG quality %d %s: "
          "%.2f MB, bytes equal on both roads; PNG: %.2f MB" % (n_img, B, B, pixels * 3 / 1e6, QUALITY, SUBSAMPLING,
                                                               sum(map(len, a)) / 1e6, sum(map(len, png)) / 1e6))
    print("(a)  download + PIL PNG, calling thread                            : %s = %.0f images/s" % (
        spread(tp, "ms/batch", 1e3), n_img / statistics.median(tp)))
    for n in WORKERS:
        mb, mc = statistics.median(tb[n]), statistics.median(tc[n])
        print("(b)  %2d workers, download + Pillow JPEG pool                        : %s = %.0f images/s" % (
            n, spread(tb[n], "ms/batch", 1e3), n_img / mb))
        print("(c)  %2d workers, ssd_jpeg_forward + download + entropy-encode pool  : %s = %.0f images/s" % (
            n, spread(tc[n], "ms/batch", 1e3), n_img / mc))
        overlap = not (max(tc[n]) < min(tb[n]) or max(tb[n]) < min(tc[n]))
        print("     ratio of the medians (b)/(c): %.2fx, spreads %s" % (mb / mc, "overlap" if overlap else "do not overlap"))
    # (d) the two kernels alone on resident buffers
    dev = h.device()
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in batch]
    samplings = [data_utils.JPEG_SAMPLING[SUBSAMPLING]] * n_img
    layout = data_utils._jpeg_encode_layout(shapes, samplings)
    desc = layout["desc"]
    host = np.zeros(layout["total"], np.uint8)
    host[:desc.nbytes] = desc.view(np.uint8)
    tables = np.empty((2, 64), np.uint16)
    h.check(h.lib().ssd_jpeg_quality_tables(QUALITY, tables.ctypes.data), "ssd_jpeg_quality_tables")
    host[layout["tables_at"]:] = np.tile(tables.reshape(-1), n_img).view(np.uint8)
    packed = torch.as_tensor(host).to(dev)
    rgb = torch.cat([t.reshape(-1) for t in batch])
    coef = torch.empty(layout["coef_bytes"], dtype=torch.uint8, device=dev)
    ws = torch.empty(layout["plane_bytes"], dtype=torch.uint8, device=dev)
    base = packed.data_ptr()

    def launch():
        h.check(h.lib().ssd_jpeg_forward(h.ptr(rgb), rgb.numel(), base, layout["total"], desc.ctypes.data, base, n_img, h.ptr(coef),
                                         coef.numel(), h.ptr(ws), ws.numel(), h.stream()), "ssd_jpeg_forward")
    for _ in range(10):
        launch()
    K = 200
    td = [events(launch, K) for _ in range(rounds)]
    moved = pixels * 3 + 2 * layout["plane_bytes"] + layout["coef_bytes"]
    print("(d)  ssd_jpeg_forward alone (2 kernels, %d blocks; device events, %d back-to-back calls): %s" % (
        layout["coef_bytes"] // 128, K, spread(td, "us/call", 1e6)))
    print("     bytes it must move: %.1f MB (pixels read, planes written and read, %.1f MB of coefficients written) -> %.2f TB/s"
          % (moved / 1e6, layout["coef_bytes"] / 1e6, moved / statistics.median(td) / 1e12))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
