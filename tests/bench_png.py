"""Diagnostics script (not a test): what encoding PNG output on the GPU (``ssd_png_encode``) buys for the output path.
64 images of 300x300 from ``draw_detections_batch``, device-resident uint8, to ``bytes`` in host memory -- once drawn on
smooth synthetic images and once on noise (the input of tests/bench_jpeg_encode.py).  The legs alternate inside this
process, every timed window >= 1 s and closed by a device synchronise:
  (a) the default path: download + ``PIL.Image.save(..., "PNG")`` image by image on the calling thread;
  (b) the same on the ``data_workers`` pool at 1 / 8 / 16 threads;
  (c) ``data_utils.encode_png_batch``: descriptors up, four launches, offsets and files down, sliced on the calling thread;
  (d) the ``ssd_png_encode`` launches alone, device events around K back-to-back calls on resident buffers.
Every figure is the median of --rounds windows with their spread (min .. max).  Beside the times: the total file sizes of
(c) against Pillow's and against zlib ``Z_RLE`` on the same filtered bytes (one IDAT, the same 57 bytes of framing), and
Pillow's decode of every (c) file is compared with the pixels first.  Usage: python tests/bench_png.py [--rounds 5] [--out FILE]"""
import argparse
import io
import os
import statistics
import sys
import zlib

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
from utils import data_utils, drawing_utils
import drawing_cases as dc
import png_cases as pc
from bench_jpeg import events, spread, window

B = 64
WORKERS = (1, 8, 16)


def drawn(kind):
    imgs, boxes, labels, scores = dc.ragged_batch(B=B)
    if kind == "smooth":
        imgs = np.stack([pc._smooth(300, 300, seed=b).astype(np.float32) / np.float32(255) for b in range(B)])
    return drawing_utils.draw_detections_batch(h.to_dev(imgs), boxes, labels, scores, dc.LABELS, colors=dc.colors(9))


def pillow_serial(batch):
    host = batch.cpu().numpy()
    return [data_utils._pillow_png(a) for a in host]


def pillow_pool(batch, workers):
    host = batch.cpu().numpy()
    return list(data_utils._encode_pool(workers).map(data_utils._pillow_png, list(host)))


def main(rounds, out_path):
    assert torch.cuda.is_available(), "bench_png.py measures on the GPU"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    lib = h.lib()
    dev = h.device()
    for kind in ("smooth", "noise"):
        batch = drawn(kind)
        host = batch.cpu().numpy()
        gpu_files, pil_files = data_utils.encode_png_batch(batch), pillow_serial(batch)
        from PIL import Image
        for blob, a in zip(gpu_files, host):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob))), a), "a device file does not decode to its pixels"
        rle = 0
        for a in host:
            co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
            rle += 57 + len(co.compress(pc.filtered_stream(a, 5)) + co.flush())
        for n in WORKERS:
            pillow_pool(batch, n)
        ta, tb, tc = [], {n: [] for n in WORKERS}, []
        for _ in range(rounds):
            ta.append(window(lambda: pillow_serial(batch)))
            for n in WORKERS:
                tb[n].append(window(lambda: pillow_pool(batch, n)))
            tc.append(window(lambda: data_utils.encode_png_batch(batch)))
        shapes = [(300, 300)] * B
        layout = data_utils._png_layout(shapes, [5] * B)
        desc = layout["desc"]
        dd = torch.as_tensor(desc.view(np.uint8)).to(dev)
        rgb = batch.reshape(-1)
        out = torch.empty(layout["out_bytes"], dtype=torch.uint8, device=dev)
        offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.ssd_png_encode_workspace_bytes(desc.ctypes.data, B)), dtype=torch.uint8, device=dev)

        def launch():
            h.check(lib.ssd_png_encode(h.ptr(rgb), rgb.numel(), desc.ctypes.data, h.ptr(dd), B, h.ptr(out), out.numel(), h.ptr(offsets),
                                       h.ptr(ws), ws.numel(), h.stream()), "ssd_png_encode")
        for _ in range(10):
            launch()
        K = 100
        td = [events(launch, K) for _ in range(rounds)]
        torch.cuda.synchronize()
        assert int(offsets[B]) == sum(map(len, gpu_files))
        mc = statistics.median(tc)
        say("[%s] %d drawn 300x300 device images (%d segments, %.2f MB raw) -> PNG bytes on the host" % (
            kind, B, layout["segments"], rgb.numel() / 1e6))
        say("  sizes: (c) %.3f MB; Pillow %.3f MB ((c)/Pillow %.3f); zlib Z_RLE on the same filtered bytes %.3f MB ((c)/Z_RLE %.3f)" % (
            sum(map(len, gpu_files)) / 1e6, sum(map(len, pil_files)) / 1e6, sum(map(len, gpu_files)) / sum(map(len, pil_files)),
            rle / 1e6, sum(map(len, gpu_files)) / rle))
        say("  (a)  calling thread, download + PIL save            : %s = %.0f images/s" % (spread(ta, "ms/batch", 1e3), B / statistics.median(ta)))
        for n in WORKERS:
            mb = statistics.median(tb[n])
            overlap = not (max(tc) < min(tb[n]) or max(tb[n]) < min(tc))
            say("  (b)  %2d workers, download + PIL save on the pool    : %s = %.0f images/s; (b)/(c) %.2fx, spreads %s" % (
                n, spread(tb[n], "ms/batch", 1e3), B / mb, mb / mc, "overlap" if overlap else "do not overlap"))
        say("  (c)  encode_png_batch                               : %s = %.0f images/s; (a)/(c) %.2fx" % (
            spread(tc, "ms/batch", 1e3), B / mc, statistics.median(ta) / mc))
        say("  (d)  ssd_png_encode alone (4 launches; device events, %d back-to-back calls): %s; %.1f %% of (c)" % (
            K, spread(td, "us/call", 1e6), 100.0 * statistics.median(td) / mc))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.rounds, a.out)
