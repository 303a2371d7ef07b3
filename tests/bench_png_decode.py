"""Diagnostics script (not a test): what decoding PNG input on the GPU behind a host inflate (``ssd_png_decode``) buys for
the custom-image path.  64 VOC-sized (500x375) RGB PNG files written by Pillow into a temporary folder -- one smooth set,
one noise set -- to the resized 300x300 float32 batch on the device.  The legs alternate inside this process, every timed
window >= 1 s and closed by a device synchronise:
  (a) today's default: ``PIL.Image.open(...).convert("RGB")`` file by file on the calling thread + ``resize_lanczos_batch``;
  (b) the same decode on a thread pool of this script's own at 1 / 8 / 16 threads + the same resize (the fair competitor;
      not product code);
  (c) the new road at 1 / 8 / 16 workers: read + ``ssd_png_parse`` + inflate on the pool, one upload of the filtered
      scanlines, ``ssd_png_decode``, ``ssd_resize_lanczos`` on the device-resident pixels;
  (d) the ``ssd_png_decode`` launches alone, device events around K back-to-back calls on resident buffers.
Every figure is the median of --rounds windows with their spread (min .. max).  Beside the times: the host half per image
on one thread (read, parse + CRC, IDAT join + inflate + filter-byte check) and the bytes uploaded per batch.  (c)'s output is compared with
(a)'s first.  Usage: python tests/bench_png_decode.py [--rounds 5] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
from utils import data_utils
import png_cases as pc
from bench_jpeg import events, spread, window

B = 64
WORKERS = (1, 8, 16)
SIZE = (300, 300)


def write_files(root, kind):
    from PIL import Image
    paths = []
    for b in range(B):
        px = pc._smooth(375, 500, seed=b) if kind == "smooth" else pc._noise(375, 500, seed=b)
        paths.append(os.path.join(root, "%s_%02d.png" % (kind, b)))
        Image.fromarray(px).save(paths[-1], "PNG")
    return paths


def pillow_road(paths, pool=None):
    decode = data_utils._decode_custom_image
    images = list(pool.map(decode, paths)) if pool is not None else [decode(p) for p in paths]
    return data_utils.resize_lanczos_batch(images, *SIZE)


def device_road(paths, pool):
    return data_utils.resize_lanczos_image_batch(list(pool.map(data_utils._custom_image_item, paths)), *SIZE)


def host_split(paths, repeats=3):
    """Seconds per image on one thread: read, parse + CRC, IDAT join + inflate + filter-byte check."""
    lib = h.lib()
    best = [float("inf")] * 3
    for _ in range(repeats):
        t0 = time.perf_counter()
        blobs = []
        for p in paths:
            with open(p, "rb") as f:
                blobs.append(f.read())
        t1 = time.perf_counter()
        infos = []
        for blob in blobs:
            info = h.PngInfo()
            assert lib.ssd_png_parse(blob, len(blob), ctypes.byref(info)) == 0
            infos.append(info)
        t2 = time.perf_counter()
        for blob, info in zip(blobs, infos):
            assert data_utils._png_inflate(blob, info) is not None
        t3 = time.perf_counter()
        best = [min(b, t / len(paths)) for b, t in zip(best, (t1 - t0, t2 - t1, t3 - t2))]
    return best, sum(map(len, blobs))


def main(rounds, out_path):
    assert torch.cuda.is_available(), "bench_png_decode.py measures on the GPU"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    lib = h.lib()
    dev = h.device()
    pools = {n: ThreadPoolExecutor(max_workers=n) for n in WORKERS}
    with tempfile.TemporaryDirectory() as root:
        for kind in ("smooth", "noise"):
            paths = write_files(root, kind)
            want = pillow_road(paths)
            for n in WORKERS:
                assert torch.equal(device_road(paths, pools[n]), want), "the device road's batch differs from the default road's"
                pillow_road(paths, pools[n])
            ta, tb, tc = [], {n: [] for n in WORKERS}, {n: [] for n in WORKERS}
            for _ in range(rounds):
                ta.append(window(lambda: pillow_road(paths)))
                for n in WORKERS:
                    tb[n].append(window(lambda: pillow_road(paths, pools[n])))
                    tc[n].append(window(lambda: device_road(paths, pools[n])))
            (t_read, t_parse, t_inflate), file_bytes = host_split(paths)
            items = [data_utils._custom_image_item(p) for p in paths]
            assert all(isinstance(x, data_utils.PngScanlines) for x in items), "a file took the fallback"
            layout = data_utils._png_decode_layout(items)
            host = np.zeros(layout["total"], np.uint8)
            data_utils._png_decode_fill(host, items, layout)
            packed = torch.from_numpy(host).to(dev)
            rgb = torch.empty(layout["rgb_bytes"], dtype=torch.uint8, device=dev)
            ws = torch.empty(layout["raw_bytes"], dtype=torch.uint8, device=dev)
            desc = layout["desc"]

            def launch():
                h.check(lib.ssd_png_decode(packed.data_ptr(), layout["total"], desc.ctypes.data, packed.data_ptr(), B, h.ptr(rgb), rgb.numel(),
                                           h.ptr(ws), ws.numel(), h.stream()), "ssd_png_decode")
            for _ in range(10):
                launch()
            K = 100
            td = [events(launch, K) for _ in range(rounds)]
            torch.cuda.synchronize()
            chains = int(desc["chains"].sum())
            say("[%s] %d PNG files of 500x375 RGB (%.2f MB of files) -> float32 [%d,%d,%d,3] on the device" % (
                kind, B, file_bytes / 1e6, B, SIZE[0], SIZE[1]))
            say("  host half per image, one thread: read %.3f ms, parse + CRC %.3f ms, inflate %.3f ms" % (
                1e3 * t_read, 1e3 * t_parse, 1e3 * t_inflate))
            say("  uploaded per batch: (c) %.2f MB of filtered scanlines (%d chains of rows), (a)/(b) %.2f MB of pixels" % (
                layout["total"] / 1e6, chains, B * 375 * 500 * 3 / 1e6))
            say("  (a)  calling thread, Pillow + resize_lanczos_batch      : %s = %.0f images/s" % (spread(ta, "ms/batch", 1e3), B / statistics.median(ta)))
            for n in WORKERS:
                mb, mc = statistics.median(tb[n]), statistics.median(tc[n])
                overlap = not (max(tc[n]) < min(tb[n]) or max(tb[n]) < min(tc[n]))
                say("  (b)  %2d threads, Pillow on a pool + the same resize     : %s = %.0f images/s" % (n, spread(tb[n], "ms/batch", 1e3), B / mb))
                say("  (c)  %2d workers, host inflate + ssd_png_decode + resize : %s = %.0f images/s; (b)/(c) %.2fx, spreads %s; (a)/(c) %.2fx" % (
                    n, spread(tc[n], "ms/batch", 1e3), B / mc, mb / mc, "overlap" if overlap else "do not overlap", statistics.median(ta) / mc))
            md = statistics.median(td)
            say("  (d)  ssd_png_decode alone (2 launches; device events, %d back-to-back calls): %s; %s %% of (c) at 1 / 8 / 16 workers" % (
                K, spread(td, "us/call", 1e6), " / ".join("%.1f" % (100.0 * md / statistics.median(tc[n])) for n in WORKERS)))
    for p in pools.values():
        p.shutdown()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.rounds, a.out)
