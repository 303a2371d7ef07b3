"""Diagnostics script (not a test): what inflating PNG input on the device (``ssd_png_inflate``, ``SSD_PNG_INFLATE_GPU=1``)
buys on top of ``SSD_PNG_DECODE_GPU=1``.  The same two sets as ``bench_png_decode.py`` -- 64 Pillow-written 500x375 RGB
files, smooth and noise -- to the resized 300x300 float32 batch on the device; the legs alternate inside this process, every
timed window >= 1 s and closed by a device synchronise:
  (c) the present road at 1 / 8 / 16 workers: read + parse + host inflate on the pool, the filtered scanlines uploaded,
      ``ssd_png_decode``, ``ssd_resize_lanczos`` (measured again here: the baseline of this run);
  (e) the new road at the same worker counts: read + parse on the pool, the IDAT payloads uploaded, ``ssd_png_inflate``,
      ``ssd_png_decode``, one read of the status words, the same resize;
  (f) ``ssd_png_inflate`` alone (2 launches), device events around K back-to-back calls on resident buffers: the batch of
      64, and ONE stream alone -- the per-wavefront rate the cap SSD_PNG_INFLATE_MAX_STREAM rests on.
Every figure is the median of --rounds windows with their spread (min .. max).  Beside the times: bytes uploaded per batch,
both ways.  (e)'s output is compared with (c)'s first.  Usage: python tests/bench_png_inflate.py [--rounds 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
from utils import data_utils
from bench_jpeg import events, spread, window
from bench_png_decode import B, SIZE, WORKERS, write_files


def road(paths, pool, inflate_on_device):
    os.environ["SSD_PNG_INFLATE_GPU"] = "1" if inflate_on_device else "0"
    return data_utils.resize_lanczos_image_batch(list(pool.map(data_utils._custom_image_item, paths)), *SIZE)


def resident(items):
    """The items' ``ssd_png_inflate`` call on device-resident buffers: ``(launch, layout)``."""
    lib, dev = h.lib(), h.device()
    layout = data_utils._png_stream_layout(items)
    host = np.zeros(layout["device_total"], np.uint8)
    data_utils._png_stream_fill(host, items, layout)
    packed = torch.from_numpy(host).to(dev)
    status = torch.zeros(len(items), dtype=torch.int32, device=dev)
    inflate = layout["inflate"]

    def launch():
        h.check(lib.ssd_png_inflate(packed.data_ptr(), packed.numel(), inflate.ctypes.data, packed.data_ptr() + layout["inflate_at"], len(items),
                                    h.ptr(status), h.stream()), "ssd_png_inflate")
    launch()
    torch.cuda.synchronize()
    assert not status.cpu().any(), "a stream was flagged"
    return launch, layout, (packed, status)


def main(rounds, out_path):
    assert torch.cuda.is_available(), "bench_png_inflate.py measures on the GPU"
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    os.environ["SSD_PNG_DECODE_GPU"] = "1"
    pools = {n: ThreadPoolExecutor(max_workers=n) for n in WORKERS}
    with tempfile.TemporaryDirectory() as root:
        for kind in ("smooth", "noise"):
            paths = write_files(root, kind)
            want = road(paths, pools[1], False)
            for n in WORKERS:
                assert torch.equal(road(paths, pools[n], True), want), "the device-inflate road's batch differs from the host-inflate road's"
            tc, te = {n: [] for n in WORKERS}, {n: [] for n in WORKERS}
            for _ in range(rounds):
                for n in WORKERS:
                    tc[n].append(window(lambda: road(paths, pools[n], False)))
                    te[n].append(window(lambda: road(paths, pools[n], True)))
            os.environ["SSD_PNG_INFLATE_GPU"] = "1"
            items = [data_utils._custom_image_item(p) for p in paths]
            assert all(isinstance(x, data_utils.PngStream) for x in items), "a file took the fallback"
            os.environ["SSD_PNG_INFLATE_GPU"] = "0"
            scanlines = data_utils._png_decode_layout([data_utils._custom_image_item(p) for p in paths])["total"]
            launch, layout, keep = resident(items)
            one, one_layout, keep_one = resident(items[:1])
            for _ in range(3):
                launch()
                one()
            tf = [events(launch, 10) for _ in range(rounds)]
            t1 = [events(one, 10) for _ in range(rounds)]
            torch.cuda.synchronize()
            zbytes = int(layout["inflate"]["zlib_bytes"].sum())
            out_bytes = sum(int(x.info.stream_bytes) for x in items)
            z1, o1 = int(one_layout["inflate"]["zlib_bytes"][0]), int(items[0].info.stream_bytes)
            say("[%s] %d PNG files of 500x375 RGB (%.2f MB of IDAT payload) -> float32 [%d,%d,%d,3] on the device" % (
                kind, B, zbytes / 1e6, B, SIZE[0], SIZE[1]))
            say("  uploaded per batch: (c) %.2f MB of filtered scanlines, (e) %.2f MB of zlib streams" % (scanlines / 1e6, layout["total"] / 1e6))
            for n in WORKERS:
                mc, me = statistics.median(tc[n]), statistics.median(te[n])
                overlap = not (max(te[n]) < min(tc[n]) or max(tc[n]) < min(te[n]))
                say("  (c)  %2d workers, host inflate + ssd_png_decode + resize           : %s = %.0f images/s" % (n, spread(tc[n], "ms/batch", 1e3), B / mc))
                say("  (e)  %2d workers, ssd_png_inflate + ssd_png_decode + resize        : %s = %.0f images/s; (c)/(e) %.2fx, spreads %s" % (
                    n, spread(te[n], "ms/batch", 1e3), B / me, mc / me, "overlap" if overlap else "do not overlap"))
            mf, m1 = statistics.median(tf), statistics.median(t1)
            say("  (f)  ssd_png_inflate alone, %d streams (device events, 10 back-to-back calls): %s = %.1f MB/s of output for the batch" % (
                B, spread(tf, "ms/call", 1e3), out_bytes / mf / 1e6))
            say("  (f)  ssd_png_inflate alone, ONE stream of %d -> %d bytes               : %s = %.1f MB/s of output, %.1f MB/s of input per wavefront" % (
                z1, o1, spread(t1, "ms/call", 1e3), o1 / m1 / 1e6, z1 / m1 / 1e6))
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
