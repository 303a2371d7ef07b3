"""Diagnostics script (not a test): what decoding baseline JPEGs on the GPU behind the host entropy decoder
(``ssd_jpeg_entropy_decode`` + ``ssd_jpeg_decode``) buys for the input path.

B=32 VOC-sized JPEG files (4:2:0, quality 92, H and W in 300..500, written to a temporary directory with Pillow) to
300x300 float32, the paths alternating inside this process, every timed window >= 1 s and closed by a device synchronise:
  (a) today's path: a pool of N threads runs ``PIL.Image.open(path).convert("RGB")``, then ``preprocess_ragged_batch``;
  (b) the new path at the same N: the pool reads the file, parses it and entropy-decodes it (``jpeg_host_decode``), then
      ``preprocess_jpeg_batch`` (one upload of coefficients, ``ssd_jpeg_decode``, ``ssd_preprocess_ragged``);
      both for N = 1, 8 and 16;
  (c) ``ssd_jpeg_decode`` alone (its two kernels), device events around K back-to-back calls on a resident packed buffer;
  (d) a device-to-device copy that moves the same number of bytes (coefficients read, component planes written and read,
      pixels written), the bandwidth yardstick for (c).
Every figure is the median of --rounds windows with their spread (min .. max).  The outputs of (a) and (b) are compared
bit for bit first.  Usage: python tests/bench_jpeg.py [--rounds 5]"""
import argparse
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
import voc_cases as vc

B, S = 32, 300
WORKERS = (1, 8, 16)


def spread(xs, unit, scale=1.0):
    xs = [x * scale for x in xs]
    return "%.3f %s (median; min %.3f .. max %.3f, n=%d)" % (statistics.median(xs), unit, min(xs), max(xs), len(xs))


def window(fn, min_seconds=1.0):
    """Seconds per call over a window of at least ``min_seconds`` that ends in a device synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def events(fn, K):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / K


def write_files(root):
    from PIL import Image
    rng = np.random.default_rng(0)
    paths = []
    for i in range(B):
        hh, ww = int(rng.integers(300, 501)), int(rng.integers(300, 501))
        p = os.path.join(root, "%03d.jpg" % i)
        Image.fromarray(vc.pixels(hh, ww, "RGB", seed=i)).save(p, quality=92, subsampling="4:2:0")
        paths.append(p)
    return paths


def load_pillow(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def load_coefficients(path):
    with open(path, "rb") as f:
        return data_utils.jpeg_host_decode(f.read())


def main(rounds):
    assert torch.cuda.is_available(), "bench_jpeg.py measures on the GPU"
    with tempfile.TemporaryDirectory() as root:
        paths = write_files(root)
        file_bytes = sum(os.path.getsize(p) for p in paths)
        pools = {n: ThreadPoolExecutor(max_workers=n) for n in WORKERS}
        old = lambda n: data_utils.preprocess_ragged_batch(list(pools[n].map(load_pillow, paths)), S, S)      # noqa: E731
        new = lambda n: data_utils.preprocess_jpeg_batch(list(pools[n].map(load_coefficients, paths)), S, S)  # noqa: E731
        a, b = old(8), new(8)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the GPU decode differs from Pillow's"
        items = [load_coefficients(p) for p in paths]
        assert all(isinstance(x, data_utils.JpegCoefficients) for x in items)
        host_pillow = window(lambda: [load_pillow(p) for p in paths]) / B
        host_entropy = window(lambda: [load_coefficients(p) for p in paths]) / B
        for n in WORKERS:
            old(n); new(n)
        ta, tb = {n: [] for n in WORKERS}, {n: [] for n in WORKERS}
        for _ in range(rounds):
            for n in WORKERS:
                ta[n].append(window(lambda: old(n)))
                tb[n].append(window(lambda: new(n)))
        pixels = sum(int(x.info.width) * int(x.info.height) for x in items)
        print("B=%d VOC-sized JPEGs (4:2:0, quality 92; %.2f MB of files, %.1f MB of pixels) -> %dx%d float32; outputs bitwise equal"
              % (B, file_bytes / 1e6, pixels * 3 / 1e6, S, S))
        print("     one thread, per image: Pillow open + convert %.3f ms, read + parse + entropy decode %.3f ms" % (
            host_pillow * 1e3, host_entropy * 1e3))
        for n in WORKERS:
            ma, mb = statistics.median(ta[n]), statistics.median(tb[n])
            print("(a)  %2d workers, Pillow decode + preprocess_ragged_batch           : %s = %.0f images/s" % (
                n, spread(ta[n], "ms/batch", 1e3), B / ma))
            print("(b)  %2d workers, host entropy decode + preprocess_jpeg_batch       : %s = %.0f images/s" % (
                n, spread(tb[n], "ms/batch", 1e3), B / mb))
            overlap = not (max(tb[n]) < min(ta[n]) or max(ta[n]) < min(tb[n]))
            print("     ratio of the medians (a)/(b): %.2fx, spreads %s" % (ma / mb, "overlap" if overlap else "do not overlap"))
        # (c) the two kernels alone on a resident packed buffer
        layout = data_utils._jpeg_layout(items)
        host = np.zeros(layout["total"], np.uint8)
        data_utils._jpeg_fill(host, items, layout, [])
        dev = h.device()
        packed = torch.as_tensor(host).to(dev)
        rgb = torch.empty(layout["rgb_bytes"], dtype=torch.uint8, device=dev)
        ws = torch.empty(layout["plane_bytes"], dtype=torch.uint8, device=dev)
        base, desc, out_desc = packed.data_ptr(), layout["desc"], layout["out_desc"]

        def launch():
            h.check(h.lib().ssd_jpeg_decode(base, layout["total"], desc.ctypes.data, base, B, h.ptr(rgb), rgb.numel(),
                                            out_desc.ctypes.data, base + layout["out_at"], h.ptr(ws), ws.numel(), h.stream()),
                    "ssd_jpeg_decode")
        for _ in range(10):
            launch()
        want = load_pillow(paths[0])
        got = rgb[:want.size].view(want.shape).cpu().numpy()
        assert np.array_equal(got, want)
        coef_bytes = sum(int(x.info.coef_bytes) for x in items)
        moved = coef_bytes + 2 * (coef_bytes // 2) + pixels * 3
        n = moved // 2
        c_src, c_dst = torch.zeros(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        copy = lambda: c_dst.copy_(c_src)                                                                      # noqa: E731
        for _ in range(10):
            copy()
        K = 200
        tc, td = [], []
        for _ in range(rounds):
            tc.append(events(launch, K))
            td.append(events(copy, K))
        mc, md = statistics.median(tc), statistics.median(td)
        print("(c)  ssd_jpeg_decode alone (2 kernels, %d blocks; device events, %d back-to-back calls): %s" % (
            coef_bytes // 128, K, spread(tc, "us/call", 1e6)))
        print("     bytes it must move: %.1f MB -> %.2f TB/s" % (moved / 1e6, moved / mc / 1e12))
        print("(d)  device copy of %.1f MB (the same %.1f MB of reads + writes): %s -> %.2f TB/s" % (
            n / 1e6, moved / 1e6, spread(td, "us/call", 1e6), moved / md / 1e12))
        print("     (c)/(d) = %.2f" % (mc / md))
        for p in pools.values():
            p.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
