"""Diagnostics script (not a test): what Huffman-decoding baseline JPEGs on the GPU (``ssd_jpeg_unpack``,
``SSD_JPEG_ENTROPY_DECODE_GPU=1``) buys for the input path, against today's default measured in the same run.

The files of tests/bench_jpeg.py: B=32 VOC-sized JPEGs (4:2:0, quality 92, H and W in 300..500) to 300x300 float32, the
legs alternating inside this process, every timed window >= 1 s and closed by a device synchronise:
  (b) today's default at N threads: the pool reads, parses and entropy-decodes each file (``jpeg_host_decode``), then
      ``preprocess_jpeg_batch`` (one upload of coefficients, ``ssd_jpeg_decode``, ``ssd_preprocess_ragged``);
  (g) the new road at the same N: the pool reads, parses and PLANS each file (``jpeg_host_plan``), then
      ``preprocess_jpeg_batch`` (one upload of scan bytes and plans, ``ssd_jpeg_unpack``, ``ssd_jpeg_decode``, the status
      read, ``ssd_preprocess_ragged``); both for N = 1, 8 and 16;
  (h) ``ssd_jpeg_unpack`` alone, device events around K back-to-back calls on a resident upload, at subseq_bits 512, 1024
      and 2048, with the sweeps its synchronise phase took.
Every figure is the median of --rounds windows with their spread (min .. max).  The outputs of (b) and (g) are compared
bit for bit first.  Usage: python tests/bench_jpeg_unpack.py [--rounds 5]"""
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
from bench_jpeg import B, S, WORKERS, events, spread, window, write_files


def load_coefficients(path):
    with open(path, "rb") as f:
        return data_utils.jpeg_host_decode(f.read())


def load_plan(path):
    with open(path, "rb") as f:
        return data_utils.jpeg_host_plan(f.read())


def main(rounds):
    assert torch.cuda.is_available(), "bench_jpeg_unpack.py measures on the GPU"
    os.environ.pop("SSD_JPEG_ENTROPY_DECODE_GPU", None)                            # the items decide the road here
    with tempfile.TemporaryDirectory() as root:
        paths = write_files(root)
        file_bytes = sum(os.path.getsize(p) for p in paths)
        pools = {n: ThreadPoolExecutor(max_workers=n) for n in WORKERS}
        old = lambda n: data_utils.preprocess_jpeg_batch(list(pools[n].map(load_coefficients, paths)), S, S)   # noqa: E731
        new = lambda n: data_utils.preprocess_jpeg_batch(list(pools[n].map(load_plan, paths)), S, S)           # noqa: E731
        a, b = old(8), new(8)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the device entropy decoder's road differs from the default"
        scans = [load_plan(p) for p in paths]
        assert all(isinstance(x, data_utils.JpegScan) for x in scans)
        coded = [load_coefficients(p) for p in paths]
        up_old, up_new = data_utils._jpeg_layout(coded)["upload"], data_utils._jpeg_layout(scans)["upload"]
        host_entropy = window(lambda: [load_coefficients(p) for p in paths]) / B
        host_plan = window(lambda: [load_plan(p) for p in paths]) / B
        for n in WORKERS:
            old(n); new(n)
        tb, tg = {n: [] for n in WORKERS}, {n: [] for n in WORKERS}
        for _ in range(rounds):
            for n in WORKERS:
                tb[n].append(window(lambda: old(n)))
                tg[n].append(window(lambda: new(n)))
        print("B=%d VOC-sized JPEGs (4:2:0, quality 92; %.2f MB of files) -> %dx%d float32; outputs bitwise equal" % (
            B, file_bytes / 1e6, S, S))
        print("     bytes uploaded per batch: (b) %.2f MB, (g) %.2f MB" % (up_old / 1e6, up_new / 1e6))
        print("     one thread, per image: read + parse + entropy decode %.3f ms, read + parse + plan %.3f ms" % (
            host_entropy * 1e3, host_plan * 1e3))
        for n in WORKERS:
            mb, mg = statistics.median(tb[n]), statistics.median(tg[n])
            print("(b)  %2d workers, host entropy decode + preprocess_jpeg_batch : %s = %.0f images/s" % (
                n, spread(tb[n], "ms/batch", 1e3), B / mb))
            print("(g)  %2d workers, scan plan + ssd_jpeg_unpack + the same       : %s = %.0f images/s" % (
                n, spread(tg[n], "ms/batch", 1e3), B / mg))
            overlap = not (max(tg[n]) < min(tb[n]) or max(tb[n]) < min(tg[n]))
            print("     ratio of the medians (b)/(g): %.2fx, spreads %s" % (mb / mg, "overlap" if overlap else "do not overlap"))
        # (h) the call alone on a resident upload
        dev = h.device()
        want = [torch.as_tensor(x.coef) for x in coded]
        for bits in (512, 1024, 2048):
            layout = data_utils._jpeg_unpack_layout(scans, bits)
            host = np.zeros(layout["total"], np.uint8)
            data_utils._jpeg_unpack_fill(host, scans, layout)
            packed = torch.as_tensor(host).to(dev)
            coef = torch.empty(layout["coef_bytes"], dtype=torch.uint8, device=dev)
            desc = layout["desc"]
            ws = torch.empty(int(h.lib().ssd_jpeg_unpack_workspace_bytes(desc.ctypes.data, B, bits)), dtype=torch.uint8, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            base = packed.data_ptr()

            def launch():
                h.check(h.lib().ssd_jpeg_unpack(base, layout["total"], desc.ctypes.data, base + layout["desc_at"], B, bits, h.ptr(coef),
                                                coef.numel(), status.data_ptr(), h.ptr(ws), ws.numel(), h.stream()), "ssd_jpeg_unpack")
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any()
            got = coef.cpu()
            for d, w in zip(desc, want):
                at = int(d["coef_offset"])
                assert torch.equal(got[at:at + w.numel() * 2].view(torch.int16), w)
            sweeps = ws[:4 * B].view(torch.int32).cpu().numpy()
            K = 50
            th = [events(launch, K) for _ in range(rounds)]
            subs = int(desc["sub_start"][-1]) + h.lib().ssd_jpeg_unpack_slots(int(desc["scan_bytes"][-1]), 1, bits)
            print("(h)  ssd_jpeg_unpack alone, subseq_bits %4d (%d slots; device events, %d back-to-back calls): %s; sweeps median %d, max %d"
                  % (bits, subs, K, spread(th, "ms/call", 1e3), int(np.median(sweeps)), int(sweeps.max())))
        for p in pools.values():
            p.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
