"""Diagnostics script (not a test): what entropy-coding JPEG output on the GPU (``ssd_jpeg_pack``) buys for the output
path, on the workload of tests/bench_jpeg_encode.py: 64 device-resident uint8 images (32 drawn 300x300 + 32 VOC-sized)
to ``bytes`` in host memory, quality 75, 4:2:0.  The legs alternate inside this process, every timed window >= 1 s and
closed by a device synchronise:
  (c) the default path: ``ssd_jpeg_forward``, one download of the int16 coefficients into pinned memory, a pool of N
      threads runs ``ssd_jpeg_entropy_encode``; N = 1, 8 and 16;
  (e) the new route (``SSD_JPEG_ENTROPY_GPU=1``): ``ssd_jpeg_forward`` + ``ssd_jpeg_pack``, a download of offsets + status
      and one of the streams themselves, sliced on the calling thread;
  (f) ``ssd_jpeg_pack`` alone (its six kernels and two fills), device events around K back-to-back calls on resident
      buffers.
Every figure is the median of --rounds windows with their spread (min .. max).  The outputs of (c) and (e) are compared
byte for byte first.  Usage: python tests/bench_jpeg_pack.py [--rounds 5]"""
import argparse
import os
import statistics
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + "/tf-ssd_amd",
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
import ssd_hip as h
from utils import data_utils
from bench_jpeg import events, spread, window
from bench_jpeg_encode import QUALITY, SUBSAMPLING, WORKERS, images


def encode(batch, entropy_gpu, workers=None):
    os.environ["SSD_JPEG_ENCODE_GPU"] = "1"
    os.environ["SSD_JPEG_ENTROPY_GPU"] = "1" if entropy_gpu else "0"
    return data_utils.encode_jpeg_batch(batch, quality=QUALITY, subsampling=SUBSAMPLING, workers=workers)


def main(rounds):
    assert torch.cuda.is_available(), "bench_jpeg_pack.py measures on the GPU"
    batch = images()
    n_img = len(batch)
    host_road, gpu_road = encode(batch, False, 8), encode(batch, True)
    assert host_road == gpu_road, "the device entropy coder's bytes differ from the host coder's"
    for n in WORKERS:
        encode(batch, False, n)
    encode(batch, True)
    tc, te = {n: [] for n in WORKERS}, []
    for _ in range(rounds):
        for n in WORKERS:
            tc[n].append(window(lambda: encode(batch, False, n)))
        te.append(window(lambda: encode(batch, True)))
    # the buffers of one call, resident, for (f) and for the download sizes
    dev = h.device()
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in batch]
    samplings = [data_utils.JPEG_SAMPLING[SUBSAMPLING]] * n_img
    tables = np.empty((2, 64), np.uint16)
    h.check(h.lib().ssd_jpeg_quality_tables(QUALITY, tables.ctypes.data), "ssd_jpeg_quality_tables")
    tables = np.tile(tables, (n_img, 1, 1))
    coef, desc = data_utils.jpeg_forward_batch(torch.cat([t.reshape(-1) for t in batch]), shapes, samplings, tables)
    layout = data_utils._jpeg_pack_layout(desc, shapes, samplings, tables)
    pd = layout["desc"]
    host = np.zeros(layout["total"], np.uint8)
    data_utils._jpeg_pack_fill(host, layout)
    packed = torch.as_tensor(host).to(dev)
    out = torch.empty(layout["out_bytes"], dtype=torch.uint8, device=dev)
    meta = torch.empty(2 * n_img + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(h.lib().ssd_jpeg_pack_workspace_bytes(pd.ctypes.data, n_img)), dtype=torch.uint8, device=dev)
    base = packed.data_ptr()

    def launch():
        h.check(h.lib().ssd_jpeg_pack(h.ptr(coef), coef.numel(), base, layout["total"], pd.ctypes.data, base, n_img, h.ptr(out),
                                      out.numel(), meta.data_ptr(), meta.data_ptr() + 4 * (n_img + 1), h.ptr(ws), ws.numel(),
                                      h.stream()), "ssd_jpeg_pack")
    for _ in range(10):
        launch()
    K = 100
    tf = [events(launch, K) for _ in range(rounds)]
    torch.cuda.synchronize()
    m = meta.cpu().numpy()
    assert not m[n_img + 1:].any() and int(m[n_img]) == sum(map(len, gpu_road))
    blocks = sum(-(-w // (8 * hs)) * -(-hh // (8 * vs)) * (hs * vs + 2) for (hh, w), (hs, vs) in zip(shapes, samplings))
    print("%d device images (%d blocks) -> bytes on the host; JPEG quality %d %s: %.2f MB of streams, bytes equal on both roads"
          % (n_img, blocks, QUALITY, SUBSAMPLING, sum(map(len, gpu_road)) / 1e6))
    print("downloaded per batch: (c) %.2f MB of int16 coefficients; (e) %.2f MB = %d bytes of offsets + status and the streams"
          % (coef.numel() / 1e6, (meta.numel() * 4 + int(m[n_img])) / 1e6, meta.numel() * 4))
    me = statistics.median(te)
    for n in WORKERS:
        mc = statistics.median(tc[n])
        print("(c)  %2d workers, ssd_jpeg_forward + download + entropy-encode pool : %s = %.0f images/s" % (
            n, spread(tc[n], "ms/batch", 1e3), n_img / mc))
        overlap = not (max(te) < min(tc[n]) or max(tc[n]) < min(te))
        print("     ratio of the medians (c)/(e): %.2fx, spreads %s" % (mc / me, "overlap" if overlap else "do not overlap"))
    print("(e)  no pool,    ssd_jpeg_forward + ssd_jpeg_pack + two downloads      : %s = %.0f images/s" % (
        spread(te, "ms/batch", 1e3), n_img / me))
    print("(f)  ssd_jpeg_pack alone (6 kernels + 2 fills; %.1f MB of workspace zeroed; device events, %d back-to-back calls): %s"
          % (ws.numel() / 1e6, K, spread(tf, "us/call", 1e6)))
    print("     (f) as a share of (e): %.1f %%" % (100.0 * statistics.median(tf) / me))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    main(ap.parse_args().rounds)
