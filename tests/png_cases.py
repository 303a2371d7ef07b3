"""The cases of the PNG encoder's tests (CPU and GPU) and a NumPy restatement of rule 1 of its stream format only: the
filtered stream ``F`` (include/ssd_hip.h, "PNG ENCODER").  Everything behind ``F`` -- tokens, codes, framing -- is checked
by decoders (zlib, Pillow), not restated.  Every case is a few bytes to about 270 KB."""
import ctypes
import io
import struct
import zlib

import numpy as np

SEGMENT = 16384
FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _smooth(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 90 * np.sin(yy / 23.0 + c) * np.cos(xx / 31.0 + 0.5 * c) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 2, (h, w, 3)), 0, 255).astype(np.uint8)


def _noise(h, w, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _flat(h, w, colour):
    return np.broadcast_to(np.asarray(colour, np.uint8), (h, w, 3)).copy()


def _row(pixels):
    return np.asarray(pixels, np.uint8).reshape(1, -1, 3)


def fibonacci_image():
    """Byte values with Fibonacci frequencies over 20 symbols (17 710 bytes, plain Huffman depth 19), shuffled by a fixed
    permutation -- sorted index i goes to i * 8171 mod 17 710, which spreads every symbol evenly and makes no long runs --
    so that the tokens of the FIRST segment alone (16 384 bytes of the one row) still need a 17-bit plain Huffman code:
    the literal / length code has to be length-limited inside one segment.  One row, mode 0."""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(n, 3 + 7 * i, np.uint8) for i, n in enumerate(fib)])
    data = data[(np.arange(len(data), dtype=np.int64) * 8171) % len(data)]
    data = data[:len(data) // 3 * 3]
    return data.reshape(1, -1, 3)


def cases():
    """[(name, rgb uint8 [H,W,3], filter 0..5)]"""
    out = []
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 2), (3, 1), (2, 3)):
        out.append(("shape_%dx%d" % (h, w), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 5))
    for w in (5461, 5460, 5462):                                                    # H = 2: a cut at, before and behind a row's end
        out.append(("cut_w%d_noise" % w, _noise(2, w, seed=w), 0))
        out.append(("cut_w%d_smooth" % w, _smooth(2, w, seed=w), 5))
        out.append(("cut_w%d_zero" % w, _flat(2, w, (0, 0, 0)), 0))
        out.append(("cut_w%d_colour" % w, _flat(2, w, (77, 77, 77)), 0))
    for first in ((1, 2, 50), (1, 50, 50), (50, 50, 50)):                            # runs: the literal tails and the 258 cap
        for n in (1, 2, 85, 86, 87, 88, 172, 173):
            out.append(("run_%d_%d_%d_n%d" % (first + (n,)), _row([first] + [(50, 50, 50)] * n), 0))
    out.append(("fibonacci", fibonacci_image(), 0))
    out.append(("stored_noise_64", _noise(64, 64), 5))
    smooth = _smooth(300, 300)
    for f in range(6):
        out.append(("smooth_300_%s" % FILTERS[f], smooth, f))
    out.append(("flat_300", _flat(300, 300, (31, 120, 200)), 5))
    return out


def small_cases():
    """The cases whose decode is cheap enough to repeat per test: everything but the 300 x 300 images in modes 0..4."""
    return [c for c in cases() if not (c[0].startswith("smooth_300_") and c[2] != 5)]


def paeth(a, b, c):
    a, b, c = (v.astype(np.int32) for v in (a, b, c))
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_stream(rgb, mode):
    """Rule 1: ``H`` rows of ``1 + 3W`` bytes."""
    H, W, _ = rgb.shape
    rows = rgb.reshape(H, 3 * W).astype(np.int32)
    out = np.empty((H, 1 + 3 * W), np.uint8)
    zero = np.zeros(3 * W, np.int32)
    for y in range(H):
        x = rows[y]
        b = rows[y - 1] if y else zero
        a = np.concatenate([zero[:3], x[:-3]]) if W > 1 else zero
        c = np.concatenate([zero[:3], b[:-3]]) if W > 1 else zero
        cand = [x, x - a, x - b, x - ((a + b) >> 1), x - paeth(a, b, c)]
        cand = [(v & 255) for v in cand]
        if mode == 5:
            sums = [int(np.minimum(v, 256 - v).sum()) for v in cand]
            t = sums.index(min(sums))
        else:
            t = mode
        out[y, 0] = t
        out[y, 1:] = cand[t]
    return out.tobytes()


def segments(H, W):
    return -(-(H * (1 + 3 * W)) // SEGMENT)


def bound(H, W):
    return 45 + 17 * segments(H, W) + H * (1 + 3 * W) + 6


def walk_chunks(blob):
    """[(type, data)] of a PNG file; asserts the signature, every CRC, and that nothing follows IEND."""
    assert blob[:8] == SIGNATURE
    at, chunks = 8, []
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert len(data) == n
        (crc,) = struct.unpack(">I", blob[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data), "CRC of %s at %d" % (kind, at)
        chunks.append((kind, data))
        at += 12 + n
    assert at == len(blob) and chunks[-1] == (b"IEND", b"")
    return chunks


def check_file(blob, rgb, mode):
    """Everything the issue asks of one file: Pillow's pixels, the chunk list, strict zlib == the restated F, the bound."""
    from PIL import Image
    H, W, _ = rgb.shape
    im = Image.open(io.BytesIO(blob))
    assert im.mode == "RGB" and im.size == (W, H)
    assert np.array_equal(np.asarray(im), rgb)
    chunks = walk_chunks(blob)
    assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * segments(H, W) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    idat = b"".join(d for k, d in chunks if k == b"IDAT")
    assert idat[:2] == b"\x78\x9c"
    assert zlib.decompress(idat) == filtered_stream(rgb, mode)                      # strict: the Adler-32 is checked
    assert len(blob) <= bound(H, W)


def host_encode(rgb, mode, out_bytes=None, guard=64, fill=0xA5):
    """``ssd_png_encode_host`` into a buffer with guard bytes: (rc, bytes written as ``bytes``, written, guards intact, the
    buffer untouched)."""
    import ssd_hip
    rgb = np.ascontiguousarray(rgb)
    H, W, _ = rgb.shape
    if out_bytes is None:
        out_bytes = int(ssd_hip.lib().ssd_png_encode_bound(H, W))
    store = np.full(out_bytes + 2 * guard, fill, np.uint8)
    written = ctypes.c_size_t(77)
    rc = ssd_hip.lib().ssd_png_encode_host(rgb.ctypes.data, H, W, int(mode), store.ctypes.data + guard, out_bytes, ctypes.byref(written))
    intact = bool((store[:guard] == fill).all() and (store[guard + out_bytes:] == fill).all())
    body = store[guard:guard + out_bytes]
    return rc, body[:written.value].tobytes(), int(written.value), intact, bool((body == fill).all())
