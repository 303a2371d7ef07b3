"""The PNG encoder's host model (``ssd_png_encode_host``) and the packer of ``data_utils.png_pack_batch``, no GPU.  PNG is
lossless, so the oracle is a decoder, not another encoder's bytes: Pillow returns the input pixels, strict zlib returns the
filtered stream restated in tests/png_cases.py (and checks the Adler-32), and a chunk walk checks the framing and every
CRC.  The GPU test then holds the kernels to this model's bytes."""
import ctypes
import heapq
import itertools
import zlib

import numpy as np
import pytest

import png_cases as pc
import ssd_hip
from utils import data_utils

pytest.importorskip("PIL")

OK, INVALID, UNSUPPORTED = 0, -1, -3
CASES = pc.cases()


@pytest.fixture(scope="module")
def files():
    """name -> the host model's file, encoded once."""
    out = {}
    for name, rgb, mode in CASES:
        rc, blob, written, intact, _ = pc.host_encode(rgb, mode)
        assert rc == OK and intact and written == len(blob), name
        out[name] = blob
    return out


@pytest.mark.parametrize("name,rgb,mode", CASES, ids=[c[0] for c in CASES])
def test_every_decoder_returns_the_pixels_and_the_stream_is_strictly_valid(files, name, rgb, mode):
    pc.check_file(files[name], rgb, mode)
    assert pc.segments(*rgb.shape[:2]) == ssd_hip.lib().ssd_png_segments(rgb.shape[0], rgb.shape[1])
    assert pc.bound(*rgb.shape[:2]) == ssd_hip.lib().ssd_png_encode_bound(rgb.shape[0], rgb.shape[1])


def test_exactly_enough_room_is_taken_and_one_byte_less_is_refused_with_nothing_written(files):
    for name, rgb, mode in pc.small_cases():
        want = files[name]
        rc, blob, written, intact, _ = pc.host_encode(rgb, mode, out_bytes=len(want))
        assert rc == OK and intact and blob == want, name
        rc, blob, written, intact, untouched = pc.host_encode(rgb, mode, out_bytes=len(want) - 1)
        assert rc == INVALID and written == 0 and intact and untouched, name
        assert ssd_hip.lib().ssd_last_error().decode().startswith("ssd_png_encode_host")


def test_the_two_size_conditions(files):
    by_name = {c[0]: c for c in CASES}
    assert len(files["flat_300"]) < 2700                                            # under 1 % of the raw 270 000 bytes
    noise = by_name["stored_noise_64"][1]
    assert len(files["stored_noise_64"]) <= pc.bound(*noise.shape[:2])
    for w in (5460, 5461, 5462):                                                    # noise in mode 0: every block is stored
        name = "cut_w%d_noise" % w
        assert len(files[name]) == pc.bound(2, w)
        for kind, data in pc.walk_chunks(files[name])[1:-1]:
            body = data[2:] if data[:2] == b"\x78\x9c" else data
            assert body[0] in (0, 1) and int.from_bytes(body[1:3], "little") == 0xFFFF ^ int.from_bytes(body[3:5], "little")


def test_refusals_of_the_host_model():
    lib = ssd_hip.lib()
    rgb = np.zeros((2, 2, 3), np.uint8)
    out = np.zeros(256, np.uint8)
    written = ctypes.c_size_t(5)
    assert lib.ssd_png_encode_host(None, 2, 2, 5, out.ctypes.data, 256, ctypes.byref(written)) == INVALID
    assert lib.ssd_png_encode_host(rgb.ctypes.data, 2, 2, 5, None, 256, ctypes.byref(written)) == INVALID
    assert lib.ssd_png_encode_host(rgb.ctypes.data, 2, 2, 5, out.ctypes.data, 256, None) == INVALID
    for H, W, f in ((0, 2, 5), (2, 16385, 5), (2, 2, 6), (2, 2, -1)):
        assert lib.ssd_png_encode_host(rgb.ctypes.data, H, W, f, out.ctypes.data, 256, ctypes.byref(written)) == UNSUPPORTED
        assert written.value == 0 and not out.any()
    assert lib.ssd_png_segments(0, 5) == 0 and lib.ssd_png_encode_bound(16385, 1) == 0
    assert lib.ssd_png_segments(16384, 16384) == 49153 and lib.ssd_png_encode_bound(16384, 16384) == 45 + 17 * 49153 + 16384 * 49153 + 6
    assert lib.ssd_png_encode_workspace_bytes(None, 0) == 0


# ---- the Huffman builder, through the Fibonacci case --------------------------------------------------------------------------

_LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _token_histogram(segment):
    """Rule 3 restated for one segment: symbol -> count, the end-of-block symbol included."""
    hist = {256: 1}
    for value, run in itertools.groupby(segment):
        hist[value] = hist.get(value, 0) + 1
        rest = len(list(run)) - 1
        while rest:
            piece = min(258, rest)
            if piece >= 3:
                sym = 257 + max(i for i, base in enumerate(_LENGTH_BASE) if base <= piece)
                hist[sym] = hist.get(sym, 0) + 1
            else:
                hist[value] += piece
            rest -= piece
    return hist


def _plain_huffman_lengths(hist):
    heap = [(n, i, (s,)) for i, (s, n) in enumerate(sorted(hist.items()))]
    heapq.heapify(heap)
    depth = dict.fromkeys(hist, 0)
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def _dynamic_header(data):
    """The code lengths a dynamic block's header declares: (BFINAL, literal / length lengths, distance lengths, code-length
    lengths).  ``data``: deflate data that begins with the block."""
    bits = int.from_bytes(data[:1024], "little")
    at = 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v
    final, kind = take(1), take(2)
    assert kind == 2
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[_CL_ORDER[i]] = take(3)
    code, next_code = {}, 0                                                         # canonical codes of the code-length code
    for n in range(1, 8):
        for s in range(19):
            if cl[s] == n:
                code[(n, next_code)] = s
                next_code += 1
        next_code <<= 1
    lengths = []
    while len(lengths) < hlit + hdist:
        n = v = 0
        while True:
            v = (v << 1) | take(1)
            n += 1
            assert n <= 7
            if (n, v) in code:
                break
        s = code[(n, v)]
        assert s != 16                                                             # the format does not use "repeat the last length"
        lengths += [s] if s < 16 else [0] * (take(3) + 3 if s == 17 else take(7) + 11)
    assert len(lengths) == hlit + hdist
    return final, lengths[:hlit], lengths[hlit:], cl


def _kraft(lengths):
    return sum(2.0 ** -n for n in lengths if n)


def test_length_limited_codes_on_the_fibonacci_case(files):
    name, rgb, mode = next(c for c in CASES if c[0] == "fibonacci")
    F = pc.filtered_stream(rgb, mode)
    assert len(F) > pc.SEGMENT                                                     # two segments; the first one is full
    hist = _token_histogram(F[:pc.SEGMENT])
    plain = _plain_huffman_lengths(hist)
    assert max(plain.values()) > 15                                                # the case does force the limit
    chunks = pc.walk_chunks(files[name])
    final, lit, dist, cl = _dynamic_header(chunks[1][1][2:])
    assert final == 0 and len(lit) == 286 and dist == [1]
    assert max(lit) == 15 and _kraft(lit) == 1.0 and max(cl) <= 7 and _kraft(cl) == 1.0
    assert {s for s, n in enumerate(lit) if n} == set(hist)                        # codes for the symbols that occur, and 256
    # rarer symbols never get shorter codes than more frequent ones
    by_count = sorted(hist, key=lambda s: hist[s])
    assert all(lit[a] >= lit[b] for a, b in zip(by_count, by_count[1:]) if hist[a] < hist[b])


def test_plain_huffman_lengths_are_kept_where_they_fit(files):
    """Where no length exceeds the limit the code costs what plain Huffman costs (the tie-breaks may differ, the sum cannot)."""
    for name in ("smooth_300_adaptive", "cut_w5462_smooth", "run_1_2_50_n173", "flat_300"):
        _, rgb, mode = next(c for c in CASES if c[0] == name)
        F = pc.filtered_stream(rgb, mode)
        hist = _token_histogram(F[:pc.SEGMENT])
        plain = _plain_huffman_lengths(hist)
        assert max(plain.values()) <= 15
        final, lit, dist, cl = _dynamic_header(pc.walk_chunks(files[name])[1][1][2:])
        assert dist == [1] and _kraft(lit) == 1.0 and _kraft(cl) == 1.0
        assert sum(hist[s] * lit[s] for s in hist) == sum(hist[s] * plain[s] for s in hist), name


def test_host_model_is_deterministic_and_position_independent(files):
    name, rgb, mode = next(c for c in CASES if c[0] == "cut_w5462_smooth")
    shifted = np.empty(rgb.size + 1, np.uint8)[1:].reshape(rgb.shape)               # the same pixels at an odd address
    shifted[...] = rgb
    assert pc.host_encode(shifted, mode)[1] == files[name] == pc.host_encode(rgb, mode)[1]


# ---- the packer ---------------------------------------------------------------------------------------------------------------

def test_png_layout_is_one_upload_in_order():
    shapes, filters = [(2, 5461), (1, 1), (300, 300), (3, 7)], [0, 5, 5, 4]
    layout = data_utils._png_layout(shapes, filters)
    desc = layout["desc"]
    assert desc.dtype == ssd_hip.PNG_DESC_DTYPE and desc.dtype.itemsize == 32 and len(desc) == 4
    assert layout["total"] % 16 == 0 and desc.nbytes <= layout["total"] < desc.nbytes + 16
    segs = [2, 1, 17, 1]
    assert segs == [ssd_hip.lib().ssd_png_segments(h, w) for h, w in shapes]
    assert [int(v) for v in desc["seg_start"]] == [0, 2, 3, 20] and layout["segments"] == 21
    assert [int(v) for v in desc["row_start"]] == [0, 2, 3, 303]
    assert [int(v) for v in desc["src_offset"]] == [0, 32766, 32769, 302769]         # the pixels back to back, any alignment
    assert [(int(d["H"]), int(d["W"])) for d in desc] == shapes and [int(v) for v in desc["filter"]] == filters
    assert int(desc["reserved"].max()) == 0
    bounds = [int(ssd_hip.lib().ssd_png_encode_bound(h, w)) for h, w in shapes]
    assert bounds == [45 + 17 * n + h * (1 + 3 * w) + 6 for n, (h, w) in zip(segs, shapes)]
    assert layout["out_bytes"] == sum(bounds)
    # the workspace holds the filtered stream and the finished chunk data of every segment, and a little more
    ws = int(ssd_hip.lib().ssd_png_encode_workspace_bytes(desc.ctypes.data, 4))
    assert ws % 16 == 0 and 21 * (16384 + 16400) <= ws <= 21 * (16384 + 16400) + 21 * 20 + 256
    assert data_utils._png_filters("paeth", 2) == [4, 4] and data_utils._png_filters(["none", "adaptive"], 2) == [0, 5]
    with pytest.raises(ValueError):
        data_utils._png_filters("best", 1)
    with pytest.raises(ValueError):
        data_utils._png_filters(["up"], 2)


def test_validation_without_a_device():
    """Everything ``ssd_png_encode`` refuses is refused before the first launch, so it can be asked without a GPU."""
    lib = ssd_hip.lib()
    shapes = [(3, 7), (2, 2)]
    layout = data_utils._png_layout(shapes, [5, 0])
    desc = layout["desc"]
    ws = int(lib.ssd_png_encode_workspace_bytes(desc.ctypes.data, 2))
    rgb_bytes = 3 * 7 * 3 + 2 * 2 * 3
    fake = 1 << 20                                                                  # never dereferenced: every call below is refused

    def call(d=desc, B=2, rgb=fake, rgb_n=rgb_bytes, out=fake, out_n=layout["out_bytes"], off=fake, w=fake, w_n=ws, dd=fake):
        return lib.ssd_png_encode(rgb, rgb_n, d.ctypes.data if d is not None else None, dd, B, out, out_n, off, w, w_n, None)
    assert call(B=0, d=None, rgb=None, out=None, off=None, w=None, dd=None) == OK     # a no-op
    assert call(B=-1) == INVALID and call(B=65536) == UNSUPPORTED
    for kw in ({"rgb": None}, {"out": None}, {"off": None}, {"w": None}, {"dd": None}, {"d": None}):
        assert call(**kw) == INVALID, kw
    assert call(w=fake + 8) == INVALID and call(off=fake + 2) == INVALID             # misaligned
    assert call(rgb_n=rgb_bytes - 1) == INVALID                                      # the last image's pixels leave the buffer
    assert call(out_n=layout["out_bytes"] - 1) == INVALID and call(w_n=ws - 1) == INVALID
    for field, value, want in (("seg_start", 2, INVALID), ("row_start", 2, INVALID), ("src_offset", -1, INVALID),
                               ("filter", 6, UNSUPPORTED), ("filter", -1, UNSUPPORTED), ("H", 0, UNSUPPORTED), ("W", 16385, UNSUPPORTED)):
        bad = desc.copy()
        bad[1][field] = value
        assert call(d=bad) == want, field
    big = data_utils._png_layout([(16384, 16384)] * 3, [5] * 3)                      # 3 x 805 MB of filtered stream: above 2^31 - 1
    assert lib.ssd_png_encode(fake, 3 * 16384 * 16384 * 3, big["desc"].ctypes.data, fake, 3, fake, 1 << 40, fake, fake, 1 << 40, None) == UNSUPPORTED
