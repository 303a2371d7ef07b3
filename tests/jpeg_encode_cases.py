"""Shared by the JPEG encoder tests (tests/test_jpeg_encode_cpu.py, tests/test_jpeg_encode_gpu.py), the fixture script
(tests/golden/make_jpeg_encode_golden.py) and tests/bench_jpeg_encode.py: the case list, seeded content, the
Pillow-written fixture, the ctypes calls of the library's host half, and libjpeg-turbo's baseline encoder restated as
NumPy int32 arithmetic in two parts -- colour through quantised coefficients (what ``ssd_jpeg_forward`` computes) and
coefficients to bytes (what ``ssd_jpeg_entropy_encode`` writes)."""
import ctypes
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode.npz")

SIZES = [(1, 1), (8, 8), (16, 16), (17, 15), (37, 53), (64, 48), (33, 100)]        # (H, W)
CONTENTS = ("noise", "gradient", "binary")
QUALITIES = [1, 30, 75, 95, 100]
SUBSAMPLINGS = ["4:4:4", "4:2:2", "4:2:0"]
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}                      # luma (h_samp, v_samp)
DC11 = "dc11_8x16_q100_444"                     # left block black, right block white: a DC difference of category 11


def content(h, w, kind, seed=0):
    """Seeded uint8 [h,w,3]: uniform noise, a gradient with a saturated stripe, or binary 0/255 noise."""
    rng = np.random.default_rng([seed, h, w, CONTENTS.index(kind)])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(yy * 255) // max(h - 1, 1), (xx * 255) // max(w - 1, 1), ((yy + xx) * 255) // max(h + w - 2, 1)], -1)
    a[:, w // 3:w // 3 + max(w // 8, 1)] = (255, 0, 255)                            # the saturated stripe
    return a.astype(np.uint8)


def black_white():
    a = np.zeros((8, 16, 3), np.uint8)
    a[:, 8:] = 255
    return a


def candidates():
    """The whole cross-product, [(name, input key, quality, subsampling)]: every one matches Pillow (checked when the
    fixture is written); the fixture keeps ``cases()``."""
    out = []
    for h, w in SIZES:
        for kind in CONTENTS:
            for q in QUALITIES:
                for s in SUBSAMPLINGS:
                    out.append(("%dx%d_%s_q%d_%s" % (h, w, kind, q, s.replace(":", "")), "%dx%d_%s" % (h, w, kind), q, s))
    return out


def cases():
    """The thinned list the fixture holds: per (size, content) three of the fifteen (quality, subsampling) pairs, rotating,
    so that every input meets all three subsamplings and every pair is met four times; and the category-11 case."""
    out = []
    for p, (h, w, kind) in enumerate((h, w, k) for h, w in SIZES for k in CONTENTS):
        for k, (q, s) in enumerate((q, s) for q in QUALITIES for s in SUBSAMPLINGS):
            if (k + p) % 5 == 0:
                out.append(("%dx%d_%s_q%d_%s" % (h, w, kind, q, s.replace(":", "")), "%dx%d_%s" % (h, w, kind), q, s))
    out.append((DC11, "dc11", 100, "4:4:4"))
    return out


def inputs():
    """{input key: uint8 [H,W,3]} of every case."""
    out = {"%dx%d_%s" % (h, w, k): content(h, w, k) for h, w in SIZES for k in CONTENTS}
    out["dc11"] = black_white()
    return out


def pillow_encode(arr, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def pillow_is_turbo():
    try:
        from PIL import features
        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:
        return False


def load_fixture():
    """{name: (uint8 [H,W,3] input, quality, subsampling, Pillow's JPEG bytes)} in ``cases()`` order, and the versions
    that wrote it."""
    z = np.load(GOLDEN)
    out = {}
    for name, key, q, s in cases():
        out[name] = (z["in_" + key], q, s, z["jpeg_" + name].tobytes())
    return out, str(z["versions"])


# ---- the standard's tables (ITU-T T.81 Annex K), natural order

STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                       47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])


def _run(a, b):
    return list(range(a, b + 1))


DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _run(0, 11))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _run(0, 11))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
            0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A]
           + _run(0x16, 0x1A) + _run(0x25, 0x2A) + _run(0x34, 0x3A) + _run(0x43, 0x4A) + _run(0x53, 0x5A) + _run(0x63, 0x6A)
           + _run(0x73, 0x7A) + _run(0x83, 0x8A) + _run(0x92, 0x9A) + _run(0xA2, 0xAA) + _run(0xB2, 0xBA) + _run(0xC2, 0xCA)
           + _run(0xD2, 0xDA) + _run(0xE1, 0xEA) + _run(0xF1, 0xFA))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
              0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16,
              0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A] + _run(0x26, 0x2A) + _run(0x35, 0x3A) + _run(0x43, 0x4A)
             + _run(0x53, 0x5A) + _run(0x63, 0x6A) + _run(0x73, 0x7A) + _run(0x82, 0x8A) + _run(0x92, 0x9A) + _run(0xA2, 0xAA)
             + _run(0xB2, 0xBA) + _run(0xC2, 0xCA) + _run(0xD2, 0xDA) + _run(0xE2, 0xEA) + _run(0xF2, 0xFA))


def quality_tables(quality):
    """``jpeg_set_quality(quality, force_baseline)``: uint16 [2,64], natural order, luma then chroma."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA)]).astype(np.uint16)


# ---- colour through quantised coefficients, as NumPy int32 arithmetic

class Geometry(object):
    """The coefficient storage of ``struct ssd_jpeg_info`` for an H x W image with h x v luma sampling: per component the
    padded plane in blocks (``bw``, ``bh``), the real blocks (``rw``, ``rh``) and the int16 offset of the plane."""

    def __init__(self, H, W, hs, vs):
        self.H, self.W, self.hs, self.vs = H, W, hs, vs
        self.mcus_x, self.mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
        self.h, self.v = (hs, 1, 1), (vs, 1, 1)
        self.bw = [self.mcus_x * h for h in self.h]
        self.bh = [self.mcus_y * v for v in self.v]
        self.rw = [-(-(-(-W * h // hs)) // 8) for h in self.h]
        self.rh = [-(-(-(-H * v // vs)) // 8) for v in self.v]
        self.at = [0]
        for c in range(3):
            self.at.append(self.at[-1] + self.bw[c] * self.bh[c] * 64)
        self.n = self.at[3]

    def plane(self, coef, c):
        """Component ``c``'s blocks as a view [bh, bw, 64] of the flat int16 storage."""
        return coef[self.at[c]:self.at[c + 1]].reshape(self.bh[c], self.bw[c], 64)

    def real(self, coef):
        """The real blocks of all three components, concatenated: what the device half must get right."""
        return np.concatenate([self.plane(coef, c)[:self.rh[c], :self.rw[c]].reshape(-1) for c in range(3)])


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component_planes(rgb, hs, vs, pad_input_rows_first=False):
    """The three uint8-valued int32 planes the forward DCT reads, padded to whole MCUs.  ``pad_input_rows_first``: the
    wrong reading of the vertical edge (input rows replicated to the MCU height before downsampling)."""
    H, W = rgb.shape[:2]
    g = Geometry(H, W, hs, vs)
    rows = g.mcus_y * 8 * vs if pad_input_rows_first else -(-H // vs) * vs           # whole row groups only
    full = [_edge(p, rows, g.mcus_x * 8 * hs) for p in rgb_to_ycc(rgb)]              # last column out to the MCU width
    out = [full[0]]
    for p in full[1:]:
        if hs == 2 and vs == 1:
            bias = np.arange(p.shape[1] // 2, dtype=np.int32) & 1                     # 0, 1, 0, 1, ...
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif hs == 2 and vs == 2:
            bias = 1 + (np.arange(p.shape[1] // 2, dtype=np.int32) & 1)               # 1, 2, 1, 2, ...
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(p)
    return [_edge(p, g.bh[c] * 8, g.bw[c] * 8) for c, p in enumerate(out)]           # last DOWNSAMPLED row to the MCU height


def _fdct_1d(d, first):
    """One 8-point pass of libjpeg's "islow" forward DCT on a list of eight int32 arrays."""
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    ds = lambda v: (v + (1 << (n - 1))) >> n                                          # noqa: E731
    out = [None] * 8
    if first:
        out[0], out[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        out[0], out[4] = (tmp10 + tmp11 + 2) >> 2, (tmp10 - tmp11 + 2) >> 2
    z1 = (tmp12 + tmp13) * 4433
    out[2], out[6] = ds(z1 + tmp13 * 6270), ds(z1 - tmp12 * 15137)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = ds(tmp4 + z1 + z3), ds(tmp5 + z2 + z4), ds(tmp6 + z2 + z3), ds(tmp7 + z1 + z4)
    return out


def fdct_quantise(plane, quant):
    """int32 samples [bh*8, bw*8] + uint16 [64] table -> int16 [bh, bw, 64] quantised coefficients, natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.astype(np.int32).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128      # [bh,bw,row,col]
    rows = np.stack(_fdct_1d([x[..., k] for k in range(8)], True), -1)               # pass 1: along the rows
    d = np.stack(_fdct_1d([rows[:, :, r, :] for r in range(8)], False), 2)           # pass 2: down the columns
    q = quant.astype(np.int32).reshape(8, 8)
    return (np.sign(d) * ((np.abs(d) + 4 * q) // (8 * q))).astype(np.int16).reshape(bh, bw, 64)


def forward(rgb, subsampling, tables, pad_input_rows_first=False):
    """``(Geometry, int16 coefficient storage)``: what ``ssd_jpeg_forward`` writes for one image (every block of the
    padded planes is computed here; only the real ones are specified)."""
    hs, vs = SAMPLING[subsampling]
    g = Geometry(rgb.shape[0], rgb.shape[1], hs, vs)
    planes = component_planes(rgb, hs, vs, pad_input_rows_first)
    coef = np.concatenate([fdct_quantise(p, tables[min(c, 1)]).reshape(-1) for c, p in enumerate(planes)])
    assert coef.size == g.n
    return g, coef


# ---- coefficients to bytes

def _huff_codes(bits, vals):
    """{symbol: (code, length)} of a table given as the DHT segment gives it."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _dht(cls_id, table):
    bits, vals = table
    return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([cls_id]) + bytes(bits) + bytes(vals)


def header(g, tables):
    out = b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for i in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(tables[i][z]) for z in ZIGZAG)
    out += b"\xff\xc0\x00\x11\x08" + g.H.to_bytes(2, "big") + g.W.to_bytes(2, "big") + b"\x03"
    out += bytes([1, (g.hs << 4) | g.vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    out += _dht(0x00, DC_LUMA) + _dht(0x10, AC_LUMA) + _dht(0x01, DC_CHROMA) + _dht(0x11, AC_CHROMA)
    return out + b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"


def entropy_encode(g, coef, tables, stats=None):
    """The whole JPEG stream of the coefficient storage ``coef`` (only real blocks are read; the dummy blocks of the last
    MCU column and row are synthesised: AC zero, DC of the block emitted before them in the MCU).  ``stats``: a dict that
    receives the counts the fixture script asserts on."""
    dc = [_huff_codes(*DC_LUMA), _huff_codes(*DC_CHROMA)]
    ac = [_huff_codes(*AC_LUMA), _huff_codes(*AC_CHROMA)]
    st = {"zrl": 0, "stuffed": 0, "dummy_right": 0, "dummy_bottom": 0, "dummy_corner": 0, "max_dc_category": 0}
    acc, nbits = 0, 0
    pred = [0, 0, 0]
    planes = [g.plane(coef, c) for c in range(3)]

    def emit_block(block, c):
        nonlocal acc, nbits
        t = min(c, 1)
        diff = int(block[0]) - pred[c]
        pred[c] = int(block[0])
        n = abs(diff).bit_length()
        st["max_dc_category"] = max(st["max_dc_category"], n)
        assert n <= 11
        code, length = dc[t][n]
        acc, nbits = (acc << length) | code, nbits + length
        if n:
            acc, nbits = (acc << n) | ((diff if diff >= 0 else diff - 1) & ((1 << n) - 1)), nbits + n
        run = 0
        for k in range(1, 64):
            v = int(block[ZIGZAG[k]])
            if v == 0:
                run += 1
                continue
            while run > 15:
                code, length = ac[t][0xF0]
                acc, nbits = (acc << length) | code, nbits + length
                st["zrl"] += 1
                run -= 16
            n = abs(v).bit_length()
            assert n <= 10
            code, length = ac[t][(run << 4) | n]
            acc, nbits = (acc << length) | code, nbits + length
            acc, nbits = (acc << n) | ((v if v >= 0 else v - 1) & ((1 << n) - 1)), nbits + n
            run = 0
        if run:
            code, length = ac[t][0x00]
            acc, nbits = (acc << length) | code, nbits + length

    zero = np.zeros(64, np.int16)
    for my in range(g.mcus_y):
        for mx in range(g.mcus_x):
            for c in range(3):
                last = None
                for v in range(g.v[c]):
                    for u in range(g.h[c]):
                        by, bx = my * g.v[c] + v, mx * g.h[c] + u
                        if by < g.rh[c] and bx < g.rw[c]:
                            last = planes[c][by, bx]
                        else:
                            st["dummy_corner" if by >= g.rh[c] and bx >= g.rw[c] else
                               "dummy_bottom" if by >= g.rh[c] else "dummy_right"] += 1
                            dummy = zero.copy()
                            dummy[0] = last[0]
                            last = dummy
                        emit_block(last, c)
    pad = -nbits % 8
    acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
    data = acc.to_bytes(nbits // 8, "big")
    st["stuffed"] = data.count(b"\xff")
    if stats is not None:
        stats.update(st)
    return header(g, tables) + data.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def restate(rgb, quality, subsampling, stats=None):
    """Pillow's ``save(f, "JPEG", quality=quality, subsampling=subsampling)`` bytes of a uint8 [H,W,3] array."""
    tables = quality_tables(quality)
    g, coef = forward(rgb, subsampling, tables)
    return entropy_encode(g, coef, tables, stats)


# ---- the library's host half through ctypes

def lib_quality_tables(quality):
    import ssd_hip
    out = np.zeros((2, 64), np.uint16)
    rc = ssd_hip.lib().ssd_jpeg_quality_tables(int(quality), out.ctypes.data)
    assert rc == 0, ssd_hip.lib().ssd_last_error().decode()
    return out


def lib_info(H, W, subsampling, tables):
    """``(return code, JpegInfo)`` of ``ssd_jpeg_encode_info``."""
    import ssd_hip
    hs, vs = SAMPLING[subsampling]
    info = ssd_hip.JpegInfo()
    t = np.ascontiguousarray(tables, np.uint16)
    rc = ssd_hip.lib().ssd_jpeg_encode_info(int(W), int(H), hs, vs, t.ctypes.data, ctypes.byref(info))
    return rc, info


def lib_entropy_encode(coef, info, out_bytes=None, guard=64, fill=0xA5):
    """``(return code, the bytes written, guard bands intact)`` of ``ssd_jpeg_entropy_encode`` writing into the middle of a
    buffer whose ``guard`` bytes before and after must stay ``fill``.  ``out_bytes``: default ``ssd_jpeg_encode_bound``."""
    import ssd_hip
    lib = ssd_hip.lib()
    n = int(lib.ssd_jpeg_encode_bound(ctypes.byref(info))) if out_bytes is None else int(out_bytes)
    store = np.full(n + 2 * guard, fill, np.uint8)
    written = ctypes.c_size_t(0)
    coef = np.ascontiguousarray(coef, np.int16)
    rc = lib.ssd_jpeg_entropy_encode(coef.ctypes.data, ctypes.byref(info), store.ctypes.data + guard, n, ctypes.byref(written))
    intact = bool((store[:guard] == fill).all() and (store[n + guard:] == fill).all())
    return rc, store[guard:guard + min(int(written.value), n)].tobytes() if rc == 0 else b"", intact
