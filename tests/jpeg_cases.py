"""Shared by the JPEG tests (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py), the fixture script
(tests/golden/make_jpeg_golden.py) and tests/bench_jpeg.py: the case list, seeded content, the Pillow-written fixture, the
ctypes calls of the library's host half, and the four device stages (dequantise + islow IDCT, range limit, fancy
upsampling, YCbCr -> RGB) restated as NumPy int32 arithmetic on the library's coefficients."""
import ctypes
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz")

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (33, 17), (40, 24)]          # (H, W)
MODES = ["444", "422", "420", "L"]
QUALITIES = [1, 30, 92, 100]
CONTENTS = ("smooth", "noise")
_SUBSAMPLING = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}
# restart intervals: 5 MCUs per row (not divisible by 3) and more than 8 intervals, so the RSTn counter wraps past 7
RESTART_420 = (32, 72)          # 4:2:0, 16x16 MCUs: 5 x 2 = 10 intervals of 1
RESTART_444 = (48, 40)          # 4:4:4, 8x8 MCUs: 5 x 6 = 30 MCUs, 10 intervals of 3 that straddle the rows
REAL_SIZE = (375, 500)          # generated in the tests, not part of the fixture


def content(h, w, mode, kind, seed=0):
    """Seeded uint8 [h,w,3] (or [h,w] for mode L): smooth structure plus a little noise, or pure noise."""
    rng = np.random.default_rng([seed, h, w, CONTENTS.index(kind), MODES.index(mode)])
    ch = 1 if mode == "L" else 3
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        a = np.stack([127.5 + 100.0 * np.sin(yy / (5.0 + 2 * c) + seed) * np.cos(xx / (7.0 - c)) + rng.normal(0, 10.0, (h, w))
                      for c in range(ch)], -1)
        a = np.clip(a, 0, 255).astype(np.uint8)
    return a[..., 0] if mode == "L" else a


def cases():
    """[(name, (H, W), mode, content kind, Pillow save options)]: the smallest shapes at which each mechanism can fail."""
    out = []
    for h, w in SIZES:                                  # partial blocks, one MCU with both edges replicated, odd chroma sizes
        for mode in MODES:
            out.append(("size_%dx%d_%s" % (h, w, mode), (h, w), mode, "smooth", {"quality": 92}))
    for q in QUALITIES:                                 # range-limit wrap, large coefficients, byte stuffing, long codes
        for kind in CONTENTS:
            for mode in MODES:
                out.append(("q%d_%s_%s" % (q, kind, mode), (17, 17), mode, kind, {"quality": q}))
    out.append(("optimize_420", (33, 17), "420", "noise", {"quality": 92, "optimize": True}))
    out.append(("optimize_L", (40, 24), "L", "smooth", {"quality": 30, "optimize": True}))
    out.append(("restart1_420", RESTART_420, "420", "smooth", {"quality": 92, "restart_marker_blocks": 1}))
    out.append(("restart3_444", RESTART_444, "444", "smooth", {"quality": 92, "restart_marker_blocks": 3}))
    out.append(("restart3_L", (40, 24), "L", "noise", {"quality": 92, "restart_marker_blocks": 3}))
    out.append(("exif_com_422", (16, 16), "422", "smooth", {"quality": 92, "comment": b"a comment segment", "exif": "exif"}))
    return out


def encode(arr, mode, options):
    """Pillow's JPEG bytes of ``arr``."""
    from PIL import Image
    opts = dict(options)
    if opts.get("exif") == "exif":
        ex = Image.Exif()
        ex[0x010E] = "an EXIF segment"
        opts["exif"] = ex
    if mode != "L":
        opts["subsampling"] = _SUBSAMPLING[mode]
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **opts)
    return buf.getvalue()


def pillow_decode(blob):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)


def pillow_is_turbo():
    try:
        from PIL import features
        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:
        return False


def real_size_blob(seed=5):
    h, w = REAL_SIZE
    return encode(content(h, w, "420", "smooth", seed), "420", {"quality": 92})


def load_fixture():
    """{name: (JPEG bytes, Pillow's RGB uint8 [H,W,3])} in ``cases()`` order, and the versions that wrote it."""
    z = np.load(GOLDEN)
    out = {}
    for name, _, _, _, _ in cases():
        out[name] = (z["jpeg_" + name].tobytes(), z["rgb_" + name])
    return out, str(z["versions"])


# ---- the library's host half through ctypes

def parse(blob):
    """``(return code, JpegInfo, error text)`` of ``ssd_jpeg_parse``."""
    import ssd_hip
    lib = ssd_hip.lib()
    info = ssd_hip.JpegInfo()
    buf = (ctypes.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob.ljust(1, b"\0"))
    rc = lib.ssd_jpeg_parse(ctypes.addressof(buf), len(blob), ctypes.byref(info))
    return rc, info, lib.ssd_last_error().decode() if rc else ""


def entropy_decode(blob, info, guard=64, fill=0x5A5A):
    """``(return code, coefficients int16 [coef_bytes / 2], guard bands intact)`` of ``ssd_jpeg_entropy_decode`` writing
    into the middle of a buffer whose ``guard`` int16 before and after must stay ``fill``."""
    import ssd_hip
    n = int(info.coef_bytes) // 2
    store = np.full(n + 2 * guard, fill, np.int16)
    buf = (ctypes.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob.ljust(1, b"\0"))
    rc = ssd_hip.lib().ssd_jpeg_entropy_decode(ctypes.addressof(buf), len(blob), ctypes.byref(info),
                                              store.ctypes.data + 2 * guard, n * 2)
    intact = bool((store[:guard] == fill).all() and (store[n + guard:] == fill).all())
    return rc, store[guard:n + guard].copy(), intact


# ---- the device stages as NumPy int32 arithmetic

def _i32(x):
    return np.asarray(x, dtype=np.int32)


def _idct_1d(v, shift):
    """One 8-point pass of libjpeg's "islow" inverse DCT on a list of eight int32 arrays (wrapping int32)."""
    c = lambda k: np.int32(k)                                                       # noqa: E731
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * c(4433)
    tmp2 = z1 + z3 * c(-15137)
    tmp3 = z1 + z2 * c(6270)
    tmp0 = (v[0] + v[4]) * c(8192)
    tmp1 = (v[0] - v[4]) * c(8192)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * c(2446), tmp1 * c(16819), tmp2 * c(25172), tmp3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = c(1 << (shift - 1))
    pairs = [(tmp10, tmp3), (tmp11, tmp2), (tmp12, tmp1), (tmp13, tmp0)]
    out = [None] * 8
    for i, (a, b) in enumerate(pairs):
        out[i] = (a + b + half) >> shift
        out[7 - i] = (a - b + half) >> shift
    return out


def range_limit(v):
    """libjpeg's post-IDCT range-limit table as a function of the masked index (it wraps; it is not a clamp)."""
    i = _i32(v) & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.int32)


def idct_plane(coef_blocks, quant):
    """int16 [bh,bw,64] quantised coefficients (natural order) + uint16 [64] table -> int32 samples [bh*8, bw*8]."""
    bh, bw = coef_blocks.shape[:2]
    with np.errstate(over="ignore"):
        x = _i32(coef_blocks).reshape(bh, bw, 8, 8) * _i32(quant).reshape(8, 8)
        cols = _idct_1d([x[:, :, r, :] for r in range(8)], 11)                     # pass 1: down the columns
        ws = np.stack(cols, 2)                                                      # [bh,bw,row,col]
        rows = _idct_1d([ws[:, :, :, k] for k in range(8)], 18)                    # pass 2: along the rows
    s = range_limit(np.stack(rows, 3))
    return s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(s):
    """Fancy 2:1 horizontal upsampling of the REAL samples ``s`` [rows, cw] -> [rows, 2 cw]."""
    s = _i32(s)
    cw = s.shape[1]
    if cw <= 2:
        return np.repeat(s, 2, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    even = (3 * s + left + 1) >> 2
    odd = (3 * s + right + 2) >> 2
    even[:, 0] = s[:, 0]
    odd[:, -1] = s[:, -1]
    return np.stack([even, odd], 2).reshape(s.shape[0], 2 * cw)


def upsample_h2v2(s, replicate_row=None):
    """Fancy 2:1 x 2:1 upsampling of the REAL samples ``s`` [ch, cw] -> [2 ch, 2 cw].  ``replicate_row``: the row that
    stands below the last one (default: the last real row itself)."""
    s = _i32(s)
    ch, cw = s.shape
    if cw <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    below_last = s[-1:] if replicate_row is None else _i32(replicate_row)[None, :]
    above = np.concatenate([s[:1], s[:-1]], 0)
    below = np.concatenate([s[1:], below_last], 0)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    for parity, far in ((0, above), (1, below)):
        t = 3 * s + far
        left = np.concatenate([t[:, :1], t[:, :-1]], 1)
        right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
        even = (3 * t + left + 8) >> 4
        odd = (3 * t + right + 7) >> 4
        even[:, 0] = (4 * t[:, 0] + 8) >> 4
        odd[:, -1] = (4 * t[:, -1] + 7) >> 4
        out[parity::2] = np.stack([even, odd], 2).reshape(ch, 2 * cw)
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = _i32(y), _i32(cb) - 128, _i32(cr) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def restate(info, coef, bottom="real"):
    """RGB uint8 [H,W,3] from the library's coefficients.  ``bottom``: which chroma row 4:2:0 replicates below the last
    real one -- "real" (the last real row) or "padded" (the next row of the padded block), the issue's open point."""
    H, W, nc = info.height, info.width, info.components
    planes = []
    for c in range(nc):
        bw, bh = info.blocks_w[c], info.blocks_h[c]
        at = int(info.coef_offset[c]) // 2
        blocks = coef[at:at + bw * bh * 64].reshape(bh, bw, 64)
        planes.append(idct_plane(blocks, np.array(info.quant[c][:], np.uint16)))
    y = planes[0][:H, :W]
    if nc == 1:
        return np.repeat(y[:, :, None], 3, 2).astype(np.uint8)
    hs, vs = info.h_samp[0], info.v_samp[0]
    cw, ch = -(-W // hs), -(-H // vs)
    up = []
    for p in planes[1:]:
        s = p[:ch, :cw]
        if hs == 1:
            u = s
        elif vs == 1:
            u = upsample_h2v1(s)
        else:
            nxt = p[ch, :cw] if bottom == "padded" and ch < p.shape[0] else None
            u = upsample_h2v2(s, nxt)
        up.append(u[:H, :W])
    return ycc_to_rgb(y, up[0], up[1])
