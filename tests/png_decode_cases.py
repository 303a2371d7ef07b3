"""Cases for the PNG decoder (``ssd_png_parse`` / ``ssd_png_decode_host`` / ``ssd_png_decode``): a pure-Python PNG writer
(``struct`` + ``zlib``) with a forced filter per row, its own filter arithmetic and a choice of IDAT splitting, and the
named files the CPU and GPU tests share.  The oracle of every case is Pillow's decode of the same bytes
(``pillow_outcome``): it knows nothing of this writer nor of the library.  All cases are tiny: the smallest sizes at which
the kernels can still go wrong -- widths around the 4 pipeline steps whose loads are issued together and around the 256
threads of a converted row, heights around the 64 rows of a band."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# every (colour type, depth) the library takes
FORMATS = [(2, 8), (2, 16), (6, 8), (6, 16), (0, 1), (0, 2), (0, 4), (0, 8), (4, 8), (4, 16), (3, 1), (3, 2), (3, 4), (3, 8)]
UNSUPPORTED, INVALID = -3, -1


def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def row_bytes(W, color_type, depth):
    return (W * CHANNELS[color_type] * depth + 7) // 8


def filter_distance(color_type, depth):
    return max(1, CHANNELS[color_type] * depth // 8)


def filtered_stream(raw, fd, types):
    """``raw`` uint8 [H, row_bytes] -> the filtered stream, row y under filter ``types[y]`` (a type above 4 filters as None)."""
    H, rb = raw.shape
    out = np.zeros((H, 1 + rb), np.uint8)
    prev = np.zeros(rb, np.int64)
    for y in range(H):
        row = raw[y].astype(np.int64)
        a = np.concatenate([np.zeros(fd, np.int64), row])[:rb]
        b = prev
        c = np.concatenate([np.zeros(fd, np.int64), prev])[:rb]
        t = int(types[y])
        if t == 1:
            pred = a
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (a + b) // 2
        elif t == 4:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:
            pred = np.zeros(rb, np.int64)
        out[y, 0] = t
        out[y, 1:] = (row - pred) & 255
        prev = row
    return out.tobytes()


def split_at(data, cuts):
    """``data`` cut at the byte positions ``cuts`` (ascending; equal neighbours make an empty piece)."""
    edges = [0] + list(cuts) + [len(data)]
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


def write_png(W, H, color_type, depth, raw, types, palette=None, cuts=(), before_idat=(), interlace=0, stream=None):
    """The file: IHDR, PLTE (``palette``: bytes), the chunks of ``before_idat`` ((kind, data) pairs), the zlib stream of
    the filtered rows (or ``stream``, taken as it is) cut into IDAT chunks at ``cuts``, IEND."""
    if stream is None:
        stream = zlib.compress(filtered_stream(raw, filter_distance(color_type, depth), types), 6)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", palette)
    for kind, data in before_idat:
        out += chunk(kind, data)
    for piece in split_at(stream, cuts):
        out += chunk(b"IDAT", piece)
    return out + chunk(b"IEND")


def _random(rng, W, H, color_type, depth):
    return rng.integers(0, 256, (H, row_bytes(W, color_type, depth)), dtype=np.uint8)


def _palette(rng, entries=256):
    return rng.integers(0, 256, 3 * entries, dtype=np.uint8).tobytes()


def _case(name, W, H, color_type, depth, blob):
    return {"name": name, "blob": blob, "W": W, "H": H, "color_type": color_type, "depth": depth}


def _written(name, rng, W, H, color_type, depth, types, **kw):
    if color_type == 3 and "palette" not in kw:
        kw["palette"] = _palette(rng, 1 << depth)
    raw = kw.pop("raw", None)
    if raw is None:
        raw = _random(rng, W, H, color_type, depth)
    types = [types] * H if isinstance(types, int) else list(types)
    return _case(name, W, H, color_type, depth, write_png(W, H, color_type, depth, raw, types, **kw))


def paeth_tie_rows():
    """uint8 [1024, 2] grey rows and their filters: for every (a, b, c) over eight values -- the ends of the range, its
    middle, neighbours -- a None row (c, b) and under it a Paeth row (a, .): pa == pb, pb == pc, pa == pc, all equal, and
    sums that wrap modulo 256 all occur."""
    values = [0, 1, 2, 64, 127, 128, 254, 255]
    rows, types = [], []
    for a in values:
        for b in values:
            for c in values:
                rows += [[c, b], [a, (a * 7 + b * 3 + c) & 255]]
                types += [0, 4]
    return np.array(rows, np.uint8), types


def written_cases():
    rng = np.random.default_rng(20261019)
    out = []
    for ct, depth in FORMATS:                                                       # 13: no multiple of 8, 4 or 2 pixels per byte
        out.append(_written("format_ct%d_d%d_13x5" % (ct, depth), rng, 13, 5, ct, depth, [0, 1, 2, 3, 4]))
    for ct, depth in [(0, 8), (0, 1), (0, 2), (0, 4), (4, 8), (2, 8), (6, 8), (4, 16), (2, 16), (6, 16)]:   # distances 1 1 1 1 2 3 4 4 6 8
        for t in range(5):
            out.append(_written("filter%d_ct%d_d%d_7x3" % (t, ct, depth), rng, 7, 3, ct, depth, t))
    for t in (2, 3, 4):                                                             # row 0: nothing above it
        for W, H in ((1, 1), (1, 9), (9, 1)):
            out.append(_written("row0_filter%d_%dx%d" % (t, W, H), rng, W, H, 2, 8, t))
    raw, types = paeth_tie_rows()
    out.append(_written("paeth_ties", rng, 2, len(types), 0, 8, types, raw=raw))
    out.append(_written("paeth_extremes_9x9", rng, 9, 9, 2, 8, 4, raw=rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), (9, 27))))
    for t, label in ((4, "paeth"), (3, "average")):                                 # the 64 rows of a band
        for H in (63, 64, 65, 129):
            out.append(_written("band_%s_5x%d" % (label, H), rng, 5, H, 2, 8, t))
    for W in (3, 4, 5, 63, 64, 65, 255, 256, 257):                                  # 4 steps of loads, 256 threads of a row
        out.append(_written("width_%dx3" % W, rng, W, 3, 2, 8, [1, 4, 3]))
        out.append(_written("width_grey_%dx3" % W, rng, W, 3, 0, 8, [4, 4, 3]))
    out.append(_written("width_bits_257x3", rng, 257, 3, 3, 2, [3, 4, 4]))
    pattern = [4, 4, 0, 4, 1, 3, 2, 2, 0, 0, 4]
    out.append(_written("chains_pattern_6x11", rng, 6, 11, 6, 8, pattern))
    out.append(_written("chains_of_one_5x9", rng, 5, 9, 2, 8, [0, 1, 0, 1, 1, 0, 0, 1, 0]))
    out.append(_written("chain_at_row_64_5x71", rng, 5, 71, 2, 8, [4] * 64 + [1] + [4, 3, 2, 4, 3, 2]))
    out.append(_written("one_chain_130_rows_5x130", rng, 5, 130, 4, 8, [4] + [2, 3, 4] * 43))
    out.append(_written("short_palette_13x5", rng, 13, 5, 3, 8, [0, 1, 2, 3, 4], palette=_palette(rng, 4)))
    base = dict(raw=_random(rng, 13, 5, 2, 8))
    n = len(zlib.compress(filtered_stream(base["raw"], 3, [0, 1, 2, 3, 4]), 6))
    out.append(_written("idat_one", rng, 13, 5, 2, 8, [0, 1, 2, 3, 4], **base))
    out.append(_written("idat_many", rng, 13, 5, 2, 8, [0, 1, 2, 3, 4], cuts=range(7, n, 7), **base))
    out.append(_written("idat_empty_pieces", rng, 13, 5, 2, 8, [0, 1, 2, 3, 4], cuts=(0, 20, 20), **base))
    out.append(_written("idat_split_in_zlib_header", rng, 13, 5, 2, 8, [0, 1, 2, 3, 4], cuts=(1,), **base))
    extra = [(b"gAMA", struct.pack(">I", 45455)), (b"tRNS", bytes(6)), (b"tEXt", b"Comment\0a test")]
    out.append(_written("ancillary_rgb", rng, 13, 5, 2, 8, [0, 1, 2, 3, 4], before_idat=extra, **base))
    out.append(_written("ancillary_palette_trns", rng, 13, 5, 3, 4, [0, 1, 2, 3, 4], before_idat=[(b"tRNS", bytes(range(0, 160, 10)))]))
    out.append(_written("ancillary_grey_trns", rng, 13, 5, 0, 8, [0, 1, 2, 3, 4], before_idat=[(b"tRNS", b"\0\x07")]))
    return out


def _pictures():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:50, 0:40]
    smooth = np.stack([128 + 100 * np.sin(yy / 9.0 + c) * np.cos(xx / 6.0) for c in range(4)], -1).astype(np.uint8)
    return {"smooth": smooth, "noise": rng.integers(0, 256, (50, 40, 4), dtype=np.uint8)}


def pillow_cases():
    """Files Pillow writes: 40 x 50, smooth and noise, in RGB, RGBA, L and P (default and ``optimize=True``)."""
    from PIL import Image
    out = []
    for label, px in _pictures().items():
        images = {"RGB": (Image.fromarray(px[..., :3]), 2), "RGBA": (Image.fromarray(px), 6), "L": (Image.fromarray(px[..., 0]), 0),
                  "P": (Image.fromarray(px[..., :3]).quantize(37), 3)}
        for mode, (im, ct) in images.items():
            for optimize in (False, True):
                buf = io.BytesIO()
                im.save(buf, "PNG", optimize=optimize)
                depth = None if mode == "P" else 8                                 # Pillow picks the palette's depth
                out.append(_case("pillow_%s_%s%s" % (label, mode, "_optimize" if optimize else ""), 40, 50, ct, depth, buf.getvalue()))
    return out


def project_cases():
    """The project's own files: ``ssd_png_encode_host`` in each filter mode and in adaptive mode (needs the library)."""
    import png_cases as pc
    px = _pictures()["smooth"][..., :3]
    out = []
    for mode in range(6):
        rc, blob = pc.host_encode(np.ascontiguousarray(px), mode)[:2]
        assert rc == 0
        out.append(_case("project_filter%d" % mode, 40, 50, 2, 8, bytes(blob)))
    return out


def accepted_cases():
    return written_cases() + pillow_cases() + project_cases()


def refusal_cases():
    """``name, blob, code``: what ``ssd_png_parse`` answers (``UNSUPPORTED``, ``INVALID``, or 0 where the file parses and
    the inflate step refuses it)."""
    rng = np.random.default_rng(3)
    raw = _random(rng, 13, 5, 2, 8)
    types = [0, 1, 2, 3, 4]
    good = write_png(13, 5, 2, 8, raw, types)
    F = filtered_stream(raw, 3, types)
    flipped = bytearray(good)
    flipped[good.index(b"IDAT") + 9] ^= 0x10                                         # a data byte: the chunk's CRC no longer fits
    return [
        ("interlaced_1x1", write_png(1, 1, 2, 8, raw[:1, :3], [0], interlace=1), UNSUPPORTED),
        ("grey_16", write_png(13, 5, 0, 16, _random(rng, 13, 5, 0, 16), types), UNSUPPORTED),
        ("crc_bit_flipped", bytes(flipped), INVALID),
        ("filter_byte_5", write_png(13, 5, 2, 8, raw, [0, 1, 5, 3, 4]), 0),
        ("inflated_short", write_png(13, 5, 2, 8, raw, types, stream=zlib.compress(F[:-3])), 0),
        ("inflated_long", write_png(13, 5, 2, 8, raw, types, stream=zlib.compress(F + bytes(5))), 0),
        ("cut_mid_chunk", good[:-20], INVALID),
        ("no_png", b"P6 13 5 255 " + bytes(195), INVALID),
        ("type_3_without_plte", write_png(13, 5, 3, 8, _random(rng, 13, 5, 3, 8), types), INVALID),
    ]


def pillow_outcome(blob):
    """``("pixels", uint8 [H,W,3])`` or ``("raises", the exception's type)``: what the road before this decoder did."""
    import warnings
    from PIL import Image
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return "pixels", np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)
    except Exception as e:                                                          # noqa: BLE001 -- whatever Pillow raises is the contract
        return "raises", type(e)
