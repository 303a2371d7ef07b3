"""Cases for the device inflater (``ssd_png_inflate`` / ``ssd_png_inflate_host``).  A case is ``(name, zlib stream, H,
row_bytes)``; what it inflates to is a valid filtered stream (filter bytes <= 4) and the reference is Python's ``zlib``.
The streams come from ``zlib.compressobj`` in its levels, strategies and window sizes, from the project's own encoder, and
from a small bit writer where zlib's compressor never goes (length 258 at distance 1, distance 32768, a code of 15 bits, a
block without any distance code, a repeat of code lengths across the literal / distance border).  ``walk`` is a small deflate reader -- test
code only -- that says what a stream contains; ``coverage()`` asserts the accepted set holds everything named in it.  A
refusal case carries the name of the status bit (``ssd_hip.PNG_INFLATE_STATUS``) the inflater documents for its cause."""
import functools
import zlib

import numpy as np

import png_decode_cases as pdc

ROW = 128                           # the hand-built cases: grey 8-bit rows of 1 + 127 bytes


# ---- a bit writer ----------------------------------------------------------------------------------------------------
class Bits(object):
    def __init__(self):
        self.out, self.cur, self.fill = bytearray(), 0, 0

    def put(self, value, n):
        """``n`` bits of ``value``, least significant first."""
        self.cur |= (value & ((1 << n) - 1)) << self.fill
        self.fill += n
        while self.fill >= 8:
            self.out.append(self.cur & 255)
            self.cur >>= 8
            self.fill -= 8

    def code(self, code, n):
        """A Huffman code: most significant bit first."""
        self.put(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.fill:
            self.put(0, 8 - self.fill)

    def bytes(self):
        self.align()
        return bytes(self.out)


LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def _symbol_of(value, base):
    return max(i for i, b in enumerate(base) if b <= value)


def put_tokens(w, tokens, lit, dist):
    """``tokens``: a literal's int, ``(length, distance)``, ``("lit", symbol)`` or ``("dist", symbol)`` (a bare symbol, for
    the refusal cases).  The end-of-block code is the caller's."""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "lit":
            w.code(*lit[t[1]])
        elif t[0] == "dist":
            w.code(*dist[t[1]])
        else:
            ls = 28 if t[0] == 258 else _symbol_of(t[0], LENGTH_BASE[:28])
            w.code(*lit[257 + ls])
            w.put(t[0] - LENGTH_BASE[ls], LENGTH_EXTRA[ls])
            ds = _symbol_of(t[1], DIST_BASE)
            w.code(*dist[ds])
            w.put(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])


def fixed_block(w, tokens, final, end=True):
    w.put(final, 1)
    w.put(1, 2)
    lit = canonical(FIXED_LIT)
    put_tokens(w, tokens, lit, canonical(FIXED_DIST))
    if end:
        w.code(*lit[256])


def stored_block(w, data, final, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    w.out += data


CL_LENS = [4] * 13 + [5] * 6       # a complete code-length code over all 19 symbols


def dynamic_block(w, lit_lens, dist_lens, tokens, final, sequence=None, end=True):
    """A dynamic block whose header spells the lengths out one by one, or as ``sequence``: (code-length symbol, extra
    value) pairs, taken as they are."""
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(15, 4)
    for s in CL_ORDER:
        w.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    if sequence is None:
        sequence = [(n, 0) for n in list(lit_lens) + list(dist_lens)]
    for s, extra in sequence:
        w.code(*cl[s])
        w.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    lit = canonical(lit_lens)
    put_tokens(w, tokens, lit, canonical(dist_lens))
    if end and 256 in lit:
        w.code(*lit[256])


def zwrap(deflate, data, cinfo=7, flg=None, cmf=None):
    cmf = (cinfo << 4) | 8 if cmf is None else cmf
    if flg is None:
        flg = 0x80
        flg += 31 - (cmf * 256 + flg) % 31
    return bytes([cmf, flg]) + deflate + (zlib.adler32(data) & 0xFFFFFFFF).to_bytes(4, "big")


# ---- a deflate reader: what a stream contains --------------------------------------------------------------------------
def _table(lens):
    top = max(lens) if lens and max(lens) else 0
    table = {}
    for s, (code, n) in canonical(lens).items():
        table[(n, code)] = s
    return table, top


def _decode(data, pos, table, top):
    code = 0
    for n in range(1, top + 1):
        code = (code << 1) | ((data[pos >> 3] >> (pos & 7)) & 1)
        pos += 1
        if (n, code) in table:
            return table[(n, code)], pos, n
    raise ValueError("no such code")


def walk(stream):
    """``(inflated bytes, facts)`` of a valid zlib stream; ``facts``: block types, the longest code used, code-length
    symbols, lengths and distances met, whether a repeat crossed the literal / distance border, whether a block had no
    distance code."""
    data = bytes(stream) + bytes(8)
    facts = {"types": set(), "longest": 0, "cl": set(), "lengths": set(), "distances": set(), "crossing": False, "no_distance_code": False}
    pos = 16
    out = bytearray()

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((data[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v
    last = 0
    while not last:
        last, kind = bits(1), bits(2)
        facts["types"].add(kind)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == (~n & 0xFFFF)
            out += data[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            continue
        if kind == 1:
            lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
        else:
            hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
            cl_lens = [0] * 19
            for s in CL_ORDER[:hclen]:
                cl_lens[s] = bits(3)
            cl, top = _table(cl_lens)
            lens = []
            while len(lens) < hlit + hdist:
                s, pos, _ = _decode(data, pos, cl, top)
                if s < 16:
                    lens.append(s)
                    continue
                facts["cl"].add(s)
                rep = 3 + bits(2) if s == 16 else (3 + bits(3) if s == 17 else 11 + bits(7))
                if len(lens) < hlit < len(lens) + rep:
                    facts["crossing"] = True
                lens += [lens[-1] if s == 16 else 0] * rep
            assert len(lens) == hlit + hdist
            lit_lens, dist_lens = lens[:hlit], lens[hlit:]
            if not any(dist_lens):
                facts["no_distance_code"] = True
        lit, lit_top = _table(lit_lens)
        dist, dist_top = _table(dist_lens)
        while True:
            s, pos, n = _decode(data, pos, lit, lit_top)
            facts["longest"] = max(facts["longest"], n)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                length = LENGTH_BASE[s - 257] + bits(LENGTH_EXTRA[s - 257])
                d, pos, n = _decode(data, pos, dist, dist_top)
                facts["longest"] = max(facts["longest"], n)
                distance = DIST_BASE[d] + bits(DIST_EXTRA[d])
                facts["lengths"].add(length)
                facts["distances"].add(distance)
                for _ in range(length):
                    out.append(out[-distance])
    return bytes(out), facts


# ---- content ------------------------------------------------------------------------------------------------------------
def _rows(body, rb, types=None):
    """``body`` (uint8, any length) as rows of ``rb`` bytes under filter bytes ``types`` (0 where None): the filtered stream
    as inflate returns it, and H."""
    body = np.asarray(body, np.uint8).reshape(-1)
    H = max(1, -(-len(body) // rb))
    rows = np.zeros((H, 1 + rb), np.uint8)
    padded = np.zeros(H * rb, np.uint8)
    padded[:len(body)] = body
    rows[:, 1:] = padded.reshape(H, rb)
    if types is not None:
        rows[:, 0] = [types[y % len(types)] for y in range(H)]
    return rows.tobytes(), H


def _smooth(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    px = np.stack([128 + 100 * np.sin(yy / 9.0 + c) * np.cos(xx / 6.0) for c in range(3)], -1).astype(np.uint8)
    return px.reshape(H, 3 * W)


def _filtered_rgb(raw, types):
    H = raw.shape[0]
    return pdc.filtered_stream(raw, 3, [types[y % len(types)] for y in range(H)])


def _compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def accepted_cases():
    """``[(name, stream, H, row_bytes)]``."""
    rng = np.random.default_rng(20261020)
    out = []
    smooth = _filtered_rgb(_smooth(50, 40), [0, 1, 2, 3, 4])                        # 50 rows of 1 + 120
    noise = _filtered_rgb(rng.integers(0, 256, (50, 120), dtype=np.uint8), [0, 1, 2, 3, 4])
    for label, data in (("smooth", smooth), ("noise", noise)):
        for level in (0, 1, 6, 9):
            out.append(("%s_level%d" % (label, level), _compress(data, level), 50, 120))
        for sname, strategy in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
            out.append(("%s_%s" % (label, sname), _compress(data, 6, strategy), 50, 120))
        out.append(("%s_wbits9" % label, _compress(data, 6, wbits=9), 50, 120))
    c = zlib.compressobj(6)
    cut = c.compress(smooth[:1500]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(smooth[1500:3000]) + c.flush(zlib.Z_FULL_FLUSH)
    cut += c.flush(zlib.Z_SYNC_FLUSH) + c.compress(smooth[3000:]) + c.flush()
    out.append(("flushes", cut, 50, 120))
    big = _filtered_rgb(np.concatenate([_smooth(60, 200), rng.integers(0, 256, (60, 600), dtype=np.uint8)]), [4, 1, 2, 0, 3])
    out.append(("rgb_200x120_level6", _compress(big, 6), 120, 600))
    out.append(("one_pixel", _compress(bytes([0, 9, 8, 7]), 6), 1, 3))
    # code lengths 1, 2, ... 14, 15, 15 (the literals 0..14 and the end-of-block code): what Fibonacci frequencies would give
    body, _ = _rows(np.concatenate([rng.integers(0, 15, 2 * (ROW - 1) - 15), np.arange(15)]).astype(np.uint8), ROW - 1)
    w = Bits()
    dynamic_block(w, list(range(1, 16)) + [0] * 241 + [15], [0], list(body), 1)
    out.append(("code_of_15_bits", zwrap(w.bytes(), body), 2, ROW - 1))
    # length 3 and length 258 at distance 1: three rows of zeros
    w = Bits()
    fixed_block(w, [0, (3, 1), (258, 1), (3 * ROW - 262, 1)], 1)
    out.append(("length_3_and_258_at_distance_1", zwrap(w.bytes(), bytes(3 * ROW)), 3, ROW - 1))
    # distance 32768 behind a stored block of 32768 bytes: rows 256 and 257 repeat rows 0 and 1
    first, _ = _rows(rng.integers(0, 256, 256 * (ROW - 1), dtype=np.uint8), ROW - 1)
    w = Bits()
    stored_block(w, first, 0)
    fixed_block(w, [(256, 32768)], 1)
    out.append(("distance_32768", zwrap(w.bytes(), first + first[:256]), 258, ROW - 1))
    # a dynamic block without any distance code; its header repeats zeros across the literal / distance border (17),
    # repeats a length (16) and a long run of zeros (18)
    body, _ = _rows(rng.integers(0, 64, 2 * (ROW - 1), dtype=np.uint8), ROW - 1)
    lit_lens = [6] * 63 + [7] + [0] * 192 + [7] + [0] * 3                        # 0..62: 6 bits; 63 and 256: 7 bits; 257..259: none
    assert sum(2.0 ** -n for n in lit_lens if n) == 1.0 and len(lit_lens) == 260
    sequence = [(6, 0)] + [(16, 3)] * 10 + [(6, 0), (6, 0), (7, 0), (18, 127), (18, 43), (7, 0), (17, 1)]
    w = Bits()
    dynamic_block(w, lit_lens, [0], list(body), 1, sequence=sequence)
    out.append(("no_distance_code", zwrap(w.bytes(), body), 2, ROW - 1))
    return out


def project_case():
    """One stream of ``ssd_png_encode_host`` (a single distance code of one bit): needs the library."""
    import png_cases as pc
    px = np.ascontiguousarray(pdc._pictures()["smooth"][..., :3])
    rc, blob = pc.host_encode(px, 5)[:2]
    assert rc == 0
    blob = bytes(blob)
    stream, at = b"", 8
    while at < len(blob):
        n = int.from_bytes(blob[at:at + 4], "big")
        if blob[at + 4:at + 8] == b"IDAT":
            stream += blob[at + 8:at + 8 + n]
        at += 12 + n
    return ("project_encoder", stream, 50, 120)


def all_accepted():
    return list(accepted_cases()) + [project_case()]


@functools.lru_cache(maxsize=None)
def coverage():
    """What the accepted set (without the library's own stream) contains; asserts every inflated stream against zlib."""
    total = {"types": set(), "longest": 0, "cl": set(), "lengths": set(), "distances": set(), "crossing": False, "no_distance_code": False}
    for name, stream, H, rb in accepted_cases():
        data, facts = walk(stream)
        assert data == zlib.decompress(stream) and len(data) == H * (1 + rb), name
        assert max(data[::1 + rb]) <= 4, name
        for k, v in facts.items():
            total[k] = total[k] | v if isinstance(v, (set, bool)) else max(total[k], v)
    assert total["types"] == {0, 1, 2}, total
    assert total["longest"] == 15, total
    assert total["cl"] == {16, 17, 18}, total
    assert total["crossing"] and total["no_distance_code"], total
    assert {3, 258} <= total["lengths"] and {1, 32768} <= total["distances"], total
    return total


@functools.lru_cache(maxsize=None)
def refusal_cases():
    """``[(name, stream, H, row_bytes, the status bit's name)]``: one per cause the inflater documents."""
    rng = np.random.default_rng(11)
    data, _ = _rows(rng.integers(0, 256, 2 * (ROW - 1), dtype=np.uint8), ROW - 1)
    good = zlib.compress(data, 6)
    rb = ROW - 1
    out = []

    def fixed(name, tokens, bit, end=True):
        w = Bits()
        fixed_block(w, tokens, 1, end=end)
        out.append((name, zwrap(w.bytes() + bytes(8), data), 2, rb, bit))

    def dynamic(name, lit_lens, sequence, bit):
        w = Bits()
        dynamic_block(w, lit_lens, [0], [], 1, sequence=sequence, end=False)
        out.append((name, zwrap(w.bytes() + bytes(8), data), 2, rb, bit))
    fixed("distance_beyond_output", [0, (3, 2)], "distance")
    fixed("distance_symbol_30", [0, ("lit", 257), ("dist", 30)], "symbol")
    fixed("length_symbol_286", [0, ("lit", 286)], "symbol")
    w = Bits()
    w.put(1, 1)
    w.put(3, 2)
    out.append(("block_type_3", zwrap(w.bytes() + bytes(8), data), 2, rb, "block_type"))
    w = Bits()
    stored_block(w, data, 1, nlen=len(data))
    out.append(("stored_len_nlen", zwrap(w.bytes(), data), 2, rb, "stored"))
    out.append(("wrong_adler", good[:-1] + bytes([good[-1] ^ 1]), 2, rb, "adler"))
    flg = 0x20
    flg += 31 - (0x78 * 256 + flg) % 31
    out.append(("fdict", bytes([0x78, flg]) + good[2:], 2, rb, "header"))
    out.append(("bad_fcheck", good[:1] + bytes([good[1] ^ 1]) + good[2:], 2, rb, "header"))
    out.append(("cinfo_8", bytes([0x88, 31 - (0x88 * 256) % 31]) + good[2:], 2, rb, "header"))
    w = Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.put(30, 5)
    w.put(0, 5)
    w.put(15, 4)
    out.append(("hlit_30", zwrap(w.bytes() + bytes(16), data), 2, rb, "symbols"))
    out.append(("one_trailing_byte", good + b"\0", 2, rb, "trailing"))
    out.append(("cut_before_trailer", good[:-4], 2, rb, "input"))
    out.append(("output_one_long", zlib.compress(data + b"\0", 6), 2, rb, "output"))
    out.append(("output_one_short", zlib.compress(data[:-1], 6), 2, rb, "output"))
    five = bytearray(data)
    five[ROW] = 5
    out.append(("filter_byte_5", zlib.compress(bytes(five), 6), 2, rb, "filter"))
    complete = [8] * 255 + [9, 9]
    spelled = [(n, 0) for n in complete + [0]]
    dynamic("repeat_with_nothing_before", complete, [(16, 0)] + spelled, "repeat")
    dynamic("repeat_past_the_lengths", complete, spelled[:-1] + [(18, 127)], "repeat")
    dynamic("oversubscribed", [8] * 257, [(8, 0)] * 257 + [(0, 0)], "oversubscribed")
    dynamic("incomplete", [8] * 255 + [0, 9], [(8, 0)] * 255 + [(0, 0), (9, 0), (0, 0)], "incomplete")
    dynamic("no_end_of_block", [8] * 256 + [0], [(8, 0)] * 256 + [(0, 0), (0, 0)], "no_end")
    return out


def as_png(stream, H, rb):
    """A grey 8-bit file of ``rb`` x ``H`` pixels around ``stream``."""
    return pdc.write_png(rb, H, 0, 8, None, None, stream=stream)


def zlib_accepts(stream, H, rb):
    """The host road's rule (``data_utils._png_inflate``) on a bare stream."""
    n = H * (1 + rb)
    z = zlib.decompressobj()
    try:
        data = z.decompress(stream, n + 1)
    except zlib.error:
        return False
    return len(data) == n and z.eof and not z.unused_data and not z.unconsumed_tail and max(data[::1 + rb]) <= 4
