"""The geometry cases of the general dense conv op (include/ssd_hip.h ``ssd_conv_desc``), shared by
tests/test_conv_geometry_cpu.py and tests/test_conv_geometry_gpu.py: non-square maps, ``kh != kw``, four different pads,
stride and dilation, so that a kernel which mixes up the two axes anywhere -- pixel decode, tap decode, row pitch, pads,
dilation -- gives a wrong answer on at least one of them (the mutant table of the CPU test shows which).

Inputs: ``clip(3 N(0,1), 0, 6)`` as float32 -- ReLU6-like, with exact zeros and sixes, inside the range contract of the
two-plane fp16 tiles; weights ``N(0,1) / sqrt(kh kw Cin)``.  Seeds are fixed integers.  Every M = B Ho Wo is <= 168.

``REFUSALS`` is the contract of the validity predicates: the (case, family) pairs that must answer SSD_E_UNSUPPORTED (-3)
with "cannot run" in ``ssd_last_error()``.  Every other pair must run, on every config of the family."""
import collections

import numpy as np

from oracle import conv_oracle as cv

Case = collections.namedtuple("Case", "name seed B H W Cin Cout kh kw stride dil pads")

CASES = [
    #    name         seed   B   H   W  Cin Cout kh kw  s  d  pads (t, b, l, r)
    Case("wide_same",   101, 2,  7, 12,  64,  84, 3, 3, 1, 1, (1, 1, 1, 1)),
    Case("tall_s2",     102, 2, 13,  6,  64, 100, 3, 3, 2, 1, (1, 1, 0, 1)),
    Case("k1x3",        103, 3,  9,  5, 128,  48, 1, 3, 1, 1, (0, 0, 1, 1)),
    Case("k3x1",        104, 3,  5,  9, 128,  48, 3, 1, 1, 1, (1, 1, 0, 0)),
    Case("dil2",        105, 1, 11,  8,  64,  64, 3, 3, 1, 2, (2, 2, 2, 2)),
    Case("dil6",        106, 1, 14,  9,  64,  32, 3, 3, 1, 6, (6, 6, 6, 6)),
    Case("four_pads",   107, 2,  6, 10,  64,  40, 3, 3, 1, 1, (2, 0, 0, 1)),   # output rows whose first tap row is all padding
    Case("k1_s2",       108, 2,  8,  5,  64,  96, 1, 1, 2, 1, (0, 0, 0, 0)),   # 1x1, not the GEMM shortcut
    Case("k1_padb",     109, 2,  4,  7,  64,  32, 1, 1, 1, 1, (0, 1, 0, 0)),   # 1x1, last output row = shift alone
    Case("k5x5",        110, 2,  6,  4,  64,  24, 5, 5, 1, 1, (2, 2, 2, 2)),   # 25 taps: inside the 32-bit tap mask
    Case("k6x6",        111, 1,  5,  7,  16,  20, 6, 6, 1, 1, (2, 3, 2, 3)),   # 36 taps: outside it
    Case("tiny_maps",   112, 5,  2,  3, 256,  84, 3, 3, 1, 1, (1, 1, 1, 1)),   # a tile spans several images
    Case("s3_valid",    113, 2, 10,  7,  64,  32, 3, 3, 3, 1, (0, 0, 0, 0)),
    Case("s2_dil2",     114, 2,  9, 12,  64,  48, 3, 3, 2, 2, (2, 2, 1, 2)),
    Case("rgb_stem",    115, 2,  9, 14,   3,  32, 3, 3, 2, 1, (1, 1, 0, 1)),
    Case("cin8_direct", 116, 2,  5,  8,   8,  24, 3, 3, 2, 1, (1, 1, 0, 1)),
]
BY_NAME = {c.name: c for c in CASES}

# config name prefix -> family ("auto" is config -1, the cost model's pick)
FAMILIES = ("auto", "mfma", "skinny", "mfma3", "bf16", "dma3", "dmab", "dmah", "wino", "direct")
PREFIX = {"mfma_": "mfma", "skinny_": "skinny", "mfma3_": "mfma3", "bf16_": "bf16", "dma3_": "dma3", "dmab_": "dmab",
          "dmah_": "dmah", "wino_": "wino", "direct_valu": "direct"}
TILE_FAMILIES = ("mfma", "skinny", "mfma3", "bf16", "dma3", "dmab", "dmah")

_ALL_TILES = frozenset(TILE_FAMILIES)
_NO_DIRECT = frozenset(("direct",))
_NO_WINO = frozenset(("wino",))

# (case, family) pairs that must refuse.  From the documented constraints:
#   * the MFMA tile families need Cin % 64 == 0 here (the widest k-step of any of them) and at most 32 taps;
#   * skinny_* also needs K >= 256;
#   * direct_valu keeps the whole weight matrix in LDS: K round_up(Cout, 4) 4 <= 65536 bytes;
#   * Winograd: 3x3, stride 1, dilation 1, Cin % 16 == 0;
#   * config -1 always finds a kernel here.
REFUSALS = {
    "wide_same":   _NO_DIRECT,
    "tall_s2":     _NO_DIRECT | _NO_WINO,
    "k1x3":        _NO_DIRECT | _NO_WINO,
    "k3x1":        _NO_DIRECT | _NO_WINO,
    "dil2":        _NO_DIRECT | _NO_WINO,
    "dil6":        _NO_DIRECT | _NO_WINO,
    "four_pads":   _NO_DIRECT,
    "k1_s2":       frozenset(("skinny",)) | _NO_WINO,
    "k1_padb":     frozenset(("skinny",)) | _NO_WINO,
    "k5x5":        _NO_DIRECT | _NO_WINO,
    "k6x6":        _ALL_TILES | _NO_WINO,
    "tiny_maps":   _NO_DIRECT,
    "s3_valid":    _NO_DIRECT | _NO_WINO,
    "s2_dil2":     _NO_DIRECT | _NO_WINO,
    "rgb_stem":    _ALL_TILES | _NO_WINO,
    "cin8_direct": _ALL_TILES | _NO_WINO,
}


def must_refuse(case, family):
    return family in REFUSALS[case.name]


def refusals_from_rules(c):
    """The same table derived from the rules above (the CPU test holds the literal table to it)."""
    K, taps = c.kh * c.kw * c.Cin, c.kh * c.kw
    out = set()
    if c.Cin % 64 or taps > 32:
        out |= set(TILE_FAMILIES)
    if K < 256:
        out.add("skinny")
    if K * ((c.Cout + 3) // 4 * 4) * 4 > 65536:
        out.add("direct")
    if not (c.kh == 3 and c.kw == 3 and c.stride == 1 and c.dil == 1 and c.Cin % 16 == 0):
        out.add("wino")
    return frozenset(out)


def out_hw(c):
    return (cv.out_size(c.H, c.kh, c.stride, c.dil, c.pads[0], c.pads[1]),
            cv.out_size(c.W, c.kw, c.stride, c.dil, c.pads[2], c.pads[3]))


_DATA = {}


def data(c):
    """Inputs and float64 references of a case, computed once, shared and never changed (arrays are read-only):
    x, w, scale, shift, res (fp32); conv (the bare float64 convolution), ref (ReLU6(conv scale + shift) + res),
    ref_nores (the same without the residual)."""
    if c.name not in _DATA:
        rng = np.random.default_rng(c.seed)
        x = np.clip(3.0 * rng.standard_normal((c.B, c.H, c.W, c.Cin)), 0.0, 6.0).astype(np.float32)
        w = (rng.standard_normal((c.kh, c.kw, c.Cin, c.Cout)) / np.sqrt(c.kh * c.kw * c.Cin)).astype(np.float32)
        scale = rng.uniform(0.5, 1.5, c.Cout).astype(np.float32)
        shift = rng.uniform(-0.5, 0.5, c.Cout).astype(np.float32)
        conv = cv.conv2d_f64(x, w, c.stride, c.dil, c.pads)
        res = rng.standard_normal(conv.shape).astype(np.float32)
        d = dict(x=x, w=w, scale=scale, shift=shift, res=res, conv=conv,
                 ref=cv.epilogue_f64(conv, scale, shift, cv.ACT_RELU6, res),
                 ref_nores=cv.epilogue_f64(conv, scale, shift, cv.ACT_RELU6))
        for v in d.values():
            v.setflags(write=False)
        _DATA[c.name] = d
    return _DATA[c.name]
