"""The two-plane fp16 conv tiles ``dmah_*`` (csrc/ssd_convdma.hip, csrc/ssd_bf16x3.h) through the C ABI:
``ssd_split_planes`` / ``ssd_join_planes`` with planes = 2, ``ssd_conv_pack_weights_f16x2``, ``ssd_conv2d_planes_f16x2``.

* split -> join within the representation bound 2^-22 |x| + 2^-33; values beyond fp16's range come back non-finite;
* every ``dmah_*`` tile, both k-step forms, against the NumPy conv oracle inside the fp32 contract (1e-4), the plane
  output equal to the split of the fp32 output;
* accuracy against float64 within 1.5x of the ``dma3_*`` tile of the same shape (+ 1e-7), also on inputs scaled by 1e-4;
* split-K, the refusals, the per-layer weight scale."""
import ctypes

import numpy as np
import pytest
import torch

import f16x2_cases as fc
from oracle import net_oracle as no
from test_conv_gpu import run_conv, same, _np, _close, guarded
from test_convdma_gpu import POISON, make_planes, join_planes, run_conv_planes, dma_configs

pytestmark = pytest.mark.gpu


def pack_weights(w):
    """HWIO fp32 -> (packed fp32 device buffer, fp16 plane device buffer, k)."""
    import ssd_hip as h
    lib = h.lib()
    kh, kw, Cin, Cout = w.shape
    wd = h.to_dev(w)
    npk = lib.ssd_conv_packed_weight_floats(kh, kw, Cin, Cout)
    packed = torch.full((npk + 4096,), float("nan"), dtype=torch.float32, device=wd.device)[:npk]
    h.check(lib.ssd_conv_pack_weights(h.ptr(wd), kh, kw, Cin, Cout, h.ptr(packed), h.stream()), "pack")
    nb = lib.ssd_conv_f16x2_weight_bytes(kh, kw, Cin, Cout)
    wpl = torch.full((nb // 2 + 64,), 0x7fc0, dtype=torch.int16, device=wd.device)
    k = ctypes.c_int(-999)
    rc = lib.ssd_conv_pack_weights_f16x2(h.ptr(packed), kh, kw, Cin, Cout, h.vp(wpl.data_ptr()), ctypes.byref(k), h.stream())
    return rc, packed, wpl, k.value


def run_conv_h(x, w, cfg, scale=None, shift=None, res=None, stride=1, dil=1, pads=(0, 0, 0, 0), act=0, split_k=1, in_planes=2,
               packed_w=None, want_planes=True, out_strides=None, canvas=None):
    """``ssd_conv2d_planes_f16x2`` on the planes of x; returns (rc, out, joined plane output or None).  ``out_strides`` /
    ``canvas``: a strided destination inside a flat buffer, as in ``run_conv``."""
    import ssd_hip as h
    lib = h.lib()
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    d = h.ConvDesc(B, H, W, Cin, Cout, kh, kw, stride, dil, pads[0], pads[2], pads[1], pads[3], act, int(res is not None))
    rc, packed, wpl, k = packed_w if packed_w is not None else pack_weights(w)
    assert rc == 0, lib.ssd_last_error()
    Ho = lib.ssd_conv_out_size(H, kh, stride, dil, pads[0], pads[1])
    Wo = lib.ssd_conv_out_size(W, kw, stride, dil, pads[2], pads[3])
    if Cin % 32:
        keep = torch.zeros((4 * x.size + 64,), dtype=torch.int16, device=packed.device)
        p0, pstride = keep.data_ptr(), (x.size + 63) // 64 * 64
    else:
        keep, p0, pstride = make_planes(x, in_planes)
    sd = guarded(scale) if scale is not None else None
    hd = guarded(shift) if shift is not None else None
    rd = guarded(res) if res is not None else None
    bs = ps = 0
    if out_strides is None:
        out = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float32, device=packed.device)
        optr = h.ptr(out)
    else:
        bs, ps, off, total = out_strides
        out = canvas if canvas is not None else torch.full((total,), float("nan"), dtype=torch.float32, device=packed.device)
        assert out.numel() == total
        optr = h.vp(out.data_ptr() + 4 * off)
    n_out = B * Ho * Wo * Cout
    op, ostride = None, 0
    if want_planes and Cout % 32 == 0:
        ostride = (n_out + 63) // 64 * 64
        op = torch.full((2 * ostride + 64,), 0x7fc0, dtype=torch.int16, device=packed.device)
    ws = torch.empty(max(1, split_k * n_out), dtype=torch.float32, device=packed.device) if split_k > 1 else None
    rc = lib.ssd_conv2d_planes_f16x2(ctypes.byref(d), h.vp(p0), pstride, h.ptr(packed), h.vp(wpl.data_ptr()), k, h.ptr(sd), h.ptr(hd),
                                     h.ptr(rd), optr, bs, ps, h.ptr(op), ostride, cfg, split_k, h.ptr(ws), h.stream())
    joined = None
    if rc == 0 and op is not None:
        joined = join_planes(op.data_ptr(), n_out, Cout, 2, ostride).reshape(B, Ho, Wo, Cout)
    return rc, out, joined


def expect_plane_output(joined, o):
    """The plane output is the split of the fp32 output beside it (non-finite where the output leaves fp16's range)."""
    want = fc.join_act(*fc.split_act(o))
    np.testing.assert_array_equal(joined.view(np.uint32), want.view(np.uint32))


def test_split_join_planes_within_the_bound():
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 6.0, 8192).astype(np.float32)                   # 128 pixels x 64 channels
    x[:8] = np.float32([0.0, -0.0, 6.0, 255.0, 1e-3, 1e-6, 2.0 ** -20, 2.0 ** -30])
    x[8:12] = np.float32([256.0, 1e4, -300.0, 3e38])                     # beyond fp16 / 256
    buf, p0, stride = make_planes(x.reshape(128, 64), 2)
    back = join_planes(p0, x.size, 64, 2, stride)
    assert not np.isfinite(back[8:12]).any()
    ok = np.ones(x.size, bool)
    ok[8:12] = False
    err = np.abs(back[ok].astype(np.float64) - x[ok].astype(np.float64))
    assert (err <= fc.REL * np.abs(x[ok].astype(np.float64)) + fc.ABS).all(), err.max()
    np.testing.assert_array_equal(back[ok].view(np.uint32), fc.join_act(*fc.split_act(x[ok])).view(np.uint32))
    allb = _np(buf)          # the poison around the two planes is untouched
    assert (allb[:POISON] == 0x7fc0).all() and (allb[POISON + x.size:POISON + stride] == 0x7fc0).all()
    assert (allb[POISON + stride + x.size:POISON + 2 * stride] == 0x7fc0).all() and (allb[POISON + 2 * stride:] == 0x7fc0).all()
    # slice-major, plane h: pixel 5, channel 40 at (1 * 128 + 5) * 32 + 8
    h_plane = allb[POISON:POISON + x.size].view(np.float16)
    assert h_plane[(128 + 5) * 32 + 8] == np.float16(np.float32(256.0) * x.reshape(128, 64)[5, 40])


DMAH_CASES = [
    # (B, H, Cin, Cout, k, stride, dil)
    (2, 19, 576, 100, 3, 1, 1),      # ragged Cout: the head tile
    (3, 10, 320, 1280, 1, 1, 1),     # 1x1 path
    (2, 10, 256, 512, 3, 2, 1),      # stride 2 SAME, pads (0, 1)
    (70, 2, 256, 84, 3, 1, 1),       # a tile spanning many images
    (1, 38, 64, 128, 3, 1, 1),       # ragged M
    (1, 19, 64, 64, 3, 1, 6),        # dilation
    (1, 12, 96, 64, 3, 1, 1),        # three k-steps: ragged last tile at two k-steps per barrier
]


@pytest.mark.parametrize("case", DMAH_CASES)
def test_conv2d_dmah_all_configs(case):
    import ssd_hip as h
    lib = h.lib()
    B, H, Cin, Cout, k, stride, dil = case
    rng = np.random.default_rng(hash(case[:5]) % 1000)
    x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
    pads = same(H, k, stride, dil) * 2 if k > 1 else (0, 0, 0, 0)
    ref = no.relu6(no.conv2d(x, w, None, stride, dil, "same" if k > 1 else "valid") * scale + shift)
    res = rng.standard_normal(ref.shape).astype(np.float32)
    pw = pack_weights(w)
    forms = {1: 0, 2: 0}
    for cfg, name in dma_configs(b"dmah_"):
        rc, out, joined = run_conv_h(x, w, cfg, scale, shift, res, stride, dil, pads, act=2, packed_w=pw)
        assert rc == 0, (name, lib.ssd_last_error())
        o = _np(out)
        _close(o, ref + res, 1e-4)
        if joined is not None:
            expect_plane_output(joined, o)
        forms[2 if name.endswith("_ks2") else 1] += 1
    assert forms[1] >= 8 and forms[2] >= 4, forms


def _f64_conv3x3(x, w):
    B, H, _, Cin = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    ref = np.zeros((B, H, H, w.shape[3]))
    for ky in range(3):
        for kx in range(3):
            ref += xp[:, ky:ky + H, kx:kx + H, :] @ w[ky, kx].astype(np.float64)
    return ref


def test_dmah_tiles_are_as_accurate_as_the_dma3_tiles():
    """K = 4608 (the shape of test_split_bf16_tiles_are_as_accurate_as_the_fp32_mfma): the error of every ``dmah_*`` tile
    against float64 is within 1.5x (+ 1e-7) of the ``dma3_*`` tile of the same shape on the same inputs -- the margin that
    test gives the split-bf16 tiles against the fp32 MFMA.  The second input is scaled by 1e-4 (errors relative to the output
    scale): its low plane lies in fp16's subnormal range."""
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(31)
    B, H, Cin, Cout = 2, 19, 512, 128
    x0 = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    pw = pack_weights(w)
    dma3 = {n[len("dma3_"):]: c for c, n in dma_configs(b"dma3_")}
    for x in (x0, (x0 * np.float32(1e-4)).astype(np.float32)):
        ref = _f64_conv3x3(x, w)
        unit = 1.0 if x is x0 else float(np.abs(ref).max())          # first input: absolute errors, as that test
        e3 = {}
        for cfg, name in dma_configs(b"dmah_"):
            tile = name[len("dmah_"):].replace("_ks2", "")
            if tile not in e3:
                rc, out, _ = run_conv_planes(x, w, 3, dma3[tile], pads=(1, 1, 1, 1), want_planes=False)
                assert rc == 0, lib.ssd_last_error()
                e3[tile] = float(np.abs(_np(out).astype(np.float64) - ref).max()) / unit
            rc, out, _ = run_conv_h(x, w, cfg, pads=(1, 1, 1, 1), packed_w=pw)
            assert rc == 0, (name, lib.ssd_last_error())
            eh = float(np.abs(_np(out).astype(np.float64) - ref).max()) / unit
            print("%-22s err %.3e  (dma3 twin %.3e, unit %.3g)" % (name, eh, e3[tile], unit))
            assert eh <= 1.5 * e3[tile] + 1e-7, (name, eh, e3[tile])


def test_dmah_split_k_agrees_and_writes_planes():
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(8)
    x = rng.uniform(0.0, 6.0, (2, 10, 10, 256)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 256, 64)) / 48.0).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, 64).astype(np.float32)
    ref = no.relu6(no.conv2d(x, w, None, 1, 1, "same") + shift)
    pw = pack_weights(w)
    names = dict((n, c) for c, n in dma_configs(b"dmah_"))
    for name in ("dmah_2x2_2x2", "dmah_2x2_2x2_ks2"):
        rc, o1, _ = run_conv_h(x, w, names[name], None, shift, None, 1, 1, (1, 1, 1, 1), act=2, packed_w=pw)
        assert rc == 0, lib.ssd_last_error()
        for sk in (2, 3):
            rc, out, joined = run_conv_h(x, w, names[name], None, shift, None, 1, 1, (1, 1, 1, 1), act=2, split_k=sk, packed_w=pw)
            assert rc == 0, (name, sk, lib.ssd_last_error())
            _close(_np(out), ref, 1e-4)
            _close(_np(out), _np(o1), 1e-4)
            expect_plane_output(joined, _np(out))


def test_dmah_refusals():
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(0)
    cfgh = dict((n, c) for c, n in dma_configs(b"dmah_"))["dmah_2x2_2x2"]
    cfg3 = dict((n, c) for c, n in dma_configs(b"dma3_"))["dma3_2x2_2x2"]
    x = rng.standard_normal((1, 8, 8, 32)).astype(np.float32)
    w = rng.standard_normal((3, 3, 32, 32)).astype(np.float32)
    for np_ in (3, 1):          # bf16 planes handed to a dmah tile
        rc, _, _ = run_conv_planes(x, w, np_, cfgh, pads=(1, 1, 1, 1))
        assert rc == -3 and b"cannot run" in lib.ssd_last_error(), (np_, rc, lib.ssd_last_error())
    rc, _, _ = run_conv_h(x, w, cfg3, pads=(1, 1, 1, 1))                  # ... and the fp16 pair to a three-plane tile
    assert rc == -3 and b"cannot run" in lib.ssd_last_error()
    rc, _ = run_conv(x, w, pads=(1, 1, 1, 1), cfg=cfgh)                  # the fp32 entry point: no planes
    assert rc == -3 and b"cannot run" in lib.ssd_last_error()
    x = rng.standard_normal((1, 8, 8, 24)).astype(np.float32)            # Cin % 32 != 0
    w = rng.standard_normal((3, 3, 24, 32)).astype(np.float32)
    rc, _, _ = run_conv_h(x, w, cfgh, pads=(1, 1, 1, 1))
    assert rc == -3 and b"cannot run" in lib.ssd_last_error()
    w[0, 0, 0, 0] = np.inf                                               # a non-finite weight: no fp16 planes for the layer
    rc, _, _, _ = pack_weights(w)
    assert rc == -3 and b"non-finite" in lib.ssd_last_error()


def test_dmah_refused_in_a_bf16_net():
    """A table that names a ``dmah_*`` tile in a precision-1 net: finalize answers SSD_E_UNSUPPORTED."""
    import helpers
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    m = get_model(hp, max_batch=2, precision="bf16")
    m.set_weights(helpers.synthetic_weights("mobilenet_v2", hp))
    m.set_tuning("2_conv_heads dmah_2x2_2x2 1\n")
    with pytest.raises(Exception) as e:
        m._ensure(2)
    assert "precision 0" in str(e.value) and "dmah_2x2_2x2" in str(e.value), str(e.value)


@pytest.mark.parametrize("wmax", [0.0, 1e-6, 300.0])
def test_dmah_weight_scale(wmax):
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(4)
    x = rng.uniform(0.0, 6.0, (1, 9, 9, 64)).astype(np.float32)
    w = rng.uniform(-1.0, 1.0, (3, 3, 64, 48)).astype(np.float32)
    w *= np.float32(wmax) / np.abs(w).max()
    pw = pack_weights(w)
    rc, _, _, k = pw
    assert rc == 0, lib.ssd_last_error()
    if wmax == 0.0:
        assert k == 0
    else:
        assert 2.0 ** 13 <= float(np.abs(w).max()) * 2.0 ** k < 2.0 ** 14, k
    assert k == fc.weight_exp(w)
    ref = no.conv2d(x, w, None, 1, 1, "same")
    cfg = dict((n, c) for c, n in dma_configs(b"dmah_"))["dmah_2x2_2x2"]
    rc, out, _ = run_conv_h(x, w, cfg, pads=(1, 1, 1, 1), packed_w=pw)
    assert rc == 0, lib.ssd_last_error()
    unit = max(float(np.abs(ref).max()), 1e-30)
    assert np.abs(_np(out) - ref).max() <= 1e-4 * unit, (np.abs(_np(out) - ref).max(), unit)
    if wmax == 0.0:
        assert not _np(out).any()
