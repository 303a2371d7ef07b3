"""GPU parity tests for the conv family and the full SSD forward graphs: HIP kernels
(through the C ABI) vs the NumPy oracle (oracle/net_oracle.py) on the same seeded inputs.
Tolerance: 1e-4 abs on O(1) activations / final boxes+scores (BASELINE.json north_star);
per-op checks use a relative bound because fp32 MFMA accumulation order differs from BLAS."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
from oracle import net_oracle as no
from oracle import bbox_oracle as bo
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _close(a, b, tol=2e-4):
    # intermediate activations (values up to 6 after ReLU6, ~50 fp32 layers deep, MFMA vs BLAS
    # accumulation order): relative bound; the 1e-4 ABSOLUTE bar of the contract is asserted on
    # the network outputs (probabilities, boxes, scores) separately.
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, "max abs err %.3e (scale %.3g)" % (err, scale)


def _deltas(d, rd, variances=(0.1, 0.1, 0.2, 0.2)):
    """Whole-network pred_deltas: the same bar as tests/test_fullsize_gpu.py::_assert_deltas.  The raw
    regression outputs reach |d| ~ 4.5 with the seeded weights and carry the fp32 accumulation-order
    noise of ~50 layers (observed 0.9 - 1.1e-4 at the largest values, oracle noise included): 1e-4
    ABSOLUTE is asserted on d * variances -- what enters the boxes, models/decoder.py:41; boxes and
    scores themselves are held to 1e-4 abs in the end-to-end tests -- and 5e-5 of the tensor's range on
    the raw values."""
    err = np.abs(d - rd)
    assert (err * np.asarray(variances, np.float32)).max() <= 1e-4
    assert err.max() <= 5e-5 * max(2.0, float(np.abs(rd).max())), "deltas: max abs err %.3e (max |ref| %.3g)" % (
        err.max(), np.abs(rd).max())


def _abs(a, b, tol=1e-4):
    """The contract's bar on network outputs: 1e-4 ABSOLUTE (BASELINE.json north_star)."""
    err = float(np.abs(a - b).max())
    assert err <= tol, "max abs err %.3e (max |ref| %.3g)" % (err, float(np.abs(b).max()))


def guarded(a, pad=4096):
    """Device copy of `a` in the middle of a NaN-poisoned buffer (pad floats on either side,
    16-byte alignment kept): an out-of-range read shows up as NaN instead of depending on
    what the allocator happened to place next to the tensor."""
    import ssd_hip as h
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 2 * pad,), float("nan"), dtype=torch.float32, device=h.device())
    view = buf[pad:pad + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def run_conv(x, w, scale=None, shift=None, res=None, stride=1, dil=1, pads=(0, 0, 0, 0), act=0, cfg=-1,
             split_k=1, out_strides=None, canvas=None):
    """``out_strides`` = (batch stride, pixel stride, offset, total floats): the destination lies inside a flat buffer,
    NaN-filled here or handed in as ``canvas`` (a float32 device tensor of ``total`` floats) -- which is what comes back."""
    import ssd_hip as h
    lib = h.lib()
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    d = h.ConvDesc(B, H, W, Cin, Cout, kh, kw, stride, dil, pads[0], pads[2], pads[1], pads[3], act,
                   int(res is not None))
    xd, wd = guarded(x), h.to_dev(w)
    # the packed weights are followed by NaN poison: a kernel that reads past [Npad][Kpad]
    # (and multiplies by a zero-padded pixel) turns the output NaN
    npk = lib.ssd_conv_packed_weight_floats(kh, kw, Cin, Cout)
    poisoned = torch.full((npk + 4096,), float("nan"), dtype=torch.float32, device=xd.device)
    packed = poisoned[:npk]
    h.check(lib.ssd_conv_pack_weights(h.ptr(wd), kh, kw, Cin, Cout, h.ptr(packed), h.stream()), "pack")
    Ho = lib.ssd_conv_out_size(H, kh, stride, dil, pads[0], pads[1])
    Wo = lib.ssd_conv_out_size(W, kw, stride, dil, pads[2], pads[3])
    sd = guarded(scale) if scale is not None else None
    hd = guarded(shift) if shift is not None else None
    rd = guarded(res) if res is not None else None
    if out_strides is None:
        out = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float32, device=xd.device)
        bs = ps = 0
        optr = h.ptr(out)
    else:
        bs, ps, off, total = out_strides
        out = canvas if canvas is not None else torch.full((total,), float("nan"), dtype=torch.float32, device=xd.device)
        assert out.numel() == total
        optr = h.vp(out.data_ptr() + 4 * off)
    ws = torch.empty(max(1, split_k * B * Ho * Wo * Cout), dtype=torch.float32, device=xd.device) if split_k > 1 else None
    rc = lib.ssd_conv2d_ex(ctypes.byref(d), h.ptr(xd), h.ptr(packed), h.ptr(sd), h.ptr(hd), h.ptr(rd), optr,
                           bs, ps, cfg, split_k, h.ptr(ws), h.stream())
    return rc, out


def same(size, k, s, d=1):
    o, a, b = no.same_pads(size, k, s, d)
    return a, b


CONV_CASES = [
    # (B, H, Cin, Cout, k, stride, dil, padding)
    (2, 19, 96, 576, 1, 1, 1, "valid"),     # MBv2 expand
    (2, 38, 144, 32, 1, 1, 1, "valid"),     # project, Cin % 32 != 0 on the 1x1 path
    (3, 10, 24, 144, 1, 1, 1, "valid"),     # K = 24 (K tail inside one tile)
    (1, 75, 16, 96, 1, 1, 1, "valid"),      # K = 16
    (2, 10, 256, 512, 3, 2, 1, "same"),     # extra1_2: stride-2 SAME (0,1)
    (2, 5, 128, 256, 3, 2, 1, "same"),      # extra2_2: (1,1)
    (2, 19, 64, 84, 3, 1, 1, "same"),       # head-like, Cout not a tile multiple
    (1, 19, 64, 126, 3, 1, 1, "same"),      # Cout % 4 != 0 -> scalar stores
    (1, 19, 32, 64, 3, 1, 6, "same"),       # conv6-like dilation 6
    (2, 5, 128, 256, 3, 1, 1, "valid"),     # conv10_2-like VALID
    (2, 1, 256, 84, 3, 1, 1, "same"),       # 1x1 feature map head
    (1, 33, 3, 32, 3, 2, 1, (0, 1, 0, 1)),  # RGB stem, keras correct_pad even -> direct kernel
    (1, 20, 3, 64, 3, 1, 1, "same"),        # VGG stem
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_all_configs(case):
    import ssd_hip as h
    lib = h.lib()
    B, H, Cin, Cout, k, stride, dil, padding = case
    rng = np.random.default_rng(hash(case[:5]) % 1000)
    x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
    if padding == "same":
        pads = same(H, k, stride, dil) * 2
    elif padding == "valid":
        pads = (0, 0, 0, 0)
    else:
        pads = padding
    ref = no.conv2d(x, w, None, stride, dil, pads if padding not in ("same", "valid") else padding)
    ref = no.relu6(ref * scale + shift)
    res = rng.standard_normal(ref.shape).astype(np.float32)
    ran = 0
    for cfg in range(-1, lib.ssd_conv_num_configs()):
        if cfg >= 0 and lib.ssd_conv_config_name(cfg).startswith(b"bf16_"):
            continue            # the bf16 (one-product) tiles have their own tolerance: tests/test_bf16_gpu.py
        rc, out = run_conv(x, w, scale, shift, res, stride, dil, pads, act=2, cfg=cfg)
        if rc == -3 and cfg >= 0:
            continue            # this tile config cannot take the shape (documented constraint)
        assert rc == 0, (cfg, lib.ssd_last_error())
        _close(_np(out), ref + res, 1e-4)
        ran += 1
    assert ran >= 2


def test_split_bf16_tiles_are_as_accurate_as_the_fp32_mfma():
    """The `mfma3_*` tiles form every fp32 product from an exact three-way bf16 split of both operands (six bf16 MFMAs,
    csrc/ssd_bf16x3.h).  On a long-K conv (K = 4608: VGG16 conv4 / the heads) their error against a float64 reference
    stays within that of the fp32-MFMA tiles (both are fp32 roundings of the same sums), far inside the 1e-4 contract."""
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(31)
    B, H, Cin, Cout = 2, 19, 512, 128
    x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    ref = np.zeros((B, H, H, Cout))
    for ky in range(3):
        for kx in range(3):
            ref += xp[:, ky:ky + H, kx:kx + H, :] @ w[ky, kx].astype(np.float64)
    errs = {"mfma_": [], "mfma3_": []}
    for cfg in range(lib.ssd_conv_num_configs()):
        name = lib.ssd_conv_config_name(cfg)
        fam = b"mfma3_" if name.startswith(b"mfma3_") else (b"mfma_" if name.startswith(b"mfma_") else None)
        if fam is None:
            continue
        rc, out = run_conv(x, w, None, None, None, 1, 1, (1, 1, 1, 1), cfg=cfg)
        if rc == -3:
            continue
        assert rc == 0, lib.ssd_last_error()
        errs[fam.decode()].append(float(np.abs(_np(out).astype(np.float64) - ref).max()))
    assert len(errs["mfma3_"]) >= 8 and len(errs["mfma_"]) >= 8
    print("max |err| vs float64: fp32 MFMA tiles %.2e, split-bf16 tiles %.2e (max |ref| %.2f)" % (
        max(errs["mfma_"]), max(errs["mfma3_"]), float(np.abs(ref).max())))
    assert max(errs["mfma3_"]) <= 1.5 * max(errs["mfma_"]) + 1e-7 and max(errs["mfma3_"]) <= 3e-5        # measured: 1.11e-5 (split-bf16) vs 1.19e-5 (fp32 MFMA)


def test_split_bf16_tiles_nonfinite_and_tiny_inputs():
    """Edge semantics of the split-bf16 tiles (csrc/ssd_bf16x3.h) next to the fp32-MFMA tiles.
    (1) A non-finite activation: `split1` turns x = +-inf into (h = inf, m = l = NaN) where the fp32 MFMA propagates
    inf, so the two families may answer inf vs NaN -- the CONTRACT both keep is: every output whose receptive field
    holds the non-finite input is non-finite, every other output is finite and unchanged (nothing leaks, nothing is
    silently made finite).  (2) Magnitudes below ~2^-110: the l plane (x - h - m, 2^-16 below x) falls into the
    bf16 / fp32 denormal range and may be flushed, so a split product keeps >= 16 significand bits instead of 24: the
    error stays <= 2^-15 RELATIVE to the output scale, i.e. ~1e-35 absolute -- irrelevant to the 1e-4 contract."""
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(5)
    B, H, Cin, Cout = 1, 12, 64, 64
    x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    ref = no.conv2d(x, w, None, 1, 1, "same")
    xbad = x.copy()
    xbad[0, 3, 4, 7] = np.inf
    xbad[0, 9, 2, 33] = np.nan
    xbad[0, 6, 10, 0] = -np.inf
    touched = np.zeros((H, H), bool)
    for (py, px) in ((3, 4), (9, 2), (6, 10)):
        touched[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    ran = {"mfma_": 0, "mfma3_": 0}
    for cfg in range(lib.ssd_conv_num_configs()):
        name = lib.ssd_conv_config_name(cfg)
        fam = "mfma3_" if name.startswith(b"mfma3_") else ("mfma_" if name.startswith(b"mfma_") else None)
        if fam is None:
            continue
        rc, out = run_conv(xbad, w, None, None, None, 1, 1, (1, 1, 1, 1), cfg=cfg)
        if rc == -3:
            continue
        assert rc == 0, lib.ssd_last_error()
        o = _np(out)[0]
        assert not np.isfinite(o[touched]).any(), (name, "a non-finite input was made finite")
        assert np.isfinite(o[~touched]).all(), (name, "a non-finite input leaked outside its receptive field")
        assert np.abs(o[~touched] - ref[0][~touched]).max() <= 1e-4, name
        ran[fam] += 1
    assert ran["mfma_"] >= 4 and ran["mfma3_"] >= 4
    # (2) tiny magnitudes: activations ~1e-34 (around 2^-113), O(1) weights
    tiny = np.float32(1e-34)
    xt = (x * tiny).astype(np.float32)
    reft = no.conv2d(xt.astype(np.float64), w.astype(np.float64), None, 1, 1, "same")
    scale = float(np.abs(reft).max())
    worst = {"mfma_": 0.0, "mfma3_": 0.0}
    for cfg in range(lib.ssd_conv_num_configs()):
        name = lib.ssd_conv_config_name(cfg)
        fam = "mfma3_" if name.startswith(b"mfma3_") else ("mfma_" if name.startswith(b"mfma_") else None)
        if fam is None:
            continue
        rc, out = run_conv(xt, w, None, None, None, 1, 1, (1, 1, 1, 1), cfg=cfg)
        if rc == -3:
            continue
        assert rc == 0, lib.ssd_last_error()
        o = _np(out).astype(np.float64)
        assert np.isfinite(o).all(), name
        worst[fam] = max(worst[fam], float(np.abs(o - reft).max()) / scale)
    print("tiny inputs (|x| ~ 1e-34): max error relative to the output scale: fp32 MFMA tiles %.2e, split-bf16 tiles %.2e" % (
        worst["mfma_"], worst["mfma3_"]))
    assert worst["mfma3_"] <= 2.0 ** -15 and worst["mfma_"] <= 2.0 ** -15


def test_conv2d_splitk_and_strided_output():
    rng = np.random.default_rng(5)
    B, H, Cin, Cout = 2, 10, 1280, 126
    x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
    ref = no.conv2d(x, w, bias)
    pads = same(H, 3, 1) * 2
    for sk in (1, 2, 5):
        rc, out = run_conv(x, w, None, bias, None, 1, 1, pads, cfg=4, split_k=sk)
        assert rc == 0
        _close(_np(out), ref)
    # head-style store: level offset 1444*21 into a [B, 2268*21] buffer, pixel stride = Cout
    Ntot = 2268 * 21
    rc, out = run_conv(x, w, None, bias, None, 1, 1, pads, out_strides=(Ntot, Cout, 1444 * 21, B * Ntot))
    assert rc == 0
    o = _np(out).reshape(B, Ntot)
    np.testing.assert_array_equal(np.isnan(o[:, :1444 * 21]), True)
    _close(o[:, 1444 * 21:1444 * 21 + H * H * Cout], ref.reshape(B, -1))
    assert np.isnan(o[:, 1444 * 21 + H * H * Cout:]).all()


def test_conv2d_errors():
    import ssd_hip as h
    x = np.zeros((1, 4, 4, 8), np.float32)
    w = np.zeros((3, 3, 8, 8), np.float32)
    rc, _ = run_conv(x, w, pads=(-1, 0, 0, 0))
    assert rc == -1 and b"padding" in h.lib().ssd_last_error()
    rc, _ = run_conv(x, w, pads=(0, 0, 0, 0), stride=0)
    assert rc == -1


@pytest.mark.parametrize("H,C,stride", [(150, 32, 1), (75, 144, 2), (38, 192, 1), (19, 576, 2), (10, 960, 1), (7, 8, 2)])
def test_dwconv3x3(H, C, stride):
    import ssd_hip as h
    rng = np.random.default_rng(H * C)
    B = 2
    x = rng.standard_normal((B, H, H, C)).astype(np.float32)
    w = rng.standard_normal((3, 3, C, 1)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    if stride == 2:
        pt, pb = no.correct_pad(H)
        pads = (pt, pb, pt, pb)
    else:
        pads = same(H, 3, 1) * 2
    ref = no.relu6(no.depthwise_conv2d(x, w, stride, pads) * scale + shift)
    xd, wd, sd, hd = guarded(x), guarded(w[..., 0]), guarded(scale), guarded(shift)
    out = torch.empty(ref.shape, dtype=torch.float32, device=xd.device)
    h.check(h.lib().ssd_dwconv3x3(h.ptr(xd), B, H, H, C, stride, pads[0], pads[2], pads[1], pads[3], h.ptr(wd),
                                  h.ptr(sd), h.ptr(hd), 2, h.ptr(out), h.stream()), "dw")
    _close(_np(out), ref, 1e-5)


@pytest.mark.parametrize("H,W,C,stride,pads", [(7, 12, 36, 1, (1, 1, 1, 1)), (13, 6, 8, 2, (1, 1, 0, 1)), (2, 9, 64, 2, (0, 1, 1, 1))])
def test_dwconv3x3_non_square(H, W, C, stride, pads):
    """H != W and pads that differ between the axes (pads = (top, bottom, left, right)): a kernel that decodes the pixel
    with the wrong extent, addresses rows with H, or swaps pad_t and pad_l cannot pass.  Reference: float64."""
    import ssd_hip as h
    rng = np.random.default_rng(1000 * H + W)
    B = 3
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    w = rng.standard_normal((3, 3, C, 1)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    xp = np.pad(x.astype(np.float64), ((0, 0), (pads[0], pads[1]), (pads[2], pads[3]), (0, 0)))
    Ho, Wo = (xp.shape[1] - 3) // stride + 1, (xp.shape[2] - 3) // stride + 1
    assert Ho != Wo
    ref = np.zeros((B, Ho, Wo, C))
    for ky in range(3):
        for kx in range(3):
            ref += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :] * w[ky, kx, :, 0].astype(np.float64)
    ref = np.minimum(np.maximum(ref * scale + shift, 0.0), 6.0)
    xd, wd, sd, hd = guarded(x), guarded(w[..., 0]), guarded(scale), guarded(shift)
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device=xd.device)
    h.check(h.lib().ssd_dwconv3x3(h.ptr(xd), B, H, W, C, stride, pads[0], pads[2], pads[1], pads[3], h.ptr(wd),
                                  h.ptr(sd), h.ptr(hd), 2, h.ptr(out), h.stream()), "dw")
    _close(_np(out), ref, 1e-5)


@pytest.mark.parametrize("H,W,C,k,stride", [(7, 12, 36, 3, 1), (13, 6, 8, 2, 2), (2, 9, 64, 3, 2)])
def test_maxpool_non_square(H, W, C, k, stride):
    """H != W; the SAME pads then differ between the axes ((13, 6) at 2x2 stride 2: (0, 1) on y, none on x;
    (2, 9) at 3x3 stride 2: (0, 1) on y, (1, 1) on x)."""
    import ssd_hip as h
    rng = np.random.default_rng(1000 * H + W)
    B = 3
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    ref = no.max_pool(x, k, stride)
    pt, pb = same(H, k, stride)
    pl, pr = same(W, k, stride)
    assert ref.shape[1] != ref.shape[2] and (stride == 1 or (pt, pb) != (pl, pr))
    xd = guarded(x)
    out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device=xd.device)
    h.check(h.lib().ssd_maxpool2d(h.ptr(xd), B, H, W, C, k, stride, pt, pl, pb, pr, h.ptr(out), h.stream()), "pool")
    np.testing.assert_array_equal(_np(out), ref)


@pytest.mark.parametrize("H,C,k,stride", [(300, 64, 2, 2), (75, 256, 2, 2), (19, 512, 3, 1), (5, 8, 3, 2)])
def test_maxpool(H, C, k, stride):
    import ssd_hip as h
    rng = np.random.default_rng(H + C)
    x = rng.standard_normal((2, H, H, C)).astype(np.float32)
    ref = no.max_pool(x, k, stride)
    a, b = same(H, k, stride)
    xd = guarded(x)
    out = torch.empty(ref.shape, dtype=torch.float32, device=xd.device)
    h.check(h.lib().ssd_maxpool2d(h.ptr(xd), 2, H, H, C, k, stride, a, a, b, b, h.ptr(out), h.stream()), "pool")
    np.testing.assert_array_equal(_np(out), ref)


def test_l2norm_and_softmax():
    import ssd_hip as h
    from models.ssd_vgg16 import L2Normalization
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 38, 38, 512)).astype(np.float32)
    x[0, 0, 0] = 0.0       # all-zero pixel hits the 1e-12 floor
    layer = L2Normalization(20.0)
    _close(_np(layer(x)), no.l2_normalize_scale(x, np.full(512, 20.0, np.float32)), 1e-6)
    assert layer.get_config()["scale_factor"] == 20.0
    for rows, L in ((64 * 2268, 21), (1000, 91), (3, 1), (300, 20000)):
        lg = (rng.standard_normal((rows, L)) * 3).astype(np.float32)
        xd = guarded(lg)
        out = torch.empty_like(xd)
        h.check(h.lib().ssd_softmax(h.ptr(xd), rows, L, h.ptr(out), h.stream()), "softmax")
        _close(_np(out), no.softmax(lg), 1e-6 if L < 100 else 1e-4)   # sequential fp32 row sum
        h.check(h.lib().ssd_softmax(h.ptr(xd), rows, L, h.ptr(xd), h.stream()), "softmax in place")
        np.testing.assert_array_equal(_np(xd), _np(out))


@pytest.fixture(scope="module")
def mbv2():
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    m = get_model(hp)
    m.set_weights(w)
    return m, hp, w


def test_param_table_matches_oracle_spec(mbv2):
    m, hp, w = mbv2
    assert m.param_specs == no.param_specs("mobilenet_v2", hp)
    got = m.get_weights()
    for k in w:
        np.testing.assert_array_equal(got[k], w[k])
    with pytest.raises(ValueError):
        m.set_weights({"nope/kernel": np.zeros(3)})
    with pytest.raises(ValueError):
        m.set_weights({"Conv1/kernel": np.zeros((3, 3, 3, 31), np.float32)})


def test_mobilenet_v2_ssd_forward_parity(mbv2):
    m, hp, w = mbv2
    x = helpers.images(2, 300, seed=0)
    acts = {}
    rd, rp = no.forward("mobilenet_v2", hp, w, x, acts)
    # un-fused graph: every intermediate activation is inspectable
    m.set_option("fuse_blocks", 0)
    d0, p0 = m(x)
    for name in ("Conv1_relu", "expanded_conv_project_BN", "block_1_expand_relu", "block_1_depthwise_relu",
                 "block_3_out", "block_13_expand_relu", "out_relu", "extra1_2", "extra4_2"):
        a = m.fetch_activation(name).reshape(acts[name].shape)
        _close(a, acts[name])
    assert np.abs(_np(p0) - rp).max() <= 1e-4
    _deltas(_np(d0), rd)
    # fused inverted-residual blocks (default): block outputs + final outputs
    m.set_option("fuse_blocks", 1)
    d, p = m(x)
    d, p = _np(d), _np(p)
    assert any(l["kind"] == "fused" and l["flops"] > 0 for l in m.layers(2))
    for name in ("expanded_conv_project_BN", "block_1_out", "block_2_out", "block_3_out", "block_5_out", "block_6_out", "block_7_out",
                 "block_9_out", "block_10_out", "block_12_out", "block_13_expand_relu", "block_14_out", "block_16_out", "out_relu", "extra4_2"):
        a = m.fetch_activation(name).reshape(acts[name].shape)
        _close(a, acts[name])
    assert d.shape == (2, 2268, 4) and p.shape == (2, 2268, 21)
    assert np.abs(p - rp).max() <= 1e-4
    _deltas(d, rd)
    np.testing.assert_allclose(p.sum(-1), 1.0, atol=1e-5)
    # batch-size independence / determinism
    d1, p1 = m(x[:1])
    np.testing.assert_array_equal(_np(d1), d[:1])
    np.testing.assert_array_equal(_np(p1), p[:1])


def test_mobilenet_v2_predict_end_to_end(mbv2):
    """image -> boxes/labels/scores through get_decoder_model(...).predict vs oracle."""
    from models.decoder import get_decoder_model
    from utils import bbox_utils
    m, hp, w = mbv2
    x = helpers.images(3, 300, seed=0)
    priors = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    dm = get_decoder_model(m, priors, hp)
    b, l, s = dm.predict(x, batch_size=2)
    rd, rp = no.forward("mobilenet_v2", hp, w, x)
    rb, rl, rs, rv, ri = co.decode_nms(rd, rp, _np(priors), hp["variances"])
    assert b.shape == (3, 200, 4) and rv.min() > 0
    # indices/labels can legitimately differ only if a score sits within fp32 noise of the
    # 0.5 threshold or an IoU within noise of 0.5; the seeded case has neither.
    np.testing.assert_array_equal(l, rl)
    assert np.abs(s - rs).max() <= 1e-4
    assert np.abs(b - rb).max() <= 1e-4


def test_vgg16_ssd_forward_parity():
    from models.ssd_vgg16 import get_model
    hp = helpers.hyper_params("vgg16")
    w = helpers.synthetic_weights("vgg16", hp)
    m = get_model(hp)
    m.set_weights(w)
    assert m.param_specs == no.param_specs("vgg16", hp)
    x = helpers.images(1, 300, seed=0)
    acts = {}
    rd, rp = no.forward("vgg16", hp, w, x, acts)
    d, p = m(x)
    for name in ("conv1_1", "pool1", "conv4_3", "l2_normalization", "pool5", "conv6", "conv7", "conv9_2", "conv11_2"):
        a = m.fetch_activation(name).reshape(acts[name].shape)
        _close(a, acts[name])
    assert _np(d).shape == (1, 8732, 4)
    assert np.abs(_np(p) - rp).max() <= 1e-4
    _deltas(_np(d), rd)


def test_entry_point_scripts(tmp_path, monkeypatch, capsys):
    """predictor.py / trainer.py keep the reference's flags and run end to end (E1)."""
    import importlib
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "40")
    predictor = importlib.import_module("predictor")
    b, l, s = predictor.main(["--backbone", "mobilenet_v2"])
    assert b.shape == (40, 200, 4) and l.shape == (40, 200) and s.shape == (40, 200)
    assert ((l > 0).sum(-1) > 0).all() and b.min() >= 0 and b.max() <= 1
    # (the trainer entry point has its own test: tests/test_train.py::test_trainer_entry_point_fit)
    out = capsys.readouterr().out
    assert "predicted 40 images" in out


def test_predictor_custom_images_and_evaluate(tmp_path, monkeypatch, capsys):
    """E1 wired to N4 and N2 (reference predictor.py:10-12, 35-40, 54-55): ``use_custom_images`` reads uint8
    images from ``custom_image_path`` (PIL + LANCZOS on the host like the reference, uint8 -> float on the
    GPU) and must give the detections of the same model on the identically prepared arrays; ``evaluate``
    drops difficult objects in ``preprocessing`` and returns the VOC07 mAP statistics, equal to the
    oracle's on the same predictions / ground truth."""
    import importlib
    from PIL import Image
    from models.decoder import get_decoder_model
    from models.ssd_mobilenet_v2 import get_model
    from oracle import eval_oracle as eo
    from utils import bbox_utils, data_utils, train_utils
    monkeypatch.chdir(tmp_path)
    predictor = importlib.import_module("predictor")
    rng = np.random.default_rng(77)
    d = tmp_path / "imgs"
    d.mkdir()
    arrays = []
    for i, (h, w) in enumerate([(375, 500), (333, 500), (300, 300), (480, 360), (512, 512)]):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 2:
            Image.fromarray(a).save(str(d / ("img_%d.png" % i)))
        else:
            np.save(str(d / ("img_%d.npy" % i)), a)
        arrays.append((("img_%d.png" if i % 2 else "img_%d.npy") % i, a))
    b, l, s = predictor.main(["--backbone", "mobilenet_v2"], use_custom_images=True, custom_image_path=str(d), batch_size=4)
    assert b.shape == (5, 200, 4) and "predicted 5 images" in capsys.readouterr().out
    # the same model on the arrays prepared on the host: LANCZOS resize, then / 255 in float32
    hp = train_utils.get_hyper_params("mobilenet_v2")
    hp["total_labels"] = 21
    m = get_model(hp, max_batch=4)
    data_utils.synthetic_weights(m)
    pri = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    dm = get_decoder_model(m, pri, hp)
    host = np.stack([np.asarray(Image.fromarray(a).resize((300, 300), Image.LANCZOS), np.uint8)
                     for _, a in sorted(arrays)]).astype(np.float32) * np.float32(1.0 / 255.0)
    rb, rl, rs = dm.predict(host, batch_size=4)
    np.testing.assert_array_equal(l, rl)
    np.testing.assert_array_equal(s, rs)
    np.testing.assert_array_equal(b, rb)
    assert ((l > 0).sum(-1) > 0).all()
    # evaluate=True: difficult objects filtered in preprocessing, mAP bookkeeping = the oracle's
    monkeypatch.setenv("SSD_SYNTHETIC_ITEMS", "12")
    b, l, s, stats = predictor.main(["--backbone", "mobilenet_v2"], evaluate=True, batch_size=5)
    out = capsys.readouterr().out
    assert "mAP: " in out and b.shape[0] == 12
    items = list(data_utils.synthetic_voc_items(12, 21))
    kept = sum(int((~it["objects"]["is_difficult"]).sum()) for it in items)
    assert sum(rec["total"] for rec in stats.values()) == kept < sum(len(it["objects"]["label"]) for it in items)
    labels = ["bg"] + data_utils.get_labels()
    ref = eo.init_stats(labels)
    gts = [(it["objects"]["bbox"][~it["objects"]["is_difficult"]], (it["objects"]["label"][~it["objects"]["is_difficult"]] + 1).astype(np.int32))
           for it in items]
    for i in range(0, 12, 5):
        chunk = gts[i:i + 5]
        g = max([len(c[0]) for c in chunk] + [1])
        gt = np.zeros((len(chunk), g, 4), np.float32)
        gl = -np.ones((len(chunk), g), np.int32)
        for j, (bb, ll) in enumerate(chunk):
            gt[j, :len(bb)] = bb
            gl[j, :len(ll)] = ll
        eo.update_stats(b[i:i + 5], l[i:i + 5], s[i:i + 5], gt, gl, ref)
    ref, ref_map = eo.calculate_mAP(ref)
    for cid in ref:
        assert ref[cid]["total"] == stats[cid]["total"] and ref[cid]["tp"] == stats[cid]["tp"], cid
        np.testing.assert_array_equal(np.asarray(ref[cid]["AP"]), np.asarray(stats[cid]["AP"]))
    assert ("mAP: %s" % float(ref_map)) in out


def test_eval_utils_map():
    """VOC07 11-point mAP (N2): perfect predictions -> AP 1; shuffled labels -> lower."""
    from utils import eval_utils
    labels = ["bg", "a", "b", "c"]
    gt, gl = helpers.gt_inputs(6, G=5, L=4, seed=9)
    T = 8
    pb = np.zeros((6, T, 4), np.float32); pl = np.zeros((6, T), np.float32); ps = np.zeros((6, T), np.float32)
    for i in range(6):
        n = int((gl[i] > 0).sum())
        pb[i, :n] = gt[i, :n]; pl[i, :n] = gl[i, :n]; ps[i, :n] = np.linspace(0.9, 0.6, n)
    stats = eval_utils.init_stats(labels)
    stats = eval_utils.update_stats(pb, pl, ps, gt, gl, stats)
    stats, m = eval_utils.calculate_mAP(stats)
    with_gt = [k for k in stats if stats[k]["total"] > 0]
    assert with_gt and all(abs(stats[k]["AP"] - 1.0) < 1e-9 for k in with_gt)
    # a class without GT/predictions contributes AP 0 to the mean, like the reference's loop
    assert abs(float(m) - len(with_gt) / 3.0) < 1e-9
    pl2 = pl.copy(); pl2[pl2 > 0] = (pl2[pl2 > 0] % 3) + 1
    stats = eval_utils.update_stats(pb, pl2, ps, gt, gl, eval_utils.init_stats(labels))
    _, m2 = eval_utils.calculate_mAP(stats)
    assert float(m2) < float(m)


@pytest.mark.parametrize("H,Cin,Cout,k,stride", [(19, 576, 100, 3, 1), (10, 1280, 150, 3, 1), (5, 512, 150, 3, 1),
                                                 (10, 256, 512, 3, 2), (3, 256, 150, 3, 1), (1, 256, 100, 3, 1),
                                                 (10, 1280, 256, 1, 1), (19, 96, 576, 1, 1)])
def test_conv2d_every_config_and_split_on_net_shapes(H, Cin, Cout, k, stride):
    """The autotuner may pick ANY valid (tile config, split-K) for a layer; every such choice
    must be correct on the real SSD layer shapes (long K, ragged N, tiny M)."""
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(H * Cin + Cout)
    B = 2
    x = rng.standard_normal((B, H, H, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
    pads = same(H, k, stride) * 2 if k == 3 else (0, 0, 0, 0)
    ref = no.relu(no.conv2d(x, w, bias, stride, 1, "same" if k == 3 else "valid"))
    ran = 0
    for cfg in range(lib.ssd_conv_num_configs()):
        if lib.ssd_conv_config_name(cfg).startswith(b"bf16_"):
            continue            # (tests/test_bf16_gpu.py)
        for split in (1, 2, 4, 8, 16):
            rc, out = run_conv(x, w, None, bias, None, stride, 1, pads, act=1, cfg=cfg, split_k=split)
            if rc == -3:
                break
            assert rc == 0, (cfg, split, lib.ssd_last_error())
            err = float(np.abs(_np(out) - ref).max())
            assert err <= 1e-4 * max(1.0, float(np.abs(ref).max())), (lib.ssd_conv_config_name(cfg), split, err)
            ran += 1
    assert ran >= 20


def test_mobilenet_v2_ssd512_forward_parity():
    """BASELINE config 5 graph: the same MobileNetV2-SSD at 512x512 (feature maps 32,16,8,4,2,1,
    6132 priors; every stride-2 depthwise pads (0,1) because all its inputs are even)."""
    from models.ssd_mobilenet_v2 import get_model
    from utils import bbox_utils
    hp = helpers.hyper_params("mobilenet_v2")
    hp["img_size"] = 512
    hp["feature_map_shapes"] = [32, 16, 8, 4, 2, 1]
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    m = get_model(hp)
    m.set_weights(w)
    assert m.num_priors == 6132
    x = helpers.images(1, 512, seed=3)
    acts = {}
    rd, rp = no.forward("mobilenet_v2", hp, w, x, acts)
    d, p = m(x)
    assert _np(d).shape == (1, 6132, 4) and _np(p).shape == (1, 6132, 21)
    for name in ("block_3_out", "block_6_out", "out_relu", "extra4_2"):
        _close(m.fetch_activation(name).reshape(acts[name].shape), acts[name])
    assert np.abs(_np(p) - rp).max() <= 1e-4
    _deltas(_np(d), rd)
    pri = bbox_utils.generate_prior_boxes(hp["feature_map_shapes"], hp["aspect_ratios"])
    assert tuple(pri.shape) == (6132, 4)
    with pytest.raises(ValueError):          # feature_map_shapes must match the graph at this img_size
        bad = dict(hp); bad["feature_map_shapes"] = [19, 10, 5, 3, 2, 1]
        get_model(bad)


def test_weights_container_roundtrip(tmp_path, mbv2):
    """N3: weights container.  `*.h5` is a real Keras-layout HDF5 file (pure-Python writer /
    reader), `*.npz` the NumPy alternative; load_weights sniffs the magic; a Keras file holding a
    subset of the layers (h5py-written fixture) loads with by_name=True."""
    import os
    from models.ssd_mobilenet_v2 import get_model
    from utils import h5_reader
    m, hp, w = mbv2
    path = str(tmp_path / "ssd_mobilenet_v2_model_weights.h5")
    m.save_weights(path)
    assert h5_reader.is_hdf5(path)
    npz = str(tmp_path / "w.npz")
    m.save_weights(npz)
    m3 = get_model(hp)
    m3.load_weights(npz)
    for k, v in m3.get_weights().items():
        np.testing.assert_array_equal(v, np.asarray(w[k], np.float32))
    # h5py-written Keras fixture (tests/golden/make_keras_h5.py): partial load by name
    fx = os.path.join(os.path.dirname(__file__), "golden", "keras_tiny_weights.h5")
    exp = np.load(os.path.join(os.path.dirname(__file__), "golden", "keras_tiny_expected.npz"))
    with pytest.raises(ValueError):
        m3.load_weights(fx)                     # topology mismatch without by_name, like Keras
    m3.load_weights(fx, by_name=True)
    got = m3.get_weights()
    for k in ("Conv1/kernel", "bn_Conv1/gamma", "bn_Conv1/moving_variance", "expanded_conv_depthwise/depthwise_kernel",
              "expanded_conv_project/kernel"):
        np.testing.assert_array_equal(got[k], exp[k])
    np.testing.assert_array_equal(got["block_1_expand/kernel"], np.asarray(w["block_1_expand/kernel"], np.float32))
    bad = str(tmp_path / "junk.h5")
    open(bad, "wb").write(b"not a weights file")
    with pytest.raises(ValueError):
        m3.load_weights(bad)
    m2 = get_model(hp)
    m2.load_weights(path)
    x = helpers.images(1, 300, seed=5)
    d1, p1 = m(x)
    # the second instance runs the first one's kernel table (tile shapes / split-K decide the summation
    # order): the round trip through the file must then be invisible bit for bit
    m2.set_tuning(m.get_tuning())
    d2, p2 = m2(x)
    assert m2.tuning_info["source"] == "explicit" and m2.tuning_info["reproducible"]
    assert m2.get_tuning() == m.get_tuning()
    w2 = m2.get_weights()
    assert set(w2) == set(w)
    for k in w:
        np.testing.assert_array_equal(w2[k], np.asarray(w[k], np.float32))
    np.testing.assert_array_equal(_np(p1), _np(p2))
    np.testing.assert_array_equal(_np(d1), _np(d2))
    # a third instance with NO table handed over: shipped table or the process-wide memo -> same kernels too
    m4 = get_model(hp, max_batch=m._finalized_for)
    m4.load_weights(npz)
    d4, p4 = m4(x)
    assert m4.tuning_info["source"] in ("shipped", "memo", "cache") and m4.get_tuning() == m.get_tuning()
    np.testing.assert_array_equal(_np(p1), _np(p4))
    np.testing.assert_array_equal(_np(d1), _np(d4))
    # and a table tuned independently (forced on-device autotune) stays within the contract's 1e-4
    import tuning
    m5 = get_model(hp)
    m5.load_weights(npz)
    m5.set_tuning("")
    d5, p5 = m5(x)
    assert m5.tuning_info["choices_timed_on_device"] > 0
    assert np.abs(_np(p1) - _np(p5)).max() <= 1e-4
    _close(_np(d1), _np(d5), tol=1e-4)


def test_conv_bk64_tiles_do_not_read_past_packed_weights():
    """K = 32 / 96 / 160 (Kpad a multiple of 32 but not of 64) under every BK=64 tile config:
    the last k-tile must not touch memory past the packed [Npad][Kpad] weights (NaN-poisoned
    in run_conv) -- this faulted in ssd_net_finalize's autotune on block_4_expand."""
    import ssd_hip as h
    lib = h.lib()
    rng = np.random.default_rng(21)
    ran = 0
    for Cin, Cout in ((32, 192), (96, 576), (160, 960)):
        x = rng.standard_normal((2, 10, 10, Cin)).astype(np.float32)
        w = (rng.standard_normal((1, 1, Cin, Cout)) / np.sqrt(Cin)).astype(np.float32)
        ref = no.conv2d(x, w, None, 1, 1, "valid")
        for c in range(lib.ssd_conv_num_configs()):
            if b"k64" not in lib.ssd_conv_config_name(c):
                continue
            rc, out = run_conv(x, w, cfg=c)
            assert rc == 0, h.last_error()
            _close(_np(out), ref)
            ran += 1
    assert ran > 0


@pytest.mark.parametrize("backbone", ["mobilenet_v2", "vgg16"])
def test_forward_parity_with_poisoned_arena(backbone, monkeypatch):
    """Every activation surrounded by NaN (SSD_HIP_DEBUG_POISON): no kernel of either graph,
    fused or layer-by-layer, may read outside its tensors or rely on zeroed scratch."""
    monkeypatch.setenv("SSD_HIP_DEBUG_POISON", "1")
    if backbone == "mobilenet_v2":
        from models.ssd_mobilenet_v2 import get_model
    else:
        from models.ssd_vgg16 import get_model
    hp = helpers.hyper_params(backbone)
    w = helpers.synthetic_weights(backbone, hp)
    x = helpers.images(3, 300, seed=11)
    rd, rp = no.forward(backbone, hp, w, x)
    for fuse in ((1, 0) if backbone == "mobilenet_v2" else (1,)):
        m = get_model(hp)
        m.set_weights(w)
        m.set_option("fuse_blocks", fuse)
        d, p = m(x)
        assert np.isfinite(_np(p)).all() and np.isfinite(_np(d)).all()
        assert np.abs(_np(p) - rp).max() <= 1e-4
        _deltas(_np(d), rd)


@pytest.mark.parametrize("B,ticket", [(1, 0), (5, 0), (5, 1), (24, 1), (64, 0), (232, 0)])
def test_image_block_kernel_vs_layer_kernels(B, ticket):
    """Whole-image inverted-residual kernel (csrc/ssd_imgblock.hip; blocks 7-12, 14-16) against the
    expand GEMM + depthwise/project kernels on the same weights: B = 1 / 5 take 12 channel groups per
    image, B = 24 takes 8-10, B = 64 four, B = 232 the direct one-group epilogue.  The group slabs are
    combined by a second launch (default) or inside the launch by the last arriving group of each image
    (image_ticket: slabs cross XCDs).  Run twice: bitwise repeatable (fixed group summation order)."""
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.images(min(B, 8), 300, seed=17)
    if B > 8:
        x = np.concatenate([x] * ((B + 7) // 8))[:B] * np.linspace(0.5, 1.0, B, dtype=np.float32)[:, None, None, None]
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    # block 13 (depthwise stride 2) also writes its expanded map -- SSD feature map 1 -- from the same kernel
    names = ["block_%d_out" % k for k in (7, 8, 9, 10, 11, 12, 13, 14, 15, 16)] + ["block_13_expand_relu"]
    m.set_option("fuse_image", 0)
    d0, p0 = m(x)
    ref = {n: m.fetch_activation(n).copy() for n in names}
    assert not any(l["name"] == "block_7_fused" and l["flops"] > 0 for l in m.layers(B))
    m.set_option("image_ticket", ticket)
    m.set_option("fuse_image", 2)       # 2: wherever the kernel applies (1 = where it won the finalize-time race)
    d1, p1 = m(x)
    assert any(l["name"] == "block_7_fused" and l["flops"] > 0 for l in m.layers(B))
    assert any(l["name"] == "block_13_fused" and l["flops"] > 0 for l in m.layers(B))
    got = {n: m.fetch_activation(n).copy() for n in names}
    for n in names:
        scale = np.abs(ref[n]).max()
        assert np.abs(got[n] - ref[n]).max() <= 2e-5 * scale, n
    assert np.abs(_np(p1) - _np(p0)).max() <= 2e-5
    d2, p2 = m(x)
    np.testing.assert_array_equal(_np(d2), _np(d1))
    np.testing.assert_array_equal(_np(p2), _np(p1))
    for n in names:
        np.testing.assert_array_equal(m.fetch_activation(n), got[n])


@pytest.mark.parametrize("B,S", [(5, 300), (64, 300), (3, 512)])
def test_band3_weights_through_lds_dma_bitwise(B, S):
    """Option image_v2 selects the whole-image kernel's form only and does not touch blocks 1-6: the split row-band kernel
    (blocks 3-6) has one form, with its weight fragments staged by LDS-DMA (two We stages + one Wp stage of 1 KB blocks).  With
    image_v2 0 and 1 the outputs of blocks 3, 5 and 6 (stem + blocks 1-6) are bitwise equal, incl. the lone last chunk of the
    144-channel block 3 and the 512 x 512 graph's pitches.  (The form that prefetched the fragments into registers, which
    image_v2 0 used to select here and which this test held bitwise equal to the LDS-DMA form, is gone.)"""
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    if S == 512:
        hp["img_size"] = 512
        hp["feature_map_shapes"] = [32, 16, 8, 4, 2, 1]
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.images(min(B, 8), S, seed=23)
    if B > 8:
        x = np.concatenate([x] * ((B + 7) // 8))[:B] * np.linspace(0.5, 1.0, B, dtype=np.float32)[:, None, None, None]
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    got = {}
    for v in (0, 1):
        m.set_option("image_v2", v)
        m(x)
        assert any(l["name"] == "block_4_fused" and l["config"] == "band3" and l["flops"] > 0 for l in m.layers(B))
        got[v] = {n: m.fetch_activation(n).copy() for n in ("block_3_out", "block_5_out", "block_6_out")}
    for n in got[0]:
        np.testing.assert_array_equal(got[0][n].view(np.uint32), got[1][n].view(np.uint32))
    assert np.abs(got[1]["block_6_out"]).max() > 0


@pytest.mark.parametrize("B,second", [(3, 1), (3, 0), (24, 1), (64, 1), (64, 0), (232, 1)])
def test_image_block_split_form_vs_layer_kernels(B, second):
    """(``second`` = option image_v2: the kernel's second form, csrc/ssd_imgblock2.hip -- compile-time geometry, adjacent
    pixels per lane, LDS-DMA weight chunks, chunk pairs dealt unevenly over the groups: B = 3 / 24 give 12 / 8 groups of
    2 - 4 pairs, B = 232 the direct one-group epilogue with the residual -- or the first form for every block; block 13,
    stride 2, has a second-form configuration of its own (kImage2's stride-2 entry) and follows the option like the
    rest.  The two forms agree within tolerance, not bitwise: the k-slot order inside the project MFMAs differs.)
    The whole-image kernel's split-bf16 form (img_choice 2: both 1x1 convolutions as exact three-way bf16 splits,
    six v_mfma_f32_16x16x32_bf16 per product, fp32 results; weights staged through LDS) pinned on every block it can
    run -- the finalize-time race only keeps it where it wins -- against the layer kernels, to the fp32 kernels' own
    tolerance; the table line reads back as "image 2" and the layer reports "image_split"."""
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.images(min(B, 8), 300, seed=19)
    if B > 8:
        x = np.concatenate([x] * ((B + 7) // 8))[:B] * np.linspace(0.5, 1.0, B, dtype=np.float32)[:, None, None, None]
    m = get_model(hp, max_batch=B)
    m.set_weights(w)
    m.set_option("image_v2", second)
    names = ["block_%d_out" % k for k in range(7, 17)] + ["block_13_expand_relu"]
    m.set_option("fuse_image", 0)
    d0, p0 = m(x)
    ref = {n: m.fetch_activation(n).copy() for n in names}
    table = m.get_tuning()
    pinned = "\n".join((l.rsplit(" ", 1)[0] + " 2") if " image " in l else l for l in table.splitlines()) + "\n"
    assert pinned.count(" image 2") == 10
    m.set_tuning(pinned)
    m.set_option("fuse_image", 1)
    d1, p1 = m(x)
    assert m.get_tuning().count(" image 2") == 10
    cfg = {l["name"]: l["config"] for l in m.layers(B) if l["flops"] > 0}
    assert all(cfg.get("block_%d_fused" % k) == "image_split" for k in range(7, 17)), cfg
    for n in names:
        scale = np.abs(ref[n]).max()
        assert np.abs(m.fetch_activation(n) - ref[n]).max() <= 2e-5 * scale, n
    assert np.abs(_np(p1) - _np(p0)).max() <= 2e-5
    d2, p2 = m(x)
    np.testing.assert_array_equal(_np(d2), _np(d1))
    np.testing.assert_array_equal(_np(p2), _np(p1))


def test_get_head_from_outputs_composition():
    """models.header.get_head_from_outputs (reference models/header.py:43-67) as a composition of
    op-level C-ABI calls vs the NumPy oracle: 12 head convs stored at their level offsets of the
    concatenated buffers + softmax; and HeadWrapper's reshape/concat order."""
    from models import header
    hp = helpers.hyper_params("mobilenet_v2", total_labels=5)
    hp["feature_map_shapes"] = [5, 3, 2, 2, 1, 1]
    rng = np.random.default_rng(21)
    chans = [48, 64, 32, 16, 16, 16]
    B = 3
    feats = [rng.standard_normal((B, f, f, c)).astype(np.float32) for f, c in zip(hp["feature_map_shapes"], chans)]
    wts = {}
    d, p = header.get_head_from_outputs(hp, feats, wts, seed=4)
    assert len(wts) == 24 and wts["2_conv_label_output/kernel"].shape == (3, 3, 64, 6 * 5)
    for i in range(1, 7):       # non-zero biases for the real check
        for kind in ("label", "boxes"):
            n = "%d_conv_%s_output/bias" % (i, kind)
            wts[n] = rng.uniform(-0.5, 0.5, wts[n].shape).astype(np.float32)
    d, p = header.get_head_from_outputs(hp, feats, wts)
    lab, box = [], []
    for i, f in enumerate(feats):
        lab.append(no.conv2d(f, wts["%d_conv_label_output/kernel" % (i + 1)], wts["%d_conv_label_output/bias" % (i + 1)]))
        box.append(no.conv2d(f, wts["%d_conv_boxes_output/kernel" % (i + 1)], wts["%d_conv_boxes_output/bias" % (i + 1)]))
    rl = np.concatenate([t.reshape(B, -1, 5) for t in lab], 1)
    rb = np.concatenate([t.reshape(B, -1, 4) for t in box], 1)
    N = sum(f * f * (len(a) + 1) for f, a in zip(hp["feature_map_shapes"], hp["aspect_ratios"]))
    assert tuple(d.shape) == (B, N, 4) and tuple(p.shape) == (B, N, 5)
    _abs(_np(d), rb, 1e-5)
    _abs(_np(p), no.softmax(rl), 1e-5)
    # HeadWrapper alone (reference models/header.py:34-41)
    hw = header.HeadWrapper(5, name="labels_head")
    np.testing.assert_array_equal(_np(hw(lab)), rl)
    assert hw.get_config() == {"name": "labels_head", "last_dimension": 5}
    with pytest.raises(ValueError):
        header.get_head_from_outputs(hp, feats[:3])


WINO_CASES = [
    # (B, H, W, Cin, Cout, padding)
    (2, 19, 19, 64, 100, "same"),       # head level 1 geometry (odd size: half tiles at the border), Cout = A*(L+4)
    (3, 10, 10, 128, 150, "same"),      # head level 2, Cout % 4 != 0 -> scalar stores
    (2, 5, 5, 48, 150, "same"),
    (4, 1, 1, 32, 100, "same"),         # 1x1 feature map: a single quarter tile
    (2, 2, 3, 16, 24, "same"),
    (1, 38, 38, 64, 64, "same"),        # VGG-like
    (2, 5, 5, 32, 40, "valid"),         # VGG conv10_2 / conv11_2: VALID 3x3
    (1, 7, 9, 16, 20, (2, 0, 0, 2)),    # asymmetric explicit pads
]


@pytest.mark.parametrize("case", WINO_CASES)
def test_conv2d_winograd_all_configs(case):
    """Winograd F(2x2,3x3) kernels (csrc/ssd_wino.hip) vs the NumPy oracle for every tile
    configuration, with and without the channel split, scale/shift/activation epilogue, strided
    destination; NaN-poisoned surroundings catch out-of-bounds reads."""
    import ssd_hip as h
    lib = h.lib()
    B, H, W, Cin, Cout, padding = case
    rng = np.random.default_rng(abs(hash(case[:5])) % 1000)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
    if padding == "same":
        pads = same(H, 3, 1) + same(W, 3, 1)
        ref = no.conv2d(x, w, None, 1, 1, "same")
    elif padding == "valid":
        pads = (0, 0, 0, 0)
        ref = no.conv2d(x, w, None, 1, 1, "valid")
    else:
        pads = padding
        ref = no.conv2d(x, w, None, 1, 1, pads)
    ref = no.relu6(ref * scale + shift)
    Ho, Wo = ref.shape[1], ref.shape[2]
    d = h.ConvDesc(B, H, W, Cin, Cout, 3, 3, 1, 1, pads[0], pads[2], pads[1], pads[3], 2, 0)
    xd, wd = guarded(x), h.to_dev(w)
    nu = lib.ssd_conv_wino_weight_floats(Cin, Cout)
    poisoned = torch.full((nu + 4096,), float("nan"), dtype=torch.float32, device=xd.device)
    U = poisoned[:nu]
    h.check(lib.ssd_conv_wino_pack_weights(h.ptr(wd), Cin, Cout, h.ptr(U), h.stream()), "wino pack")
    sd, hd = guarded(scale), guarded(shift)
    worst = 0.0
    for cfg in range(lib.ssd_conv_wino_num_configs()):
        for sk in (1, 2, 3):
            if sk > Cin // 16:
                continue
            out = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float32, device=xd.device)
            ws = torch.full((max(1, sk * B * Ho * Wo * Cout),), float("nan"), dtype=torch.float32, device=xd.device) if sk > 1 else None
            rc = lib.ssd_conv2d_wino(ctypes.byref(d), h.ptr(xd), h.ptr(U), h.ptr(sd), h.ptr(hd), h.ptr(out), 0, 0, cfg, sk,
                                     h.ptr(ws), h.stream())
            assert rc == 0, (cfg, sk, lib.ssd_last_error())
            err = float(np.abs(_np(out) - ref).max())
            worst = max(worst, err)
            assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (cfg, sk, err)
    # strided destination (the concatenated head buffer): level slab inside a NaN canvas
    total = B * (Ho * Wo * Cout + 77) + 13
    canvas = torch.full((total,), float("nan"), dtype=torch.float32, device=xd.device)
    off = 12 if Cout % 4 == 0 else 13
    rc = lib.ssd_conv2d_wino(ctypes.byref(d), h.ptr(xd), h.ptr(U), h.ptr(sd), h.ptr(hd), h.vp(canvas.data_ptr() + 4 * off),
                             Ho * Wo * Cout + 77, Cout, 0, 1, None, h.stream())
    assert rc == 0
    c = _np(canvas)
    for b in range(B):
        s0 = off + b * (Ho * Wo * Cout + 77)
        np.testing.assert_allclose(c[s0:s0 + Ho * Wo * Cout].reshape(Ho, Wo, Cout), ref[b], atol=2e-5 * max(1.0, float(np.abs(ref).max())))
        assert np.isnan(c[s0 + Ho * Wo * Cout:s0 + Ho * Wo * Cout + 77 - (0 if b < B - 1 else 77 - 1)]).all()
    print("winograd worst abs err %.2e (max |ref| %.2f)" % (worst, float(np.abs(ref).max())))
    # not applicable: stride 2 / Cin % 16 != 0
    bad = h.ConvDesc(B, H, W, Cin, Cout, 3, 3, 2, 1, 1, 1, 1, 1, 0, 0)
    assert lib.ssd_conv2d_wino(ctypes.byref(bad), h.ptr(xd), h.ptr(U), None, None, h.ptr(out), 0, 0, 0, 1, None, h.stream()) == -3
