"""Every dense conv tile against the float64 oracle (oracle/conv_oracle.py) OFF the square-map path: the sixteen geometry
cases of tests/conv_geometry_cases.py (H != W, kh != kw, four different pads, stride, dilation; M <= 168), every config of
every family through the entry point that owns it:

* ``ssd_conv2d_ex``: config -1, ``mfma_*``, ``skinny_*``, ``mfma3_*``, ``bf16_*``, ``direct_valu``;
* ``ssd_conv2d_planes``: ``dma3_*`` (3 planes), ``dmab_*`` (1 plane);  ``ssd_conv2d_planes_f16x2``: ``dmah_*``;
* ``ssd_conv2d_wino``: the Winograd tiles, with the channel split 1, 2, 3.

Epilogue on (scale, shift, ReLU6, dense residual; Winograd takes no residual; the RGB stem runs with and without one: the
stem kernel and the generic direct kernel).  Bars, all the existing ones: fp32 families 1e-4 max(1, max |ref|), Winograd 2e-5
max(1, max |ref|), ``bf16_*`` / ``dmab_*`` (no epilogue) 2e-5 max |ref| against the float64 conv of the bf16-rounded operands,
``dma3_*`` bitwise its ``mfma3_*`` twin, a plane output = the split of the fp32 output beside it.

A refusal is a condition: the (case, family) pairs of ``conv_geometry_cases.REFUSALS`` answer -3 with "cannot run", every
other pair returns 0 on every config.

Strided destination (the concatenated head buffer) on two cases, every config that runs there, split-K 1, 2, 3: a
16-byte aligned layout (vector stores) and an odd one (scalar stores) inside a canvas pre-filled with a NaN of a chosen
payload -- values within the family's bar, every word outside the destination bit for bit untouched.

Every input sits in a NaN-poisoned buffer (``guarded`` / ``make_planes``)."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

import conv_geometry_cases as gc
from oracle import conv_oracle as cv
from test_conv_gpu import run_conv, guarded, _np
from test_bf16_gpu import bf16_round
from test_convdma_gpu import make_planes, run_conv_planes, dma_configs
from test_f16x2_gpu import run_conv_h, pack_weights, expect_plane_output

# (the shared inputs are read-only NumPy arrays; torch warns once when it wraps one, and only ever copies FROM it)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

PAYLOAD = 0x7FC5A5A5            # a quiet NaN no kernel produces
RECORD = {}                     # (family, case) -> worst err / scale, printed by the last test
IDS = lambda c: c.name


def family_of(name):
    for prefix, fam in gc.PREFIX.items():
        if name.startswith(prefix):
            return fam
    raise AssertionError("config %r belongs to no known family" % name)


def ex_configs():
    """(config id, name, family) of what ``ssd_conv2d_ex`` owns."""
    import ssd_hip as h
    lib = h.lib()
    out = [(-1, "auto", "auto")]
    for cfg in range(lib.ssd_conv_num_configs()):
        name = lib.ssd_conv_config_name(cfg).decode()
        if family_of(name) in ("mfma", "skinny", "mfma3", "bf16", "direct"):
            out.append((cfg, name, family_of(name)))
    return out


_BREF = {}


def bf16_ref(c):
    """float64 conv of the bf16-rounded operands (what ``bf16_*`` / ``dmab_*`` define), once per case."""
    if c.name not in _BREF:
        d = gc.data(c)
        r = cv.conv2d_f64(bf16_round(d["x"]), bf16_round(d["w"]), c.stride, c.dil, c.pads)
        r.setflags(write=False)
        _BREF[c.name] = r
    return _BREF[c.name]


def bars(c):
    """family -> (reference, bar, scale the record divides by)."""
    d = gc.data(c)
    s32 = max(1.0, float(np.abs(d["ref"]).max()))
    sno = max(1.0, float(np.abs(d["ref_nores"]).max()))
    sb = float(np.abs(bf16_ref(c)).max())
    fp32 = (d["ref"], 1e-4 * s32, s32)
    rounded = (bf16_ref(c), 2e-5 * sb, sb)
    return {"auto": fp32, "mfma": fp32, "skinny": fp32, "mfma3": fp32, "direct": fp32, "dma3": fp32, "dmah": fp32,
            "bf16": rounded, "dmab": rounded, "wino": (d["ref_nores"], 2e-5 * sno, sno),
            "nores": (d["ref_nores"], 1e-4 * sno, sno)}


def hold(got, ref, bar, scale, fam, c, tag):
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    key = (fam, c.name)
    RECORD[key] = max(RECORD.get(key, 0.0), err / scale) if err == err else float("nan")
    assert err <= bar, "%s %s %s: max abs err %.3e, bar %.3e" % (c.name, fam, tag, err, bar)


def refused(rc, c, fam, tag):
    import ssd_hip as h
    msg = h.lib().ssd_last_error()
    assert rc == -3 and b"cannot run" in msg, "%s %s %s must refuse with -3 'cannot run': rc %d, %r" % (c.name, fam, tag, rc, msg)


def ran_ok(rc, c, fam, tag):
    import ssd_hip as h
    assert rc == 0, "%s %s %s must run (it is not in the refusal table): rc %d, %r" % (c.name, fam, tag, rc, h.lib().ssd_last_error())


def ex_args(c, fam, residual=True):
    """run_conv arguments of a family: no epilogue for the bf16 tiles, the full one for the others."""
    d = gc.data(c)
    if fam == "bf16":
        return dict(stride=c.stride, dil=c.dil, pads=c.pads)
    return dict(scale=d["scale"], shift=d["shift"], res=d["res"] if residual else None, stride=c.stride, dil=c.dil, pads=c.pads, act=2)


class Wino:
    """``ssd_conv2d_wino`` on a case: weights transformed once (3x3 cases only: the transform reads 9 Cin Cout floats)."""

    def __init__(self, c):
        import ssd_hip as h
        lib = h.lib()
        d = gc.data(c)
        self.c, self.h, self.lib = c, h, lib
        self.desc = h.ConvDesc(c.B, c.H, c.W, c.Cin, c.Cout, c.kh, c.kw, c.stride, c.dil, c.pads[0], c.pads[2], c.pads[1], c.pads[3], 2, 0)
        self.xd = guarded(d["x"])
        nu = lib.ssd_conv_wino_weight_floats(c.Cin, c.Cout)
        poisoned = torch.full((nu + 4096,), float("nan"), dtype=torch.float32, device=self.xd.device)
        self.U = poisoned[:nu]
        if c.kh == 3 and c.kw == 3:
            wd = h.to_dev(d["w"])
            h.check(lib.ssd_conv_wino_pack_weights(h.ptr(wd), c.Cin, c.Cout, h.ptr(self.U), h.stream()), "wino pack")
        else:
            self.U.zero_()
        self.sd, self.hd = guarded(d["scale"]), guarded(d["shift"])
        self.Ho, self.Wo = gc.out_hw(c)

    def run(self, cfg, sk, out_strides=None, canvas=None):
        h, c = self.h, self.c
        if out_strides is None:
            out = torch.full((c.B, self.Ho, self.Wo, c.Cout), float("nan"), dtype=torch.float32, device=self.xd.device)
            bs = ps = 0
            optr = h.ptr(out)
        else:
            bs, ps, off, total = out_strides
            out = canvas
            assert out.numel() == total
            optr = h.vp(out.data_ptr() + 4 * off)
        ws = torch.full((sk * c.B * self.Ho * self.Wo * c.Cout,), float("nan"), dtype=torch.float32, device=self.xd.device) if sk > 1 else None
        rc = self.lib.ssd_conv2d_wino(ctypes.byref(self.desc), h.ptr(self.xd), h.ptr(self.U), h.ptr(self.sd), h.ptr(self.hd), optr, bs, ps,
                                      cfg, sk, h.ptr(ws), h.stream())
        return rc, out


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_every_config_on_every_geometry_case(c):
    import ssd_hip as h
    lib = h.lib()
    d = gc.data(c)
    B = bars(c)
    ran = collections.Counter()
    mfma3_bits = {}
    # ---- ssd_conv2d_ex
    for cfg, name, fam in ex_configs():
        rc, out = run_conv(d["x"], d["w"], cfg=cfg, **ex_args(c, fam))
        if gc.must_refuse(c, fam):
            refused(rc, c, fam, name)
            continue
        ran_ok(rc, c, fam, name)
        hold(_np(out), *B[fam], fam, c, name)
        ran[fam] += 1
        if fam == "mfma3":
            mfma3_bits[name[len("mfma3_"):]] = _np(out).view(np.uint32)
        if c.Cin == 3 and fam in ("auto", "direct"):      # without a residual the RGB conv takes the stem kernel
            rc, out = run_conv(d["x"], d["w"], cfg=cfg, **ex_args(c, fam, residual=False))
            ran_ok(rc, c, fam, name + " (stem)")
            hold(_np(out), *B["nores"], fam, c, name + " (stem)")
    # ---- ssd_conv2d_planes: dma3_* (bitwise the mfma3_* twin), dmab_*
    for cfg, name in dma_configs(b"dma3_"):
        rc, out, joined = run_conv_planes(d["x"], d["w"], 3, cfg, d["scale"], d["shift"], d["res"], c.stride, c.dil, c.pads, act=2)
        if gc.must_refuse(c, "dma3"):
            refused(rc, c, "dma3", name)
            continue
        ran_ok(rc, c, "dma3", name)
        o = _np(out)
        hold(o, *B["dma3"], "dma3", c, name)
        if joined is not None:
            np.testing.assert_array_equal(joined.view(np.uint32), o.view(np.uint32), err_msg="%s %s plane output" % (c.name, name))
        twin = mfma3_bits.get(name[len("dma3_"):])
        if twin is not None:
            np.testing.assert_array_equal(o.view(np.uint32), twin, err_msg="%s %s vs its mfma3 twin" % (c.name, name))
            ran["twin"] += 1
        ran["dma3"] += 1
    for cfg, name in dma_configs(b"dmab_"):
        rc, out, joined = run_conv_planes(d["x"], d["w"], 1, cfg, None, None, None, c.stride, c.dil, c.pads)
        if gc.must_refuse(c, "dmab"):
            refused(rc, c, "dmab", name)
            continue
        ran_ok(rc, c, "dmab", name)
        hold(_np(out), *B["dmab"], "dmab", c, name)
        if joined is not None:
            np.testing.assert_array_equal(joined, bf16_round(_np(out)), err_msg="%s %s plane output" % (c.name, name))
        ran["dmab"] += 1
    # ---- ssd_conv2d_planes_f16x2: dmah_*
    pw = pack_weights(d["w"])
    for cfg, name in dma_configs(b"dmah_"):
        rc, out, joined = run_conv_h(d["x"], d["w"], cfg, d["scale"], d["shift"], d["res"], c.stride, c.dil, c.pads, act=2, packed_w=pw)
        if gc.must_refuse(c, "dmah"):
            refused(rc, c, "dmah", name)
            continue
        ran_ok(rc, c, "dmah", name)
        hold(_np(out), *B["dmah"], "dmah", c, name)
        if joined is not None:
            expect_plane_output(joined, _np(out))
        ran["dmah"] += 1
    # ---- ssd_conv2d_wino
    wn = Wino(c)
    for cfg in range(lib.ssd_conv_wino_num_configs()):
        for sk in (1, 2, 3):
            if sk > max(1, c.Cin // 16):
                continue
            rc, out = wn.run(cfg, sk)
            tag = "wino config %d split %d" % (cfg, sk)
            if gc.must_refuse(c, "wino"):
                refused(rc, c, "wino", tag)
                continue
            ran_ok(rc, c, "wino", tag)
            hold(_np(out), *B["wino"], "wino", c, tag)
            ran["wino"] += 1
    for fam in gc.FAMILIES:
        assert (ran[fam] == 0) == gc.must_refuse(c, fam), (c.name, fam, dict(ran))
    if not gc.must_refuse(c, "dma3"):
        assert ran["twin"] >= 4, dict(ran)


def layout(c, which):
    """(batch stride, pixel stride, offset, total), flat indices [B, Ho Wo, Cout] of the destination.  Layout 1: pixel
    stride Cout + 12, offset 16 floats, batch stride padded by 80 floats -- all multiples of 4: the vector stores.
    Layout 2: pixel stride Cout + 1, offset 13: ``vec_store`` off, the scalar stores."""
    Ho, Wo = gc.out_hw(c)
    P = Ho * Wo
    if which == 1:
        ps, off = c.Cout + 12, 16
        bs = P * ps + 80
        assert ps % 4 == 0 and bs % 4 == 0
    else:
        ps, off = c.Cout + 1, 13
        bs = P * ps + 7
    total = off + c.B * bs + 64
    idx = off + np.arange(c.B)[:, None, None] * bs + np.arange(P)[None, :, None] * ps + np.arange(c.Cout)[None, None, :]
    assert idx.max() < total - 64
    return (bs, ps, off, total), idx


def fresh_canvas(total):
    import ssd_hip as h
    return torch.full((total,), PAYLOAD, dtype=torch.int32, device=h.device()).view(torch.float32)


def hold_canvas(canvas, idx, ref, bar, scale, fam, c, tag):
    u = canvas.cpu().numpy().view(np.uint32)
    inside = np.zeros(u.size, bool)
    inside[idx.ravel()] = True
    stray = np.flatnonzero(~inside & (u != PAYLOAD))
    assert stray.size == 0, "%s %s %s: %d words outside the destination were written, first at %d" % (c.name, fam, tag, stray.size, stray[0])
    hold(u.view(np.float32)[idx], ref.reshape(idx.shape), bar, scale, fam, c, tag)


@pytest.mark.parametrize("which", [1, 2], ids=["vector", "scalar"])
@pytest.mark.parametrize("name", ["wide_same", "tall_s2"])
def test_strided_destination_every_config_and_split(name, which):
    import ssd_hip as h
    lib = h.lib()
    c = gc.BY_NAME[name]
    d = gc.data(c)
    B = bars(c)
    strides, idx = layout(c, which)
    ran = collections.Counter()
    for cfg, cname, fam in ex_configs():
        if gc.must_refuse(c, fam):
            continue
        for sk in ((1,) if fam in ("auto", "skinny", "direct") else (1, 2, 3)):
            canvas = fresh_canvas(strides[3])
            rc, _ = run_conv(d["x"], d["w"], cfg=cfg, split_k=sk, out_strides=strides, canvas=canvas, **ex_args(c, fam))
            tag = "%s split %d layout %d" % (cname, sk, which)
            ran_ok(rc, c, fam, tag)
            hold_canvas(canvas, idx, *B[fam], fam, c, tag)
            ran[fam] += 1
    pw = pack_weights(d["w"])
    for fam, np_ in (("dma3", 3), ("dmab", 1), ("dmah", 2)):
        epi = (None, None, None) if fam == "dmab" else (d["scale"], d["shift"], d["res"])
        for cfg, cname in dma_configs(fam.encode() + b"_"):
            for sk in (1, 2, 3):
                canvas = fresh_canvas(strides[3])
                kw = dict(stride=c.stride, dil=c.dil, pads=c.pads, act=0 if fam == "dmab" else 2, split_k=sk, want_planes=False,
                          out_strides=strides, canvas=canvas)
                if fam == "dmah":
                    rc, _, _ = run_conv_h(d["x"], d["w"], cfg, *epi, packed_w=pw, **kw)
                else:
                    rc, _, _ = run_conv_planes(d["x"], d["w"], np_, cfg, *epi, **kw)
                tag = "%s split %d layout %d" % (cname, sk, which)
                ran_ok(rc, c, fam, tag)
                hold_canvas(canvas, idx, *B[fam], fam, c, tag)
                ran[fam] += 1
    if not gc.must_refuse(c, "wino"):
        wn = Wino(c)
        for cfg in range(lib.ssd_conv_wino_num_configs()):
            for sk in (1, 2, 3):
                canvas = fresh_canvas(strides[3])
                rc, _ = wn.run(cfg, sk, strides, canvas)
                tag = "wino config %d split %d layout %d" % (cfg, sk, which)
                ran_ok(rc, c, "wino", tag)
                hold_canvas(canvas, idx, *B["wino"], "wino", c, tag)
                ran["wino"] += 1
    for fam in gc.FAMILIES:
        assert (ran[fam] == 0) == gc.must_refuse(c, fam), (fam, dict(ran))


def test_plane_output_needs_a_dense_destination():
    """The plane entry points write an output as planes beside a DENSE fp32 output only: with a strided one they answer
    SSD_E_INVALID and touch nothing (which is why the strided runs above ask for no plane output)."""
    import ssd_hip as h
    lib = h.lib()
    c = gc.BY_NAME["dil2"]          # Cout = 64: whole 32-channel slices, the helpers allocate the plane output
    d = gc.data(c)
    strides, idx = layout(c, 1)
    for fam in ("dma3", "dmah"):
        cfg, name = dma_configs(fam.encode() + b"_")[0]
        canvas = fresh_canvas(strides[3])
        kw = dict(stride=c.stride, dil=c.dil, pads=c.pads, act=2, want_planes=True, out_strides=strides, canvas=canvas)
        if fam == "dmah":
            rc, _, _ = run_conv_h(d["x"], d["w"], cfg, d["scale"], d["shift"], d["res"], **kw)
        else:
            rc, _, _ = run_conv_planes(d["x"], d["w"], 3, cfg, d["scale"], d["shift"], d["res"], **kw)
        assert rc == -1 and b"dense" in lib.ssd_last_error(), (name, rc, lib.ssd_last_error())
        assert (canvas.cpu().numpy().view(np.uint32) == PAYLOAD).all(), name


def test_error_record():
    """The measured worst err / scale per family and case of the runs above (scale: max(1, max |ref|), or max |ref| of the
    rounded-operand reference for bf16 / dmab): a record, no bar.  ``SSD_CONV_GEOMETRY_RECORD=<file>`` also writes it there."""
    lines = ["worst max-abs-error / scale per (family, case); '-' = refused (conv_geometry_cases.REFUSALS) or not run",
             "%-12s" % "case" + "".join("%10s" % f for f in gc.FAMILIES)]
    for c in gc.CASES:
        row = "%-12s" % c.name
        for f in gc.FAMILIES:
            row += "%10s" % ("%.2e" % RECORD[(f, c.name)] if (f, c.name) in RECORD else "-")
        lines.append(row)
    text = "\n".join(lines) + "\n"
    print(text)
    path = os.environ.get("SSD_CONV_GEOMETRY_RECORD")
    if path:
        with open(path, "w") as f:
            f.write(text)
    assert all(v == v for v in RECORD.values())
