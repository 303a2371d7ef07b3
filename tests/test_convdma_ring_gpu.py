"""The three-stage LDS ring of the one-k-step ``dmah_*`` tiles (csrc/ssd_convdma.hip) against the two-stage loop it replaces.

Both loops issue every accumulator's MFMAs in the same order, so their outputs must be BITWISE equal: every ``dmah_*``
name without ``_ks2`` runs each case through ``ssd_conv2d_planes_f16x2`` with ``ssd_conv_desc::dma_two_stage`` 0 (the
ring) and 1 (the two-stage loop), three launches each -- a stage refilled too early, or read before its copies landed,
depends on timing -- and all six outputs must agree bit for bit.  Each case is also held to the float64 oracle
(oracle/conv_oracle.py) at the bar tests/test_conv_geometry_gpu.py uses for the family: 1e-4 max(1, max |ref|), epilogue on
(scale, shift, ReLU6, residual).

Cases (B = 2; M = 70 rows of a 64- to 256-row tile: an M tail, rows of both images in one tile):

* 3x3, pad 1, map 7 x 5: Cin 32 / 96 (9 / 27 K tiles), Cout 24 (N tail) / 150, split-K 1, 2, 7 -- split 7 over 9 tiles
  leaves three empty K ranges, whose workgroups must still pass the barriers and write zero partials;
* 1x1, same map: Cin 32, 64, 96 = 1, 2, 3 K tiles (shorter than, equal to and just past the ring's prologue), split-K 1, 2;
* 3x3 stride 2, pads (0, 1, 0, 1), 10 x 10 map, Cin 64, Cout 40: the geometry of extra1_2;
* the MobileNetV2 fp32 net at B = 2: option ``dma_ring`` 0 against 1, ``predict`` outputs bitwise equal and the same
  ``ssd_net_layer_config`` strings.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers
from oracle import conv_oracle as cv
from test_conv_gpu import guarded, _np
from test_convdma_gpu import make_planes, dma_configs
from test_f16x2_gpu import pack_weights

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

Case = collections.namedtuple("Case", "name seed B H W Cin Cout k stride pads splits")

CASES = [Case("3x3_c%d_n%d" % (cin, cout), 200 + i, 2, 7, 5, cin, cout, 3, 1, (1, 1, 1, 1), (1, 2, 7))
         for i, (cin, cout) in enumerate([(32, 24), (32, 150), (96, 24), (96, 150)])] + \
        [Case("1x1_c%d" % cin, 210 + i, 2, 7, 5, cin, 150, 1, 1, (0, 0, 0, 0), (1, 2)) for i, cin in enumerate([32, 64, 96])] + \
        [Case("extra1_2_s2", 220, 2, 10, 10, 64, 40, 3, 2, (0, 1, 0, 1), (1,))]


@functools.lru_cache(maxsize=None)
def data(c):
    """Inputs (clip(3 N(0,1), 0, 6): ReLU6-like, inside the fp16 pair's range contract) and the float64 reference of a
    case, computed once and read-only."""
    rng = np.random.default_rng(c.seed)
    x = np.clip(3.0 * rng.standard_normal((c.B, c.H, c.W, c.Cin)), 0.0, 6.0).astype(np.float32)
    w = (rng.standard_normal((c.k, c.k, c.Cin, c.Cout)) / np.sqrt(c.k * c.k * c.Cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, c.Cout).astype(np.float32)
    shift = rng.uniform(-0.5, 0.5, c.Cout).astype(np.float32)
    conv = cv.conv2d_f64(x, w, c.stride, 1, c.pads)
    res = rng.standard_normal(conv.shape).astype(np.float32)
    d = dict(x=x, w=w, scale=scale, shift=shift, res=res, ref=cv.epilogue_f64(conv, scale, shift, cv.ACT_RELU6, res))
    for v in d.values():
        v.setflags(write=False)
    return d


def ring_configs():
    return [(cfg, name) for cfg, name in dma_configs(b"dmah_") if not name.endswith("_ks2")]


class Runner:
    """One case on the device: planes, packed weights and epilogue vectors made once; ``run`` launches one config."""

    def __init__(self, c):
        import ssd_hip as h
        self.h, self.lib, self.c = h, h.lib(), c
        d = data(c)
        rc, self.packed, self.wpl, self.k = pack_weights(d["w"])
        assert rc == 0, self.lib.ssd_last_error()
        self.keep, self.p0, self.pstride = make_planes(d["x"], 2)
        self.sd, self.hd, self.rd = guarded(d["scale"]), guarded(d["shift"]), guarded(d["res"])
        self.shape = d["ref"].shape

    def run(self, cfg, split_k, two_stage):
        h, c = self.h, self.c
        desc = h.ConvDesc(c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.k, c.stride, 1, c.pads[0], c.pads[2], c.pads[1], c.pads[3], 2, 1,
                          two_stage)
        out = torch.full(self.shape, float("nan"), dtype=torch.float32, device=self.packed.device)
        ws = torch.full((split_k * out.numel(),), float("nan"), dtype=torch.float32, device=out.device) if split_k > 1 else None
        rc = self.lib.ssd_conv2d_planes_f16x2(ctypes.byref(desc), h.vp(self.p0), self.pstride, h.ptr(self.packed),
                                              h.vp(self.wpl.data_ptr()), self.k, h.ptr(self.sd), h.ptr(self.hd), h.ptr(self.rd),
                                              h.ptr(out), 0, 0, None, 0, cfg, split_k, h.ptr(ws), h.stream())
        assert rc == 0, "%s config %d split %d two_stage %d: rc %d, %r" % (c.name, cfg, split_k, two_stage, rc, self.lib.ssd_last_error())
        return _np(out)


def test_the_descriptor_mirror_has_the_switch():
    import ssd_hip as h
    assert h.ConvDesc._fields_[-1][0] == "dma_two_stage"
    assert h.ConvDesc(*range(15)).dma_two_stage == 0          # a zero-filled tail: the ring
    assert len(ring_configs()) >= 14


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_ring_equals_two_stage_bitwise_and_holds_the_oracle(c):
    d = data(c)
    r = Runner(c)
    scale = max(1.0, float(np.abs(d["ref"]).max()))
    worst = 0.0
    for cfg, name in ring_configs():
        for sk in c.splits:
            first = None
            for two_stage in (0, 1):
                for launch in range(3):
                    bits = r.run(cfg, sk, two_stage).view(np.uint32)
                    if first is None:
                        first = bits
                    else:
                        np.testing.assert_array_equal(bits, first, err_msg="%s %s split %d: two_stage %d launch %d differs from the ring's first launch"
                                                      % (c.name, name, sk, two_stage, launch))
            err = float(np.abs(first.view(np.float32).astype(np.float64) - d["ref"]).max())
            worst = max(worst, err)
            assert err <= 1e-4 * scale, "%s %s split %d: max abs err %.3e, bar %.3e" % (c.name, name, sk, err, 1e-4 * scale)
    print("%s: worst max-abs error %.3e (bar %.3e)" % (c.name, worst, 1e-4 * scale))


def test_net_option_dma_ring_keeps_every_bit():
    from models.ssd_mobilenet_v2 import get_model
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.block_test_images(2, 300)
    outs, cfgs = {}, {}
    for ring in (1, 0):
        m = get_model(hp, max_batch=2)
        m.set_weights(w)
        m.set_option("dma_ring", ring)
        runs = [m.predict(x, batch_size=2) for _ in range(3)]
        for dd, pp in runs[1:]:
            np.testing.assert_array_equal(dd.view(np.uint32), runs[0][0].view(np.uint32))
            np.testing.assert_array_equal(pp.view(np.uint32), runs[0][1].view(np.uint32))
        outs[ring] = runs[0]
        cfgs[ring] = [l["config"] for l in m.layers(2)]
        del m
    assert np.isfinite(outs[1][0]).all() and np.isfinite(outs[1][1]).all()
    assert cfgs[1] == cfgs[0]
    assert any(cfg.startswith("dmah_") and not cfg.split("/")[0].split(" ")[0].endswith("_ks2") for cfg in cfgs[1]), cfgs[1]
    np.testing.assert_array_equal(outs[1][0].view(np.uint32), outs[0][0].view(np.uint32))
    np.testing.assert_array_equal(outs[1][1].view(np.uint32), outs[0][1].view(np.uint32))
