"""Target assignment strategies on the GPU: ``ssd_match_encode_cfg`` against the NumPy oracle of tests/match_cases.py.
Exact: label_idx, match_idx and the one-hot tensor (IoU and distance bits are the oracle's by construction, so ties are part
of the cases, not something to stay away from).  Deltas: within ``test_bbox_gpu.TOL`` of
``oracle.bbox_oracle.get_deltas_from_bboxes`` on the oracle's chosen boxes.  Every case runs twice: identical bits."""
import os

import numpy as np
import pytest
import torch

import helpers
import match_cases as mc
from test_bbox_gpu import TOL

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _np(t):
    return t.detach().cpu().numpy()


def run_cfg(cfg, priors, gt, gl, poison=0):
    """The four outputs of one ``ssd_match_encode_cfg`` call (NumPy); the workspace is filled with ``poison`` first."""
    import ssd_hip as h
    lib = h.lib()
    B, G = gl.shape
    N = priors.shape[0]
    p, g, l = h.to_dev(np.array(priors)), h.to_dev(np.array(gt)), h.to_dev(np.array(gl), torch.int32)      # the cases are read-only
    dev = p.device
    deltas = torch.full((B, N, 4), 7.0, dtype=torch.float32, device=dev)
    onehot = torch.full((B, N, mc.L), 7.0, dtype=torch.float32, device=dev)
    lab = torch.full((B, N), 77, dtype=torch.int32, device=dev)
    am = torch.full((B, N), 77, dtype=torch.int32, device=dev)
    nbytes = lib.ssd_match_encode_cfg_workspace_bytes(B, N, G, cfg)
    ws = torch.full((max(nbytes, 16),), poison, dtype=torch.uint8, device=dev)
    var_p, _keep = h.host4(helpers.VARIANCES)
    h.check(lib.ssd_match_encode_cfg(h.ptr(p), h.ptr(g), h.ptr(l), var_p, cfg, B, N, G, mc.L, h.ptr(deltas), h.ptr(lab), h.ptr(am),
                                     h.ptr(onehot), h.ptr(ws), nbytes, h.stream()), "ssd_match_encode_cfg")
    torch.cuda.synchronize()
    return _np(deltas), _np(onehot), _np(lab), _np(am)


def config_of(case):
    import ssd_hip as h
    return h.match_config(case.strategy, case.iou_threshold, case.topk or 9, case.level_start)


@pytest.mark.parametrize("name", mc.names())
def test_strategy_against_the_oracle(name):
    case = mc.by_name(name)
    want = mc.oracle(case)
    cfg = config_of(case)
    d, oh, lab, am = run_cfg(cfg, case.priors, case.gt, case.gl)
    print("%s: %d positives, %d forced, max |ddelta| %.3g" % (
        name, int((want.label_idx > 0).sum()), sum(len(f) for f in want.forced), np.abs(d - want.deltas).max() if d.size else 0.0))
    np.testing.assert_array_equal(lab, want.label_idx)
    np.testing.assert_array_equal(am, want.match_idx)
    np.testing.assert_array_equal(oh, want.onehot)
    np.testing.assert_allclose(d, want.deltas, atol=TOL, rtol=0)
    again = run_cfg(cfg, case.priors, case.gt, case.gl, poison=0xA5)         # whatever the workspace held
    for a, b in zip((d, oh, lab, am), again):
        assert a.tobytes() == b.tobytes(), "a second run gives other bits"


def test_max_iou_through_cfg_is_ssd_match_encode():
    import ssd_hip as h
    from utils import train_utils
    z = np.load(os.path.join(GOLD, "match.npz"))
    p = mc.priors_of("mobilenet_v2")
    hp = helpers.hyper_params()
    old = [_np(t) for t in train_utils.calculate_actual_outputs(p, z["gt"], z["gl"], hp, return_indices=True)]
    d, oh, lab, am = run_cfg(h.match_config("max_iou", 0.5), p, z["gt"], z["gl"])
    for a, b in zip(old, (d, oh, lab, am)):
        assert a.tobytes() == b.tobytes()
    new = [_np(t) for t in train_utils.calculate_actual_outputs(p, z["gt"], z["gl"], dict(hp, match_strategy="max_iou"),
                                                                return_indices=True)]
    for a, b in zip(old, new):
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(lab, z["label_idx"])
    np.testing.assert_array_equal(am, z["match_idx"])


@pytest.mark.parametrize("name", ["real_mobilenet_v2", "atss_real_top9"])
def test_hyper_parameter_keys_select_the_strategy(name):
    """``calculate_actual_outputs`` behind ``match_strategy`` / ``match_topk``: ATSS's levels come from the feature maps."""
    from utils import train_utils
    case = mc.by_name(name)
    want = mc.oracle(case)
    hp = dict(helpers.hyper_params("mobilenet_v2"), match_strategy=case.strategy)
    if case.strategy == "atss":
        hp["match_topk"] = case.topk
    d, oh, lab, am = (_np(t) for t in train_utils.calculate_actual_outputs(case.priors, case.gt, case.gl, hp, return_indices=True))
    np.testing.assert_array_equal(lab, want.label_idx)
    np.testing.assert_array_equal(am, want.match_idx)
    np.testing.assert_array_equal(oh, want.onehot)
    np.testing.assert_allclose(d, want.deltas, atol=TOL, rtol=0)


def test_limits_are_refused_before_any_launch():
    import ssd_hip as h
    lib = h.lib()
    p = h.to_dev(mc.priors_of("mobilenet_v2")[:300])
    G = 3073                                                                  # ssd_match_encode's LDS limit is 3072 rows
    gt = torch.zeros((1, G, 4), device=p.device)
    gl = torch.zeros((1, G), dtype=torch.int32, device=p.device)
    out = torch.full((1, 300, 4), 7.0, device=p.device)
    idx = torch.full((2, 300), 77, dtype=torch.int32, device=p.device)
    ws = torch.zeros((300 * 8,), dtype=torch.uint8, device=p.device)
    var_p, _keep = h.host4(helpers.VARIANCES)
    for cfg in (h.match_config("max_iou"), h.match_config("bipartite"), h.match_config("atss", level_start=[0, 300])):
        rc = lib.ssd_match_encode_cfg(h.ptr(p), h.ptr(gt), h.ptr(gl), var_p, cfg, 1, 300, G, mc.L, h.ptr(out), h.ptr(idx[0]),
                                      h.ptr(idx[1]), None, h.ptr(ws), ws.numel(), h.stream())
        assert rc == -3 and b"LDS" in lib.ssd_last_error(), (cfg.strategy, rc)
    cfg = h.match_config("bipartite")
    rc = lib.ssd_match_encode_cfg(h.ptr(p), h.ptr(gt), h.ptr(gl), var_p, cfg, 1, 300, 5, mc.L, h.ptr(out), h.ptr(idx[0]),
                                  h.ptr(idx[1]), None, h.ptr(ws), 300 * 4 + 5 * 8 - 1, h.stream())
    assert rc == -1 and b"workspace" in lib.ssd_last_error()
    torch.cuda.synchronize()
    assert (_np(out) == 7).all() and (_np(idx) == 77).all()


def test_trainer_with_bipartite_matching(tmp_path, monkeypatch, capsys):
    """trainer.main on the synthetic stream with SSD_TRAINER_MATCH=bipartite, one epoch of two steps: finite losses, and the
    first batch's positives are the oracle's."""
    import importlib
    from utils import train_utils
    monkeypatch.chdir(tmp_path)
    for k, v in (("SSD_TRAINER_EPOCHS", "1"), ("SSD_TRAINER_STEPS", "2"), ("SSD_TRAINER_BATCH", "4"), ("SSD_TRAINER_AUGMENT", "0"),
                 ("SSD_TRAINER_MATCH", "bipartite")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("SSD_TRAINER_MATCH_TOPK", raising=False)
    monkeypatch.delenv("SSD_VOC_DIR", raising=False)
    table = dict(train_utils.get_hyper_params("mobilenet_v2"))
    seen = []
    real = train_utils.calculate_actual_outputs

    def spy(prior_boxes, gt_boxes, gt_labels, hyper_params, *a, **kw):
        out = real(prior_boxes, gt_boxes, gt_labels, hyper_params, *a, **kw)
        if not seen:
            host = lambda x: _np(x) if isinstance(x, torch.Tensor) else np.asarray(x)
            seen.append((host(prior_boxes).astype(np.float32), host(gt_boxes).astype(np.float32), host(gt_labels).astype(np.int32),
                         dict(hyper_params), _np(out[1])))
        return out
    monkeypatch.setattr(train_utils, "calculate_actual_outputs", spy)
    trainer = importlib.import_module("trainer")
    hist = trainer.main(["--backbone", "mobilenet_v2"])
    out = capsys.readouterr().out
    assert "target assignment: bipartite" in out and "Epoch 1/1" in out
    assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"]).all() and np.isfinite(hist["val_loss"]).all()
    priors, gt, gl, hp, onehot = seen[0]
    assert hp["match_strategy"] == "bipartite"
    case = mc.Case("trainer/first_batch", 1000, "bipartite", priors, gt, gl, hp["iou_threshold"], 0, None)
    want = mc.oracle(case)
    positives = int(onehot[..., 1:].sum())
    plain = mc.oracle(case._replace(name="trainer/first_batch/max_iou", strategy="max_iou"))
    print("first batch: %d positives (%d under max_iou), %d forced" % (positives, int((plain.label_idx > 0).sum()),
                                                                       sum(len(f) for f in want.forced)))
    assert positives == int((want.label_idx > 0).sum())
    np.testing.assert_array_equal(onehot, want.onehot)
    after = train_utils.get_hyper_params("mobilenet_v2")
    assert not [k for k in after if k.startswith("match")] and set(after) - {"total_labels"} == set(table) - {"total_labels"}
