"""A partial kernel table times exactly what it lacks: the contract behind ``tools/make_tuning_tables.py --retime`` and
every cache miss.  Three lines are taken out of a complete table -- a running conv whose input has no other reader, a conv
that is fused away under the table's routes, an image line -- and the finalize must time those three choices, keep every
line it was handed as it is, and put each missing name back exactly once.  None of the three reads a tensor that a kept
"dmah_*" line reads, so no kept line can legitimately change."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

DROPPED = ("extra2_2", "block_7_expand", "block_16_fused")


def _np(t):
    return t.detach().cpu().numpy()


def _close(a, b, tol):
    # tests/test_conv_gpu.py::_close: relative to the tensor's range
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, "max abs err %.3e (scale %.3g)" % (err, scale)


def _without(table, names):
    return [l for l in table.splitlines() if l.split()[0] not in names]


def test_partial_table_times_exactly_what_it_lacks():
    import ssd_hip
    import tuning
    from models.ssd_mobilenet_v2 import get_model
    lib = ssd_hip.lib()
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.images(3, 300, seed=5)

    def model(table):
        m = get_model(hp, max_batch=3)
        m.set_weights(w)
        m.set_tuning(table)
        d, p = m(x)
        return m, _np(d), _np(p)

    # A: the shipped table, nothing timed
    key = tuning.table_key("mobilenet_v2", 300, hp["total_labels"], hp["aspect_ratios"], 3)
    shipped = tuning.load_shipped(key)
    assert shipped is not None, "no shipped table %s" % key
    a, da, pa = model(shipped)
    assert a.tuning_info["choices_timed_on_device"] == 0
    full = a.get_tuning()

    # B: the same table minus three lines
    handed = _without(full, DROPPED)
    assert len(handed) == len(full.splitlines()) - 3 and "__launch graph" in handed[-1]
    n_conv = sum(1 for l in handed if l.split()[1] not in ("image", "graph"))
    b, db, pb = model("".join(l + "\n" for l in handed))
    assert b.tuning_info["layers_from_table"] == n_conv
    assert b.tuning_info["choices_timed_on_device"] == 3
    got = b.get_tuning()
    assert _without(got, DROPPED) == handed
    names = {lib.ssd_conv_config_name(c).decode() for c in range(lib.ssd_conv_num_configs())}
    for name in DROPPED:
        lines = [l.split() for l in got.splitlines() if l.split()[0] == name]
        assert len(lines) == 1 and len(lines[0]) == 3, (name, lines)
        _, cfg, num = lines[0]
        if name.endswith("_fused"):
            assert cfg == "image" and int(num) in (0, 1, 2), lines[0]
        else:
            assert cfg in names and 1 <= int(num) <= 64, lines[0]
    assert np.abs(pa - pb).max() <= 1e-4
    _close(da, db, tol=1e-4)

    # C: B's table handed on: nothing timed, the same text, the same bits
    c, dc, pc = model(got)
    assert c.tuning_info["choices_timed_on_device"] == 0
    assert c.get_tuning() == got
    np.testing.assert_array_equal(pb, pc)
    np.testing.assert_array_equal(db, dc)
