"""``image_forms(B)`` over the whole option matrix of tests/image_form_cases.py against the table recorded before the
forms were decided in one place (tests/golden/image_forms.json): the plan reports, cell for cell, what the scattered
rules reported -- and since the launcher now runs the plan and nothing else, what runs.  No forward: the query is host
arithmetic; eight finalizes on a pinned table, none of them timing anything."""
import pytest

import image_form_cases as ic

pytestmark = pytest.mark.gpu


def test_every_cell_of_the_matrix_reproduces_the_recorded_forms():
    want = ic.load_golden()
    got = ic.table()
    assert sorted(got) == sorted(want)
    assert len(got) == len(ic.nets()) * len(ic.settings()) * len(ic.BATCHES) == 256
    assert not ic.EXCEPTIONS        # (a rule listed there would need its bitwise test here)
    bad = ["%s: %s, recorded %s" % (k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    assert not bad, "\n".join(bad)
    # the matrix does reach every form, and the fp16 pair only where every rule of the plan allows it
    assert {f for v in got.values() for f in v} == {0, 1, 2, 3}
    for k, v in got.items():
        if 2 in v:
            assert k.startswith("fp32 f16x2=1 pin=2 v2=1 "), k
