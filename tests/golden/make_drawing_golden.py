"""Writes tests/golden/drawing.npz: the reference's PIL call sequence (``ImageDraw.text`` in the legacy bitmap font, then
``ImageDraw.rectangle(outline, width=3)``, per box) executed by Pillow on the small cases of tests/drawing_cases.py
named in ``FIXTURE_NAMES``, with their inputs.  The committed file pins Pillow's bytes independently of the Pillow
installed where the tests run; the Pillow version that wrote it is recorded inside.  Arrays and that string only.
Usage: python tests/golden/make_drawing_golden.py"""
import os
import sys

import numpy as np
import PIL

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drawing_cases as dc  # noqa: E402

if __name__ == "__main__":
    data = {"pillow_version": np.array(PIL.__version__)}
    by_name = {c["name"]: c for c in dc.cases()}
    for name in dc.FIXTURE_NAMES:
        case = by_name[name]
        for key in ("img", "boxes", "labels", "probs", "colors"):
            data["%s_%s" % (key, name)] = case[key]
        data["out_" + name] = dc.pillow(case)
    np.savez_compressed(dc.GOLDEN, **data)
    print("wrote %s (%d bytes, %d arrays, Pillow %s)" % (dc.GOLDEN, os.path.getsize(dc.GOLDEN), len(data), PIL.__version__))
