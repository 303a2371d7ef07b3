"""Writes tests/golden/lanczos.npz: ``PIL.Image.resize(..., Image.LANCZOS)`` executed on the small seeded sources of
tests/lanczos_cases.py (downscale, upscale, mixed, one axis equal, both equal).  The committed file pins Pillow's bits
independently of the Pillow installed where the tests run; the Pillow version that wrote it is recorded inside.
Usage: python tests/golden/make_lanczos_golden.py"""
import os
import sys

import numpy as np
import PIL

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lanczos_cases as lc  # noqa: E402

if __name__ == "__main__":
    data = {"pillow_version": np.array(PIL.__version__)}
    for name, (h, w), content in lc.FIXTURE_SOURCES:
        src = lc.image(h, w, content)
        data["src_" + name] = src
        for oh, ow in lc.FIXTURE_OUT:
            data["out_%s_%dx%d" % (name, oh, ow)] = lc.pillow(src, oh, ow)
    np.savez_compressed(lc.GOLDEN, **data)
    print("wrote %s (%d bytes, %d arrays, Pillow %s)" % (lc.GOLDEN, os.path.getsize(lc.GOLDEN), len(data), PIL.__version__))
