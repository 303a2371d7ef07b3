"""Writes tests/golden/jpeg.npz: for every case of tests/jpeg_cases.py the JPEG bytes Pillow wrote and the RGB pixels
Pillow decodes from them (``Image.open(...).convert("RGB")``).  The decoder tests compare against these bytes, so the
fixture pins the arithmetic of the library that wrote it: Pillow 12.2.0 with libjpeg-turbo 3.1.4.1 (recorded in the
file as ``versions``).  Run from the repository root: ``python tests/golden/make_jpeg_golden.py``."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases as jc  # noqa: E402


def main():
    import PIL
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the fixture is libjpeg-turbo's arithmetic"
    arrays = {"versions": np.array("Pillow %s / libjpeg-turbo %s" % (PIL.__version__, features.version_feature("libjpeg_turbo")))}
    for name, (h, w), mode, kind, options in jc.cases():
        blob = jc.encode(jc.content(h, w, mode, kind), mode, options)
        arrays["jpeg_" + name] = np.frombuffer(blob, np.uint8)
        arrays["rgb_" + name] = jc.pillow_decode(blob)
    np.savez_compressed(jc.GOLDEN, **arrays)
    print("%s: %d cases, %d bytes, %s" % (jc.GOLDEN, len(jc.cases()), os.path.getsize(jc.GOLDEN), arrays["versions"]))


if __name__ == "__main__":
    main()
