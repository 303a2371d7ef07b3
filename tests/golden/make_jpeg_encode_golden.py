"""Writes tests/golden/jpeg_encode.npz: the uint8 inputs of tests/jpeg_encode_cases.py and, for every case it keeps, the
bytes of ``PIL.Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s)``.  The encoder tests compare against these
bytes, so the fixture pins the arithmetic of the library that wrote it: Pillow 12.2.0 with libjpeg-turbo 3.1.4.1
(recorded in the file as ``versions``).  The whole candidate cross-product is checked against the NumPy restatement
first; the kept cases must exercise a ZRL symbol, a stuffed 0xFF, dummy blocks to the right, below and in the corner, and
a DC difference of category 11.  Run from the repository root: ``python tests/golden/make_jpeg_encode_golden.py``."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_encode_cases as jc  # noqa: E402


def main():
    import PIL
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the fixture is libjpeg-turbo's arithmetic"
    arrays = {"versions": np.array("Pillow %s / libjpeg-turbo %s" % (PIL.__version__, features.version_feature("libjpeg_turbo")))}
    inputs = jc.inputs()
    for name, key, q, s in jc.candidates():
        assert jc.restate(inputs[key], q, s) == jc.pillow_encode(inputs[key], q, s), name
    total = {}
    for name, key, q, s in jc.cases():
        blob = jc.pillow_encode(inputs[key], q, s)
        stats = {}
        assert jc.restate(inputs[key], q, s, stats) == blob, name
        for k, v in stats.items():
            total[k] = max(total.get(k, 0), v) if k == "max_dc_category" else total.get(k, 0) + v
        arrays["in_" + key] = inputs[key]
        arrays["jpeg_" + name] = np.frombuffer(blob, np.uint8)
    assert total["zrl"] >= 1 and total["stuffed"] >= 1, total
    assert total["dummy_right"] >= 1 and total["dummy_bottom"] >= 1 and total["dummy_corner"] >= 1, total
    assert total["max_dc_category"] == 11, total
    np.savez_compressed(jc.GOLDEN, **arrays)
    print("%s: %d of %d cases, %d bytes, %s, %s" % (jc.GOLDEN, len(jc.cases()), len(jc.candidates()) + 1,
                                                   os.path.getsize(jc.GOLDEN), arrays["versions"], total))


if __name__ == "__main__":
    main()
