#!/usr/bin/env python
"""One line per cell of the whole-image form matrix (tests/image_form_cases.py) at B = 3: the forms ``image_forms``
reports for blocks 7 - 16 and the sha256 of ``deltas`` and ``probs`` of one forward on seeded input.  Evidence for a change
that must not move a bit: run it before and after and compare the two outputs line by line (profiles/image_plan_matrix_*.txt)."""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tf-ssd_amd"), os.path.join(REPO, "tests")]

import helpers                      # noqa: E402
import image_form_cases as ic       # noqa: E402

B = 3


def main():
    hp = helpers.hyper_params("mobilenet_v2")
    w = helpers.synthetic_weights("mobilenet_v2", hp)
    x = helpers.block_test_images(B, hp["img_size"])
    for precision, f16, pin in ic.nets():
        m = ic.finalized_model(precision, f16, pin, w)
        for v2, ticket, lanes in ic.settings():
            ic.apply(m, v2, ticket, lanes)
            forms = ic.forms_of(m, B)
            d, p = m(x)
            sha = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:32] for t in (d, p)]
            print("%-48s forms %s  deltas %s  probs %s" % (ic.cell_key(precision, f16, pin, v2, ticket, lanes, B),
                                                          "".join(str(f) for f in forms), sha[0], sha[1]), flush=True)
        del m


if __name__ == "__main__":
    main()
