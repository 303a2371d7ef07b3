"""Which numeric form of the whole-image block kernel runs blocks 7 - 16 of MobileNetV2-SSD300 under every option that bears
on it: the matrix behind tests/test_image_forms_gpu.py, tests/golden/image_forms.json and tools/image_form_matrix.py.

Eight nets (21 labels, seeded ``synthetic_weights``, max_batch 64, the shipped b64 table of their precision with every
``block_k_fused image`` line pinned -- no choice is timed):

    precision fp32 / bf16   x   image_f16x2 0 / 1   x   table lines ``image 1`` / ``image 2``

and on each the options that need no refinalize, image_v2 0 / 1 x image_ticket 0 / 1 x lanes_hint 1 / 8, read through
``image_forms(B)`` at B = 1 (twelve groups), 3, 28 (at lanes_hint 8 the smallest batch with one group per image:
28 * 8 * 8 >= 7/8 of 2048) and 64.  The query is host arithmetic: no forward runs.

The golden table was recorded by ``python tests/image_form_cases.py`` on the commit BEFORE the forms were decided in one
place (csrc/ssd_imgblock.hip, image_block_plan); that commit's launcher could still change a block's form after
``image_forms`` had answered (split-bf16 -> fp32 MFMA where the split form's LDS tiles did not fit).  The enumeration of
every block shape, form and group count (profiles/HISTORY.md, "One plan for the whole-image blocks") found no tuple where
that fired, so EXCEPTIONS is empty: every cell must be reproduced."""
import itertools
import json
import os

import helpers

BLOCKS = ["block_%d_fused" % k for k in range(7, 17)]
PRECISIONS = ("fp32", "bf16")
F16X2 = (0, 1)
PINS = (1, 2)
IMAGE_V2 = (0, 1)
IMAGE_TICKET = (0, 1)
LANES_HINT = (1, 8)
BATCHES = (1, 3, 28, 64)
MAX_BATCH = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_forms.json")

# Rules (not cells) under which the recorded form was not the form that ran: (predicate over a cell's settings, reason).
EXCEPTIONS = []


def nets():
    return list(itertools.product(PRECISIONS, F16X2, PINS))


def settings():
    return list(itertools.product(IMAGE_V2, IMAGE_TICKET, LANES_HINT))


def cell_key(precision, f16, pin, v2, ticket, lanes, B):
    return "%s f16x2=%d pin=%d v2=%d ticket=%d lanes=%d B=%d" % (precision, f16, pin, v2, ticket, lanes, B)


def pinned_table(precision, pin):
    """The shipped b64 table of the precision (header dropped), every whole-image line pinned to ``image <pin>``."""
    import tuning
    hp = helpers.hyper_params("mobilenet_v2")
    key = tuning.table_key("mobilenet_v2", hp["img_size"], hp["total_labels"], hp["aspect_ratios"], MAX_BATCH)
    text = tuning.load_shipped(key + ("_bf16" if precision == "bf16" else ""))
    assert text is not None, key
    lines = tuning.body(text).splitlines()
    assert [l.split()[0] for l in lines if " image " in l] == BLOCKS
    return "".join(((l.rsplit(" ", 1)[0] + " %d" % pin) if " image " in l else l) + "\n" for l in lines)


def finalized_model(precision, f16, pin, weights):
    from models.ssd_mobilenet_v2 import get_model
    m = get_model(helpers.hyper_params("mobilenet_v2"), max_batch=MAX_BATCH, precision=precision)
    m.set_weights(weights)
    m.set_option("image_f16x2", f16)
    m.set_tuning(pinned_table(precision, pin))
    m._ensure(MAX_BATCH)
    assert m.tuning_info["source"] == "explicit" and m.tuning_info["choices_timed_on_device"] == 0, m.tuning_info
    return m


def apply(m, v2, ticket, lanes):
    m.set_option("image_v2", v2)
    m.set_option("image_ticket", ticket)
    m.set_option("lanes_hint", lanes)


def forms_of(m, B):
    forms = m.image_forms(B)
    assert sorted(forms) == sorted(BLOCKS), forms
    return [forms[n] for n in BLOCKS]


def table():
    """cell key -> the forms of blocks 7 - 16."""
    w = helpers.synthetic_weights("mobilenet_v2", helpers.hyper_params("mobilenet_v2"))
    out = {}
    for precision, f16, pin in nets():
        m = finalized_model(precision, f16, pin, w)
        for v2, ticket, lanes in settings():
            apply(m, v2, ticket, lanes)
            for B in BATCHES:
                out[cell_key(precision, f16, pin, v2, ticket, lanes, B)] = forms_of(m, B)
        del m
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":          # records the golden table: run on the commit whose answers are the reference
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [repo, os.path.join(repo, "tf-ssd_amd")]
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(table().items())) + "\n}\n")
