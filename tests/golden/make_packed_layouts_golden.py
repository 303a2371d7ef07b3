"""Writes tests/golden/packed_layouts.json: what the four host packers of ``utils/data_utils.py`` produced for the cases
of tests/packed_layout_cases.py BEFORE the packers were folded onto one layout helper, at the commit recorded in the file
as ``commit``.  tests/test_packed_layout_cpu.py compares the current packers with it, so it is a record of that commit
and is never regenerated from later code.  It was run once, at that commit, from the repository root with the library
built: ``python tests/golden/make_packed_layouts_golden.py``."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "tf-ssd_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)
import packed_layout_cases as pc  # noqa: E402


def encode_fill_at_that_commit(host, layout, tables):
    """``jpeg_forward_batch``'s inline ``fill`` of that commit, which had no name to call it by."""
    desc = layout["desc"]
    host[:desc.nbytes] = desc.view(np.uint8)
    host[layout["tables_at"]:layout["total"]] = np.ascontiguousarray(tables, np.uint16).reshape(len(desc), 128).view(np.uint8).reshape(-1)


def main():
    from utils import data_utils
    assert not hasattr(data_utils, "_jpeg_encode_fill"), "this tree is past the commit the fixture records"
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO).decode().strip()
    record = {"commit": commit, "packers": pc.compute(data_utils, encode_fill_at_that_commit)}
    with open(pc.GOLDEN, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: commit %s, %d bytes" % (pc.GOLDEN, commit[:12], os.path.getsize(pc.GOLDEN)))


if __name__ == "__main__":
    main()
