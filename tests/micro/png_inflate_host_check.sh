#!/bin/bash
# Builds tests/micro/png_inflate_host_check.cpp with AddressSanitizer + UBSan on the HOST code and runs
# ssd_png_inflate_host over the cases of tests/png_inflate_cases.py (those that need no library to make) and over every
# truncation and single-byte corruption of the first three.  CPU only: no GPU is opened, nothing is loaded into Python.
# Usage: from the repository root, tests/micro/png_inflate_host_check.sh [work directory]
set -e
cd "$(dirname "$0")/../.."
WORK=${1:-$(mktemp -d)}
mkdir -p "$WORK"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
python - "$WORK/png_inflate_cases.bin" <<'PY'
import sys
import zlib
import numpy as np
sys.path.insert(0, "tests")
import png_inflate_cases as ic

BITS = ["header", "block_type", "stored", "symbols", "repeat", "oversubscribed", "incomplete", "no_end", "symbol", "distance", "input", "output",
        "adler", "trailing", "filter"]                                              # include/ssd_hip.h, SSD_PNG_INFLATE_*: bit k
with open(sys.argv[1], "wb") as f:
    for name, stream, H, rb in ic.accepted_cases():
        f.write(np.array([len(stream), H, rb, 0, 0], np.int32).tobytes())
        f.write(stream + zlib.decompress(stream))
    for name, stream, H, rb, bit in ic.refusal_cases():
        f.write(np.array([len(stream), H, rb, 1 << BITS.index(bit), 0], np.int32).tobytes())
        f.write(stream)
PY
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -ffp-contract=off tests/micro/png_inflate_host_check.cpp tf-ssd_amd/csrc/ssd_png_inflate.hip -o "$WORK/png_inflate_host_check"
"$WORK/png_inflate_host_check" "$WORK/png_inflate_cases.bin"
