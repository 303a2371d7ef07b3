#!/bin/bash
# Builds tests/micro/png_host_check.cpp with AddressSanitizer + UBSan on the HOST code and runs ssd_png_encode_host over the
# cases of tests/png_cases.py.  CPU only: no GPU is opened, nothing is loaded into Python.  Usage: from the repository
# root, tests/micro/png_host_check.sh [work directory]
set -e
cd "$(dirname "$0")/../.."
WORK=${1:-$(mktemp -d)}
mkdir -p "$WORK"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
python - "$WORK/png_cases.bin" <<'PY'
import sys
import numpy as np
sys.path.insert(0, "tests")
import png_cases as pc
with open(sys.argv[1], "wb") as f:
    for name, rgb, mode in pc.cases():
        F = pc.filtered_stream(rgb, mode)
        f.write(np.array([rgb.shape[0], rgb.shape[1], mode, len(F)], np.int32).tobytes())
        f.write(np.ascontiguousarray(rgb).tobytes())
        f.write(F)
PY
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -ffp-contract=off tests/micro/png_host_check.cpp tf-ssd_amd/csrc/ssd_png.hip -o "$WORK/png_host_check"
"$WORK/png_host_check" "$WORK/png_cases.bin"
