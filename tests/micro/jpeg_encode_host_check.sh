#!/bin/bash
# Builds tests/micro/jpeg_encode_host_check.cpp with AddressSanitizer + UBSan on the HOST code and runs it on the cases of
# tests/golden/jpeg_encode.npz.  CPU only: no GPU is opened, nothing is loaded into Python.  Usage: from the repository
# root, tests/micro/jpeg_encode_host_check.sh [work directory]
set -e
cd "$(dirname "$0")/../.."
WORK=${1:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
python - "$WORK/jpeg_encode_cases.bin" <<'PY'
import sys
import numpy as np
sys.path.insert(0, "tests")
import jpeg_encode_cases as jc
fixture = jc.load_fixture()[0]
with open(sys.argv[1], "wb") as f:
    for name, (rgb, q, s, blob) in fixture.items():
        g, coef = jc.forward(rgb, s, jc.quality_tables(q))
        f.write(np.array([g.H, g.W, g.hs, g.vs, q, coef.size, len(blob)], np.int32).tobytes())
        f.write(coef.astype(np.int16).tobytes())
        f.write(blob)
PY
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -ffp-contract=off tests/micro/jpeg_encode_host_check.cpp tf-ssd_amd/csrc/ssd_jpeg_enc.hip tf-ssd_amd/csrc/ssd_jpeg.hip \
  -o "$WORK/jpeg_encode_host_check"
"$WORK/jpeg_encode_host_check" "$WORK/jpeg_encode_cases.bin"
