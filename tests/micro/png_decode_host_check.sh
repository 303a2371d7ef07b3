#!/bin/bash
# Builds tests/micro/png_decode_host_check.cpp with AddressSanitizer + UBSan on the HOST code and runs ssd_png_parse,
# ssd_png_idat and ssd_png_decode_host over the cases of tests/png_decode_cases.py (those that need no library to make) and
# over every truncation and single-byte corruption of the first three.  CPU only: no GPU is opened, nothing is loaded into
# Python.  Usage: from the repository root, tests/micro/png_decode_host_check.sh [work directory]
set -e
cd "$(dirname "$0")/../.."
WORK=${1:-$(mktemp -d)}
mkdir -p "$WORK"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
python - "$WORK/png_decode_cases.bin" <<'PY'
import struct
import sys
import zlib
import numpy as np
sys.path.insert(0, "tests")
import png_decode_cases as dc

def stream_of(blob):
    pos, data = 8, b""
    while pos < len(blob):
        n = struct.unpack(">I", blob[pos:pos + 4])[0]
        if blob[pos + 4:pos + 8] == b"IDAT":
            data += blob[pos + 8:pos + 8 + n]
        pos += 12 + n
    return zlib.decompress(data)

with open(sys.argv[1], "wb") as f:
    for case in dc.written_cases() + dc.pillow_cases():
        kind, px = dc.pillow_outcome(case["blob"])
        assert kind == "pixels"
        F = stream_of(case["blob"])
        f.write(np.array([len(case["blob"]), len(F), px.shape[0], px.shape[1], 0], np.int32).tobytes())
        f.write(case["blob"] + F + np.ascontiguousarray(px).tobytes())
    for name, blob, code in dc.refusal_cases():
        f.write(np.array([len(blob), -1, 0, 0, code], np.int32).tobytes())
        f.write(blob)
PY
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -ffp-contract=off tests/micro/png_decode_host_check.cpp tf-ssd_amd/csrc/ssd_png_dec.hip -o "$WORK/png_decode_host_check"
"$WORK/png_decode_host_check" "$WORK/png_decode_cases.bin"
