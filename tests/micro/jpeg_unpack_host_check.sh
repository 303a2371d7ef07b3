#!/bin/bash
# Builds tests/micro/jpeg_unpack_host_check.cpp with AddressSanitizer + UBSan on the HOST code and runs it on the fixture,
# the real-size streams and the malformed set of tests/jpeg_unpack_cases.py.  CPU only: no GPU is opened, nothing is loaded
# into Python.  Usage: from the repository root, tests/micro/jpeg_unpack_host_check.sh [work directory]
set -e
cd "$(dirname "$0")/../.."
WORK=${1:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
python - "$WORK/jpeg_unpack_cases.bin" <<'PY'
import sys
import numpy as np
sys.path.insert(0, "tests")
sys.path.insert(0, "tf-ssd_amd")
import jpeg_cases as jc
import jpeg_unpack_cases as uc
fixture = jc.load_fixture()[0]
sound = [blob for blob, _ in fixture.values()] + list(uc.real_streams().values())
with open(sys.argv[1], "wb") as f:
    def dump(blob, info):
        f.write(np.array([len(blob)], np.int32).tobytes())
        f.write(bytes(info))
        f.write(blob)
    for blob in sound:
        rc, info, err = jc.parse(blob)
        assert rc == 0, err
        dump(blob, info)
    for base in (fixture["size_17x33_420"][0], uc.real_streams()["real_size"], fixture["restart1_420"][0]):
        rc, info, _ = jc.parse(base)
        for _, blob in uc.malformed(base):
            dump(blob, info)
PY
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
  -ffp-contract=off -fwrapv tests/micro/jpeg_unpack_host_check.cpp tf-ssd_amd/csrc/ssd_jpeg.hip -o "$WORK/jpeg_unpack_host_check"
"$WORK/jpeg_unpack_host_check" "$WORK/jpeg_unpack_cases.bin"
