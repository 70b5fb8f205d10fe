"""tests/cpp/ff_overflow.cpp: operator*, sqr, diff_of_products and sum_of_products<6> of ff.hip.h on the host over the limb-pattern operands of
tests/helpers/limb_cases.py, in a stand-alone program built with -fsanitize=signed-integer-overflow,shift -fno-sanitize-recover (an overflowing
signed column accumulator ends it).  CPU only; where the toolchain cannot link the sanitizer's runtime the program is built without it, with a
warning, and still compares the routines with each other."""
import os
import subprocess
import warnings

import numpy as np

from tests import util
from tests.helpers import limb_cases as lc

SRC = os.path.join(util.ROOT, "tests", "cpp", "ff_overflow.cpp")
CSRC = os.path.join(util.ROOT, "snarkvm_amd", "csrc")
SAN = ["-fsanitize=signed-integer-overflow,shift", "-fno-sanitize-recover=all"]


def _build(tmp_path):
    """-> (exe, sanitized).  The unsanitized build is tried only when the sanitized one fails at the LINK of the sanitizer's runtime (a toolchain
    without libclang_rt.ubsan for the host); any other failure is a failure."""
    exe = str(tmp_path / "ff_overflow")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = [hipcc, "-x", "hip", "--offload-host-only", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, SRC, "-o", exe]
    r = subprocess.run(base + [x for flag in SAN for x in ("-Xarch_host", flag)], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True
    assert "ubsan" in r.stderr and ("cannot find" in r.stderr or "no such file" in r.stderr.lower() or "undefined" in r.stderr), r.stderr
    warnings.warn("the sanitizer runtime does not link here: tests/cpp/ff_overflow.cpp built WITHOUT " + " ".join(SAN) + "; values are still checked")
    subprocess.run(base, check=True, capture_output=True)
    return exe, False


def test_column_accumulators_do_not_overflow_on_limb_patterns(tmp_path):
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for field in (0, 1):
            arr = lc.cases(field).arr
            f.write(np.uint32(arr.shape[0]).tobytes())
            f.write(np.ascontiguousarray(arr, dtype="<u8").tobytes())
    exe, sanitized = _build(tmp_path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    print(("built with " if sanitized else "built WITHOUT ") + " ".join(SAN))
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
