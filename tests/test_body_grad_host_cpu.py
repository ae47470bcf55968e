"""CPU: the host half of the body model's gradient calls.  tests/body_grad_host/ is a stand-alone program (its own main) that runs the transposed-image packer of
csrc/amuse_body_pack.hpp and csrc/amuse_body_grad.hip on the stubbed HIP runtime of tests/host_asan under AddressSanitizer / UBSan (nothing loaded into Python
runs under a sanitizer); the image's layout is restated here in numpy, and its digest for an exact integer-valued matrix is pinned in
tests/golden/body_grad_pack.json - by the restatement and by the program's own output."""
import json
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((REPO / "tests" / "golden" / "body_grad_pack.json").read_text())


def _image(V):
    """the transposed image of posedirs[k][v * 3 + c] = (31 k + 7 v + 3 c) % 61 - 30, pre-scaled by 2^9 (its largest entry, 30, then sits in 2^13..2^14): fp16 bits,
    [pairs][32 feature tiles][64 lanes][8]: lane = (v & 3) * 16 + (k & 15), element = 4 (group & 1) + c, pair = v >> 3; everything else zero.  lo plane: zero."""
    pairs = ((V + 3) // 4 + 1) // 2
    k, v, c = np.meshgrid(np.arange(486), np.arange(V), np.arange(3), indexing="ij")
    val = ((31 * k + 7 * v + 3 * c) % 61 - 30).astype(np.float32) * np.float32(512.0)
    hi = np.zeros((pairs, 32, 64, 8), np.float16)
    hi[v >> 3, k >> 4, (v & 3) * 16 + (k & 15), ((v >> 2) & 1) * 4 + c] = val.astype(np.float16)
    assert np.array_equal(hi.astype(np.float32)[v >> 3, k >> 4, (v & 3) * 16 + (k & 15), ((v >> 2) & 1) * 4 + c], val)   # exact in fp16
    return hi.view(np.uint16).reshape(-1), np.zeros(hi.size, np.uint16)


def _fnv(planes):
    h = 1469598103934665603
    for p in planes:
        for b in p.astype("<u2").tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


@pytest.mark.parametrize("V", [37, 203])
def test_transposed_image_digest(V):
    assert _fnv(_image(V)) == GOLDEN["digest"][str(V)]
    assert GOLDEN["bytes_at_V_10475"] == (((10475 + 3) // 4 + 1) // 2) * 65536 == 85852160


def test_body_grad_host_program_under_asan_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("hipcc not available")
    build = subprocess.run(["bash", str(REPO / "tests" / "build_host_program.sh"), "body_grad", str(tmp_path), "amuse_body"], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
    run = subprocess.run([str(tmp_path / "body_grad_host")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stdout.strip().endswith("body_grad_host ok"), run.stdout[-2000:] + run.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    got = dict(re.findall(r"digest V (\d+) ([0-9a-f]{16})", run.stdout))
    assert got == GOLDEN["digest"], (got, GOLDEN["digest"])
