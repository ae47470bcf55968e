"""CPU: tests/seam_host/ - the long-form candidates' host code (csrc/amuse_seam_host.hpp through the entry points of csrc/amuse_seam.hip: the plan, the argument
checks of cost / path / select, the packing of sequences into launches across the per-launch capacity) in a stand-alone program (its own main, stand-in
launchers) under AddressSanitizer / UBSan, on the stubbed HIP runtime of tests/host_asan (compiled unchanged).  Nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def test_seam_host_program_under_asan_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("hipcc not available")
    build = subprocess.run(["bash", str(REPO / "tests" / "build_host_program.sh"), "seam", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
    run = subprocess.run([str(tmp_path / "seam_host")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stdout.strip().endswith("seam_host ok"), run.stdout[-2000:] + run.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
