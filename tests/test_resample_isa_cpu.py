"""CPU: the gfx950 ISA of the resampler (csrc/k_resample.hip) as hipcc emits it from the committed source - the resource check of tests/test_stitch_isa_cpu.py:
one kernel, no spills and NO scratch at all, no LDS (the kernel stages nothing), and a register count within the recorded one plus a small allowance."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = 25      # what hipcc emitted when the kernel was written
VGPRS_ALLOWED = 32       # the recorded count plus a small allowance (sixteen waves per SIMD stay possible up to 32)


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_resample_kernel_registers_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_resample.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == 1 and "k_resample" in next(iter(ks)), sorted(ks)
    name, k = next(iter(ks.items()))
    print(f"k_resample: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED}), scratch {k['scratch']}, LDS {k['lds']}")
    assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == 0 and k["vgprs"] <= VGPRS_ALLOWED, k
