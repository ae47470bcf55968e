"""CPU: the resource counts of BVH export's kernels (csrc/k_bvh.hip) as hipcc emits them for gfx950 from the committed source, in the style of
tests/test_smooth_isa_cpu.py: four kernels, no spills, no scratch (the channel axes are picked by selects, the per-sequence offsets read from the kernel arguments),
no LDS, and register counts that leave every kernel at full occupancy (<= 64 VGPRs: eight waves per SIMD).  Only the metadata is read."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = {"k_bvh_format": 14, "k_bvh_motion": 25, "k_bvh_walk": 61, "k_bvh_decode": 38}      # what hipcc emitted when the kernels were written


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_bvh_kernels_registers_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_bvh.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        short = next((n for n in VGPRS_RECORDED if n in m.group(2)), m.group(2))
        ks[short] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert sorted(ks) == sorted(VGPRS_RECORDED), sorted(ks)
    for name, k in ks.items():
        print(f"{name}: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED[name]}), scratch {k['scratch']}, LDS {k['lds']}")
        assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == 0 and k["vgprs"] <= 64, (name, k)
