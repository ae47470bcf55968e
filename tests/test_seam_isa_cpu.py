"""CPU: the gfx950 resource metadata of the long-form candidates' kernels (csrc/k_seam.hip) as hipcc emits it from the committed source, in the style of
tests/test_stitch_isa_cpu.py: the four kernels exist, none spills and none has scratch (the per-sequence offsets are read from the kernel arguments by a uniform
index, not copied to private memory), LDS is what the design says - none, except the path kernel's 960 windows x 64 candidates of one-byte back-pointers - and the
register counts keep eight waves per SIMD possible (<= 64 VGPRs; recorded below)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# what hipcc emitted when the kernels were written; the assertions below are the bound, these are the record
VGPRS_RECORDED = {"k_seam_quats": 25, "k_seam_cost": 40, "k_seam_path": 20, "k_seam_select": 11}
LDS = {"k_seam_quats": 0, "k_seam_cost": 0, "k_seam_path": 960 * 64, "k_seam_select": 0}


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_seam_kernels_registers_lds_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_seam.hip"],
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
        assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == LDS[name] and k["vgprs"] <= 64, (name, k)
    assert "v_mfma" not in out.stdout and "global_atomic" not in out.stdout and "ds_add" not in out.stdout      # no matrix core, no atomics anywhere
