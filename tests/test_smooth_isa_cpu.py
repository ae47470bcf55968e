"""CPU: the gfx950 ISA of motion smoothing's kernel (csrc/k_smooth.hip) as hipcc emits it from the committed source, in the style of tests/test_stitch_isa_cpu.py:
one kernel, no spills and NO scratch at all (the per-sequence offsets and the half-windows are read from the kernel arguments, not copied to private memory),
no matrix-core instruction, no global atomic, LDS exactly the quaternion tile the source states ((32 + 2 x 15) rows x 56 slots x 16 B = 55,552 B), and a register
count that keeps what the kernel's comment claims: the LDS lets two workgroups of four waves share a CU, two waves per SIMD, which 512 / 2 = 256 VGPRs would
still allow - the bound here is 128, half of that, so that a smaller tile could double the occupancy without meeting the registers first (recorded below)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = 77      # what hipcc emitted when the kernel was written; the assertion below is the bound, this is the record
LDS_BYTES = (32 + 2 * 15) * 56 * 16


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_smooth_kernel_registers_lds_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_smooth.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == 1 and "k_smooth" in next(iter(ks)), sorted(ks)
    name, k = next(iter(ks.items()))
    print(f"k_smooth: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED}), scratch {k['scratch']}, LDS {k['lds']}")
    src = (CSRC / "amuse_smooth_host.hpp").read_text()
    assert "kSmoothTile = 32" in src and "AMUSE_SMOOTH_MAX_HALF" in src          # what LDS_BYTES restates
    assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == LDS_BYTES and k["vgprs"] <= 128, k
    assert 2 * k["lds"] <= 160 * 1024 < 3 * k["lds"]                               # two workgroups per CU, as the kernel's comment says
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
    assert m, name
    body = m.group(1)
    assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body)
    assert "v_mfma" not in body and "global_atomic" not in body
