"""CPU: the gfx950 ISA of long-form inference's join (csrc/k_stitch.hip) as hipcc emits it from the committed source, in the style of tests/test_body_isa_cpu.py:
one kernel, no spills and NO scratch at all (the per-sequence offsets are read from the kernel arguments by a uniform index, not copied to private memory), no LDS,
no matrix-core instruction, and a register count that keeps eight waves per SIMD possible (<= 64 VGPRs; recorded below)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = 33      # what hipcc emitted when the kernel was written; the assertion below is the bound, this is the record


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_stitch_kernel_registers_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_stitch.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == 1 and "k_stitch" in next(iter(ks)), sorted(ks)
    name, k = next(iter(ks.items()))
    print(f"k_stitch: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED}), scratch {k['scratch']}, LDS {k['lds']}")
    assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == 0 and k["vgprs"] <= 64, k
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
    assert m, name
    body = m.group(1)
    assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body)
    assert "v_mfma" not in body and "ds_" not in body and "global_atomic" not in body
    assert "global_load_dword" in body and "global_store_dword" in body
