"""CPU: the gfx950 metadata of the motion-metric kernel (csrc/k_motion_metrics.hip) as hipcc emits it from the committed source, in the style of
tests/test_render_isa_cpu.py: it compiles for gfx950, has no spills and NO scratch at all, the LDS the design intends - the partials of eight waves, 19 doubles
per lane -, no matrix-core instruction, no atomic, and a register count (recorded below) that lets the workgroup's eight waves sit two to a SIMD."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = {"k_motion_metrics": 112}      # what hipcc emitted when the kernel was written; the assertion below is the bound
WAVES, PARTIALS = 8, 19                         # csrc/amuse_motion_metrics_host.hpp kMetricsWaves, kMetricsPartials


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_motion_metrics_kernel_registers_lds_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_motion_metrics.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == 1, sorted(ks)
    hpp = (CSRC / "amuse_motion_metrics_host.hpp").read_text()
    assert re.search(rf"kMetricsWaves = {WAVES};", hpp) and re.search(rf"kMetricsPartials = {PARTIALS};", hpp)
    (name, k), = ks.items()
    assert "k_motion_metrics" in name
    print(f"k_motion_metrics: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED['k_motion_metrics']}), scratch {k['scratch']}, LDS {k['lds']}")
    # 512 threads = two waves per SIMD: 256 registers each is the file's limit; 128 keeps four, so two workgroups can share a CU (their LDS allows it too)
    assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == WAVES * PARTIALS * 64 * 8 == 77824 and k["vgprs"] <= 128, k
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
    assert m, name
    body = m.group(1)
    assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body)
    assert "v_mfma" not in body and "global_atomic" not in body and "flat_atomic" not in body
    assert "v_fma_f64" in body                                                          # the sums of squares are double
