"""CPU: the gfx950 ISA of the preview renderer's two kernels (csrc/k_render.hip) as hipcc emits them from the committed source, in the style of
tests/test_stitch_isa_cpu.py: no spills and NO scratch at all, LDS = the 32 x 32 tile of 64-bit keys the plan's tile size gives (the projection kernel uses none),
no global atomic (the depth test is an LDS minimum: there is no global depth buffer), no matrix-core instruction, and register counts that keep several waves
per SIMD (recorded below)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = {"k_render_project": 32, "k_render_tile": 76}      # what hipcc emitted when the kernels were written; the assertions below are the bounds
TILE = 32                                                            # samples per tile side: amuse_render_plan's tiles_x = ceil(width ss / 32)


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_render_kernels_registers_lds_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_render.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == 2, sorted(ks)
    by = {short: next((n, k) for n, k in ks.items() if short in n) for short in VGPRS_RECORDED}
    from amuse_amd import render
    assert render.plan(TILE, TILE, 1, 10, 10, 1)["tiles_x"] == 1 and render.plan(TILE + 1, TILE, 1, 10, 10, 1)["tiles_x"] == 2      # the plan's tile IS 32 samples
    want_lds = {"k_render_project": 0, "k_render_tile": TILE * TILE * 8}
    for short, (name, k) in by.items():
        print(f"{short}: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED[short]}), scratch {k['scratch']}, LDS {k['lds']}")
        assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == want_lds[short] and k["vgprs"] <= 128, (short, k)
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
        assert m, name
        body = m.group(1)
        assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body)
        assert "v_mfma" not in body and "global_atomic" not in body and "flat_atomic" not in body
        if short == "k_render_tile":
            assert re.search(r"\bds_min_u64\b", body) and "ds_min_rtn_u64" not in body      # the depth test: one LDS minimum per covered sample, no return value
        else:
            assert "ds_" not in body and "v_fma_f64" in body                                # the depth is quantised in double
