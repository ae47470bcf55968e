"""CPU: the gfx950 metadata of the beat-alignment kernels (csrc/k_beat.hip) as hipcc emits them from the committed source, in the style of
tests/test_motion_metrics_isa_cpu.py: the file compiles for gfx950; no kernel spills or uses scratch at all; each kernel's LDS is the size the host header
states (csrc/amuse_beat_host.hpp); no matrix-core instruction and no atomic; the pick and align kernels do their arithmetic in double; and the register counts
(recorded below) keep the occupancy the design claims: the envelope kernel's 256 threads are one wave per SIMD, and at <= 64 VGPRs eight such workgroups fit a
CU (their 4 KiB of LDS allow far more), which is what hides its barriers; the one-wave align kernel and the pick kernel stay below 128."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPRS_RECORDED = {"k_beat_envelope": 64, "k_beat_pick": 24, "k_beat_align": 62}      # what hipcc emitted when the kernels were written; the bounds are below
VGPR_BOUND = {"k_beat_envelope": 64, "k_beat_pick": 128, "k_beat_align": 128}
LDS_NAMES = {"k_beat_envelope": "kBeatEnvLdsBytes", "k_beat_pick": "kBeatPickLdsBytes", "k_beat_align": "kBeatAlignLdsBytes"}
LDS_BYTES = {"k_beat_envelope": (2 * 512 + 8 + 2) * 4, "k_beat_pick": 4 * 4, "k_beat_align": 65 * 64 * 8 + 131072 // 8}


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_beat_kernels_registers_lds_and_no_scratch():
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", "k_beat.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)",
                         out.stdout):
        ks[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgprs=int(m.group(4)), spills=int(m.group(5)))
    assert len(ks) == 3, sorted(ks)
    hpp = (CSRC / "amuse_beat_host.hpp").read_text()
    assert re.search(r"kBeatRun = 16;", hpp) and re.search(r"kBeatMaxOrder = 32;", hpp) and re.search(r"kBeatMaxAudioFrames = 131072;", hpp)
    assert re.search(r"kBeatEnvLdsBytes = \(2 \* kBeatFft \+ 8 \+ 2\) \* 4;", hpp) and re.search(r"kBeatAlignLdsBytes = kBeatRing \* 64 \* 8 \+ kBeatMaxAudioFrames / 8;", hpp)
    seen = set()
    for mangled, k in ks.items():
        name = next(n for n in VGPRS_RECORDED if n in mangled)
        seen.add(name)
        print(f"{name}: {k['vgprs']} VGPRs (recorded {VGPRS_RECORDED[name]}, bound {VGPR_BOUND[name]}), scratch {k['scratch']}, LDS {k['lds']} ({LDS_NAMES[name]})")
        assert k["spills"] == 0 and k["scratch"] == 0 and k["lds"] == LDS_BYTES[name] and k["vgprs"] <= VGPR_BOUND[name], (name, k)
        m = re.search(r"^" + re.escape(mangled) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
        assert m, name
        body = m.group(1)
        assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body), name
        assert "v_mfma" not in body and "global_atomic" not in body and "flat_atomic" not in body and "ds_add" not in body, name
        if name == "k_beat_envelope":
            assert "v_sin_f32" in body or "v_cos_f32" in body or "s_barrier" in body          # the FFT in LDS
            assert "_f64" not in body                                                          # the envelope is fp32
        else:
            assert "v_add_f64" in body or "v_fma_f64" in body                                  # double after the load
        if name == "k_beat_align":
            assert "v_fma_f64" in body and "v_sqrt_f64" in body or "v_rsq_f64" in body         # speeds and exp in double
    assert seen == set(VGPRS_RECORDED)
