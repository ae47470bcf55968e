"""CPU: the gfx950 ISA of the audio parity mode's kernels (csrc/k_audio_gemm_x.hip, csrc/k_audio_x.hip) as hipcc emits it from the committed sources, in the style of
tests/test_isa_cpu.py: register budget, no spills and NO scratch at all - the GEMM's k loop and the attention's key loop run on registers and LDS only."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _kernels(src, extra=()):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", *extra, "-S", "--cuda-device-only", "-o", "-", src],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", out.stdout):
        ks[m.group(1)] = dict(scratch=int(m.group(2)), vgprs=int(m.group(3)), spills=int(m.group(4)))
    assert ks, "no kernel metadata found"
    # scratch instructions per kernel body
    body = {}
    for name in ks:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
        assert m, name
        body[name] = m.group(1)
    return ks, body


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
@pytest.mark.parametrize("src,extra,hot,n_hot", [
    ("k_audio_gemm_x.hip", (), "k_gemm_x", 4),                                                        # the four epilogues of the split-fp16 GEMM
    ("k_audio_x.hip", ("-mllvm", "-amdgpu-mfma-vgpr-form=1", "-fno-honor-nans"), "k_ast_attn_x", 1),   # the flags of the Makefile
])
def test_parity_mode_kernels_have_no_scratch(src, extra, hot, n_hot):
    ks, body = _kernels(src, extra)
    assert sum(hot in n for n in ks) == n_hot, sorted(ks)
    for name, k in ks.items():
        assert k["vgprs"] <= 256 and k["spills"] == 0 and k["scratch"] == 0, (name, k)
        assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body[name]), name
        if hot in name:
            assert body[name].count("v_mfma_f32_16x16x32_f16") >= 48 and "v_mfma_f32_16x16x32_bf16" not in body[name], name
            assert "global_load_lds_dwordx4" in body[name], name
