"""CPU: the gfx950 ISA of the audio model's tail kernels (csrc/k_audio_tail.hip) as hipcc emits it from the committed source, in the style of
tests/test_audio_isa_cpu.py: the register count of every kernel at the count the build has, no spills and NO scratch at all; the skinny GEMM streams its
weights global -> VGPR with non-temporal 16-byte loads (no LDS-DMA: no two waves share a weight), reads its activation fragments from LDS and runs on the
MFMA its precision names."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (UN k-steps per chunk, row tiles, split) -> VGPRs: two register buffers of UN (x 2 planes) x 4 VGPRs, the accumulators and the LDS fragments in flight
GEMM_VGPRS = {(16, 2, False): 157, (16, 1, False): 145, (2, 2, False): 47, (2, 1, False): 35,
              (8, 2, True): 155, (8, 1, True): 145, (2, 2, True): 62, (2, 1, True): 52}
TRUNK_VGPRS = {"k_tail_linear": 48, "k_tail_attn": 38, "k_tail_add_ln": 20, "k_tail_cat": 6, "k_tail_head": 21}


def _kernels(src):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", "-", src],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    ks = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", out.stdout):
        ks[m.group(1)] = dict(scratch=int(m.group(2)), vgprs=int(m.group(3)), spills=int(m.group(4)))
    assert ks, "no kernel metadata found"
    body = {}
    for name in ks:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", out.stdout, re.M | re.S)
        assert m, name
        body[name] = m.group(1)
    return ks, body


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not installed")
def test_tail_kernels_registers_and_no_scratch():
    ks, body = _kernels("k_audio_tail.hip")
    assert len(ks) == len(GEMM_VGPRS) + len(TRUNK_VGPRS), sorted(ks)
    seen = set()
    for name, k in ks.items():
        assert k["spills"] == 0 and k["scratch"] == 0, (name, k)
        assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body[name]), name
        g = re.search(r"k_tail_gemmILi(\d+)ELi(\d+)ELb([01])E", name)
        if g:
            key = (int(g.group(1)), int(g.group(2)), g.group(3) == "1")
            seen.add(key)
            assert k["vgprs"] == GEMM_VGPRS[key], (key, k)
            un, nrt, x = key
            mfma, other = ("v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x32_bf16") if x else ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x32_f16")
            # both register buffers' chunks are unrolled: UN k-steps x row tiles (x 3 products in the split mode) each
            assert body[name].count(mfma) == 2 * un * nrt * (3 if x else 1) and other not in body[name], (key, body[name].count(mfma))
            nt = len(re.findall(r"global_load_dwordx4 [^\n]* nt\b", body[name]))
            assert nt >= 2 * un * (2 if x else 1), (key, nt)                      # the weight stream: every load of it non-temporal ...
            assert len(re.findall(r"global_load_dwordx4", body[name])) - nt <= 4   # ... what is left: the activation row's two halves (LDS fill) and the bias of either buffer's epilogue
            assert "global_load_lds" not in body[name] and "ds_read_b128" in body[name], key
            assert re.search(r"global_store_dwordx4", body[name]), key
        else:
            short = re.search(r"(k_tail_[a-z_]+?)E", name).group(1)
            assert k["vgprs"] == TRUNK_VGPRS[short], (short, k)
            assert "v_mfma" not in body[name], short                               # the trunk is plain fp32 FMAs
    assert seen == set(GEMM_VGPRS)
