"""CPU: the gfx950 ISA of the body-model kernels (csrc/k_body.hip) as hipcc emits it from the committed source, in the style of tests/test_audio_tail_isa_cpu.py:
every kernel within 256 VGPRs (two 8-wave workgroups' worth of waves per SIMD stay possible), no spills and NO scratch at all; the skinning kernel runs on
v_mfma_f32_16x16x32_f16 - three per product in the split instantiations, one in the one-product ones - and reads its pose features from LDS."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SKIN = {(1, True, False), (1, False, False), (2, True, True), (2, False, True), (3, True, True), (3, False, True)}   # (sets, split, loss)


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
def test_body_kernels_registers_and_no_scratch():
    ks, body = _kernels("k_body.hip")
    assert len(ks) == len(SKIN) + 2, sorted(ks)
    seen = set()
    for name, k in ks.items():
        assert k["spills"] == 0 and k["scratch"] == 0 and k["vgprs"] <= 256, (name, k)
        assert not re.search(r"\b(scratch_|buffer_(load|store)_dword\S*\s+\S+,\s*off,\s*s\[\d+:\d+\],\s*0\s+offset)", body[name]), name
        g = re.search(r"k_body_skinILi(\d)ELb([01])ELb([01])E", name)
        if g:
            key = (int(g.group(1)), g.group(2) == "1", g.group(3) == "1")
            seen.add(key)
            nset, split, loss = key
            # 16 k-steps x sets x (3 | 1) products, fully unrolled; nothing else on the matrix cores
            assert body[name].count("v_mfma_f32_16x16x32_f16") == 16 * nset * (3 if split else 1), (key, body[name].count("v_mfma_f32_16x16x32_f16"))
            assert len(re.findall(r"v_mfma_", body[name])) == body[name].count("v_mfma_f32_16x16x32_f16")
            assert "ds_read_b128" in body[name] and "global_load_dwordx4" in body[name], key
            if not loss:
                assert "global_store_dword" in body[name], key                               # forward stores vertices ...
            else:
                assert "global_atomic" not in body[name] and "ds_add" not in body[name], key   # ... the loss: plain stores of per-workgroup partials, no float atomics
        else:
            assert "v_mfma" not in body[name], name
    assert seen == SKIN
