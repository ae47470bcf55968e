"""CPU: the gfx950 ISA of the body model's backward kernels (csrc/k_body_bwd.hip) as hipcc emits it from the committed source, in the style of
tests/test_body_isa_cpu.py: every kernel within 256 VGPRs, no spills and no scratch; the skinning-backward kernel runs the count of v_mfma_f32_16x16x32_f16 its
head comment derives - 16 k-steps x 2 groups x 2 sets forward + 32 feature tiles transposed, x 3 split or x 1 one-product - and accumulates its skinning
gradients with 64-bit integer LDS adds, no float atomics; the per-frame kernel has no matrix-core instruction."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


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
def test_body_bwd_kernels_registers_mfma_counts_and_no_scratch():
    ks, body = _kernels("k_body_bwd.hip")
    assert len(ks) == 3, sorted(ks)
    seen = set()
    for name, k in ks.items():
        assert k["spills"] == 0 and k["scratch"] == 0 and k["vgprs"] <= 256, (name, k)
        assert "scratch_" not in body[name], name
        assert not re.search(r"(global|flat|ds)_(atomic_)?(add|pk_add)_(rtn_)?f(16|32|64)", body[name]), name   # no float atomics anywhere
        g = re.search(r"k_body_skin_bwdILb([01])E", name)
        if g:
            split = g.group(1) == "1"
            seen.add(split)
            n = body[name].count("v_mfma_f32_16x16x32_f16")
            assert n == (16 * 2 * 2 + 32) * (3 if split else 1), (split, n)
            assert len(re.findall(r"v_mfma_", body[name])) == n
            assert "ds_add_u64" in body[name] and "global_atomic" not in body[name], name   # fixed-point sums in LDS
            assert "ds_read_b128" in body[name] and "global_load_dwordx4" in body[name], name
        else:
            assert "k_body_pose_bwd" in name and "v_mfma" not in body[name] and "atomic" not in body[name] and "ds_add" not in body[name], name
    assert seen == {True, False}
