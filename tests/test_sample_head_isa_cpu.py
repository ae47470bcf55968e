"""CPU: the gfx950 listings of the 8-wave sampling kernels (k_sampler8.hip, its fp16 build k_sampler8h.hip, k_sampler8x.hip), built through the Makefile's
own rule, i.e. with each unit's own flags (cross-compiles without a GPU).  Token assembly reads LDS only: no instantiation may hold a
flat_load (a per-lane choice between an LDS and a global pointer compiles to one, and the address then goes through the aperture check to reach LDS;
the build before the assembly left the step head had 18 in the product instantiation alone).  And no instantiation - eval, train-mode, phase-stamped - may spill
or use scratch, or take more registers than it did before that change (VGPRS: .vgpr_count of that build's listing)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNITS = ("k_sampler8", "k_sampler8h", "k_sampler8x")
# template arguments as they are mangled: <PROF, DROP> of k_sample8 / k_sample8h, <PROF> of k_sample8x
VGPRS = {
    "k_sample8ILb0ELb0E": 255, "k_sample8ILb1ELb0E": 254, "k_sample8ILb0ELb1E": 254, "k_sample8ILb1ELb1E": 256,
    "k_sample8hILb0ELb0E": 255, "k_sample8hILb1ELb0E": 254, "k_sample8hILb0ELb1E": 254, "k_sample8hILb1ELb1E": 256,
    "k_sample8xILb0E": 256, "k_sample8xILb1E": 256,
}


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa")
    made = subprocess.run(["make", "-s", "-C", str(CSRC), "isa", f"HIPCC={HIPCC}", f"OUT={out}", "ISA=" + " ".join(f"{out}/{u}.s" for u in UNITS), "-j3"],
                          capture_output=True, text=True, timeout=900)
    assert made.returncode == 0, made.stderr[-2000:]
    return {u: (out / f"{u}.s").read_text() for u in UNITS}


def _bodies(asm):
    """symbol -> the instructions of every k_sample8* kernel of a listing (label line .. s_endpgm)"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w*k_sample8\w*):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            ins = line.split(";")[0].strip()
            if ins:
                cur.append(ins)
            if ins == "s_endpgm":
                cur = None
    return out


def _metadata(asm):
    """symbol -> {key: int} from the listing's amdhsa.kernels metadata"""
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|amdhsa\.target|\.\.\.|$)", asm[asm.index("amdhsa.kernels"):], re.S):
        text = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", text).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", text)}
    return out


def test_every_instantiation_is_listed(listings):
    names = [n for u in UNITS for n in _metadata(listings[u])]
    assert sorted(k for k in VGPRS if any(k in n for n in names)) == sorted(VGPRS) and len(names) == len(VGPRS), names
    assert sorted(n for u in UNITS for n in _bodies(listings[u])) == sorted(names)


@pytest.mark.parametrize("unit", UNITS)
def test_no_flat_load(listings, unit):
    for name, ins in _bodies(listings[unit]).items():
        flat = [i for i in ins if i.startswith("flat_load")]
        assert not flat, (name, len(flat), flat[:3])


@pytest.mark.parametrize("unit", UNITS)
def test_no_spill_no_scratch_registers_at_most_the_parents(listings, unit):
    for name, md in _metadata(listings[unit]).items():
        key = next(k for k in VGPRS if k in name)
        assert md["vgpr_spill_count"] == 0, (name, md)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["vgpr_count"] <= VGPRS[key], (name, md, VGPRS[key])
