"""The shared device helpers of amuse_amd/csrc have ONE definition each.  The sampler and decoder kernels grew by copying a kernel and changing its
arithmetic; the copies of these helpers were folded into amuse_dev.hpp (LDS-DMA, split-fp16 products, scheduler update), amuse_stage.hpp (the LDS-DMA
weight-stage ring) and amuse_sample8.hpp (the 8-wave samplers' scaffold).  A text check of the project's own function names: a second definition in
any .hip / .hpp of the directory fails it."""
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
SOURCES = sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.hpp")))
HELPERS = ["glds16", "lds_addr", "mfma3", "mfma3t", "sched_update", "part_row", "lane_info", "a8_slot", "u_slot", "stamp8", "store_tap_tile",
           "stage_fetch", "stage_end", "wfrag"]


def _defining_files(name):
    # a definition or declaration: `__device__ <qualifiers and return type> name(` (a call has no __device__ in front of it on its line)
    pat = re.compile(r"__device__\b[^;{}()\n]*\b" + re.escape(name) + r"\s*\(")
    return [(p.name, len(pat.findall(p.read_text()))) for p in SOURCES if pat.search(p.read_text())]


@pytest.mark.parametrize("name", HELPERS)
def test_one_definition(name):
    assert SOURCES, CSRC
    found = _defining_files(name)
    assert len(found) == 1 and found[0][1] == 1, f"{name} is defined in {found}"


def test_scheduler_division_written_once():
    hits = [(p.name, p.read_text().count("__fdiv_rn(num, sa)")) for p in SOURCES if "__fdiv_rn(num, sa)" in p.read_text()]
    assert hits == [("amuse_dev.hpp", 1)], hits
