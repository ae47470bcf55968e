"""Register / spill / LDS / scratch figures of every kernel in amuse_amd/csrc, from the gfx950 ISA hipcc emits for the committed sources
(cross-compiles without a GPU; `make isa` of csrc/Makefile, so every unit gets its object's own flags).  Usage: python tools/isa_report.py > profiles/rNN_isa_resources.txt"""
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "amuse_amd" / "csrc"
isa_dir = Path(tempfile.mkdtemp(prefix="amuse_isa_"))
made = subprocess.run(["make", "-s", "-C", str(CSRC), "-j8", "isa", f"OUT={isa_dir}"], capture_output=True, text=True)
if made.returncode:
    sys.exit(made.stderr[-2000:])
print(f"{'kernel':70s} {'VGPR':>5s} {'spill':>6s} {'SGPR':>5s} {'LDS static':>11s} {'scratch B/lane':>15s} {'v_mfma':>7s}")
for asm in sorted(isa_dir.glob("k_*.s")):
    text = asm.read_text()
    mfma = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
        elif cur and "v_mfma" in line:
            mfma[cur] = mfma.get(cur, 0) + 1
    print(f"# {asm.stem}.hip")
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text):
        lds, name, scratch, sgpr, vgpr, spill = m.groups()
        nice = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        nice = re.sub(r"amuse::\(anonymous namespace\)::", "", nice)
        nice = re.sub(r"\(.*\)$", "", nice).replace("void ", "")
        print(f"{nice[:70]:70s} {vgpr:>5s} {spill:>6s} {sgpr:>5s} {lds:>11s} {scratch:>15s} {mfma.get(name, 0):>7d}")
shutil.rmtree(isa_dir, ignore_errors=True)
