"""CPU: every runtime call and every kernel launch of the library's launch sequences, with all arguments and in order, against tests/golden/launch_args.json.
tests/host_asan/launch_args.cpp drives the host code through the C ABI on the stubbed HIP runtime, whose launch log (tests/host_asan/hip_stub.cpp,
amuse_stub_log(2)) prints one line per hipMalloc / hipFree / copy / memset / event call and per launcher: its stream and every field of its argument struct,
pointers as `dev#<n>+<offset>/<size>` (the n-th allocation of the process), `<driver buffer>+<offset>`, `0` or `host`.  tests/golden/pack_images.json pins the
uploaded bytes and stage tables; this pins what that leaves open: workspace carving, chunk offsets, attention arguments, the hoisted constants' launches, events
and the order of it all.  The golden holds, per section in order, the line count and the SHA-256 of the section's text.

The golden file was recorded ONCE, with this driver and stub, from the library sources of the commit BEFORE the launch sequences were gathered into one staged
sequence (the three hand-written copies in amuse_api.hip vae_decode / amuse_vae_encode and amuse_variants.hip pose_step):
`tests/host_asan/build.sh DIR && DIR/launch_args > LOG && python tests/test_launch_args_cpu.py --record LOG`.  It is never regenerated from refactored host code:
a change that moves a launch, a pointer or an allocation is a change of behaviour and says so.  To repeat the check, or to see WHAT differs when a section's
digest does: check out that commit's amuse_amd/csrc, build, `python tests/test_launch_args_cpu.py --dump OLD.txt`, the same on the new sources, and diff."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "launch_args.json"


def sections_of(text):
    """[(name, text of the section)] of a driver log, in order."""
    secs = []
    for line in text.splitlines():
        if line.startswith("== "):
            secs.append((line[3:], []))
        elif secs and line != "LAUNCH ARGS OK":
            secs[-1][1].append(line)
    return [(name, "".join(l + "\n" for l in lines)) for name, lines in secs]


def to_golden(text):
    return {"sections": [[name, body.count("\n"), hashlib.sha256(body.encode()).hexdigest()] for name, body in sections_of(text)]}


def run_driver(build_dir):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(Path(build_dir) / "launch_args")], capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0 and "LAUNCH ARGS OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    return run.stdout


def test_launch_arguments_allocations_and_order_match_the_golden(host_asan_build):
    text = run_driver(host_asan_build)
    got = to_golden(text)["sections"]
    want = json.loads(GOLDEN.read_text())["sections"]
    for g, w in zip(got, want):
        assert g[0] == w[0], f"section '{g[0]}' where the golden has '{w[0]}'"
        assert g[1:] == w[1:], f"first section that differs: '{g[0]}' ({g[1]} lines, golden {w[1]}); see the module docstring for how to diff the text"
    assert len(got) == len(want) and len({g[0] for g in got}) == len(got)
    assert sum(g[1] for g in got) > 10000
    # every context is torn down completely: the driver prints the stub's live-allocation count behind each amuse_destroy
    destroys = [body for name, body in sections_of(text) if name.endswith(" destroy")]
    assert len(destroys) == 4 and all(body.endswith("live allocations after destroy: 0\n") for body in destroys)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":      # record: see the module docstring
        GOLDEN.write_text(json.dumps(to_golden(Path(sys.argv[2]).read_text()), indent=0, separators=(",", ":")) + "\n")
    elif len(sys.argv) == 3 and sys.argv[1] == "--dump":      # the full text of this tree's log
        with tempfile.TemporaryDirectory() as d:
            subprocess.run(["bash", str(HERE / "host_asan" / "build.sh"), d], check=True)
            Path(sys.argv[2]).write_text(run_driver(d))
    else:
        sys.exit("usage: test_launch_args_cpu.py --record LOG | --dump FILE")
