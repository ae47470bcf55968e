"""CPU: every runtime call and every kernel launch of the audio front-end's host code, in BOTH precisions, with all arguments and in order, against
tests/golden/audio_launch_args.json.  tests/host_asan/audio_launch_args.cpp drives amuse_audio_api.hip, amuse_audio_x.hip and amuse_audio_tail.hip through the C ABI
on the stubbed HIP runtime (tests/host_asan/hip_stub.cpp + audio_x_stub.cpp for the parity mode's launchers + tests/host_tail/tail_stub.cpp), whose launch log
(amuse_stub_log(2)) prints one line per hipMalloc / hipFree / copy / memset / event call and per launcher, weight pointers also by the digest of the image uploaded
there.  That pins the parameter walk and both packers (upload order, sizes, digests), the workspaces (allocation order and sizes, growth, free order), every launch
argument of the encoder sequence, streams and events, and teardown.  The golden holds, per section in order, the line count and the SHA-256 of the section's text.
The driver is a stand-alone program under -fsanitize=address,undefined: any sanitizer report or leak fails the test.

ONE canonicalisation: each run of consecutive `hipMemset` lines is sorted before hashing, at record time and at check time.  The recorded sources zero the seven
activation buffers of a workspace in a different order in the two modes (bf16: X, H, O, F, P, Vt, QK; fp32x: X, H, QK, Vt, O, F, P); the calls are synchronous and
independent, and one shared ensure_ws has one order.  Everything else is compared in order and byte for byte.

The golden file was recorded ONCE, with this driver and these stubs, from the library sources of the commit BEFORE the two precisions' host code was gathered into
one encoder description (csrc/amuse_audio_enc.hpp): in a checkout of that commit with tests/host_asan/{hip_stub.cpp,stub_log.hpp,audio_x_stub.cpp,
audio_launch_args.cpp} and this file copied in, `python tests/test_audio_launch_args_cpu.py --dump LOG && python tests/test_audio_launch_args_cpu.py --record LOG`.
It is never regenerated from refactored host code: a change that moves a launch, a pointer, an upload or an allocation is a change of behaviour and says so.  To
see WHAT differs when a section's digest does: `--dump` on both trees and diff the texts (sort the hipMemset runs first).

Peak resident memory of the driver (ASan build): 4.6 GB for the encoder invocation, 4.0 GB for the `tail` invocation."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
GOLDEN = HERE / "golden" / "audio_launch_args.json"
SAN = "-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1".split()
BANNER = "AUDIO LAUNCH ARGS OK"


def canonical(lines):
    """The lines with every run of consecutive hipMemset lines sorted (module docstring)."""
    out, run = [], []
    for line in lines + [""]:
        if line.startswith("hipMemset "):
            run.append(line)
            continue
        out += sorted(run) + [line]
        run = []
    return out[:-1]


def sections_of(text):
    """[(name, canonical text of the section)] of a driver log, in order."""
    secs = []
    for line in text.splitlines():
        if line.startswith("== "):
            secs.append((line[3:], []))
        elif secs and line != BANNER:
            secs[-1][1].append(line)
    return [(name, "".join(l + "\n" for l in canonical(lines))) for name, lines in secs]


def to_golden(text):
    return {"sections": [[name, body.count("\n"), hashlib.sha256(body.encode()).hexdigest()] for name, body in sections_of(text)]}


def build_driver(out):
    """audio_launch_args in `out`, which holds the objects of tests/host_asan/build.sh: beside them the parity mode's and the tail's host code (host-only, as
    build.sh compiles the rest), the stubs of their launchers and the driver."""
    out = Path(out)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    host = [hipcc, "--offload-host-only", "-std=c++17", *SAN]
    for unit in ("amuse_audio_x", "amuse_audio_tail"):
        subprocess.run([*host, "-Wno-unused-function", "-c", str(REPO / "amuse_amd" / "csrc" / f"{unit}.hip"), "-o", str(out / f"{unit}.o")], check=True, capture_output=True, timeout=600)
    for stub in (HERE / "host_asan" / "audio_x_stub.cpp", HERE / "host_tail" / "tail_stub.cpp"):
        subprocess.run([*host, "-x", "hip", "-c", str(stub), "-o", str(out / f"{stub.stem}.o")], check=True, capture_output=True, timeout=600)
    subprocess.run([cxx, "-std=c++17", *SAN, "-c", str(HERE / "host_asan" / "audio_launch_args.cpp"), "-o", str(out / "audio_launch_args.o")], check=True, capture_output=True, timeout=600)
    objs = [str(out / f"{o}.o") for o in ("audio_launch_args", "hip_stub", "audio_x_stub", "tail_stub", "amuse_api", "amuse_variants", "amuse_audio_api", "amuse_audio_x", "amuse_audio_tail")]
    link = subprocess.run([cxx, *SAN, *objs, "-o", str(out / "audio_launch_args")], capture_output=True, text=True, timeout=600)
    assert link.returncode == 0, link.stderr[-3000:]
    return out / "audio_launch_args"


def run_driver(prog):
    """The log of both invocations: the encoders' calls, then the labels behind the tail."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    text = ""
    for args in ([], ["tail"]):
        run = subprocess.run([str(prog), *args], capture_output=True, text=True, timeout=900, env=env)
        assert run.returncode == 0 and BANNER in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
        assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
        text += run.stdout
    return text


def test_audio_launch_arguments_uploads_allocations_and_order_match_the_golden(host_asan_build):
    text = run_driver(build_driver(host_asan_build))
    got = to_golden(text)["sections"]
    want = json.loads(GOLDEN.read_text())["sections"]
    for g, w in zip(got, want):
        assert g[0] == w[0], f"section '{g[0]}' where the golden has '{w[0]}'"
        assert g[1:] == w[1:], f"first section that differs: '{g[0]}' ({g[1]} lines, golden {w[1]}); see the module docstring for how to diff the text"
    assert len(got) == len(want) and len({g[0] for g in got}) == len(got)
    assert sum(g[1] for g in got) > 10000
    secs = dict(sections_of(text))
    # switching between modes that are both built allocates, uploads and frees nothing
    for name in ("back to bf16", "to fp32x again"):
        assert secs[name] and not any(l.startswith(("hipMalloc", "hipFree", "hipMemcpy", "hipMemset")) for l in secs[name].splitlines()), name
    # both contexts are torn down completely: the driver prints the stub's live-allocation count behind amuse_audio_destroy
    assert all(secs[name].endswith("live allocations after destroy: 0\n") for name in ("destroy", "tail destroy"))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":      # record: see the module docstring
        GOLDEN.write_text(json.dumps(to_golden(Path(sys.argv[2]).read_text()), indent=0, separators=(",", ":")) + "\n")
    elif len(sys.argv) == 3 and sys.argv[1] == "--dump":      # the full text of this tree's log
        with tempfile.TemporaryDirectory() as d:
            subprocess.run(["bash", str(HERE / "host_asan" / "build.sh"), d], check=True)
            Path(sys.argv[2]).write_text(run_driver(build_driver(d)))
    else:
        sys.exit("usage: test_audio_launch_args_cpu.py --record LOG | --dump FILE")
