"""CPU: every kernel launch and runtime call of the training step's host code (csrc/amuse_train.hip and the launchers of k_train.hip, k_train_attn.hip,
k_train_gemm.hip), with all arguments and in order, against tests/golden/train_launch_args.json; and its error paths.
tests/train_host/ links those translation units as they are (host side only) against the stubbed HIP runtime of tests/host_asan at its raw launch level
(hip_stub.cpp, amuse_stub_log(3)): a kernel registers under its mangled name, every <<< >>> prints kernel, grid, block, dynamic LDS bytes, stream and - through the
driver's table of parameter letters - its pointer and scalar arguments (structs passed by value, AttnArgs and LayerSums, are skipped and say so), every runtime call
its sizes and handles.  Pointers print as in tests/test_launch_args_cpu.py; every pointer field of amuse_train_layer has a named address of its own.  The golden holds,
per section in order, the line count and the SHA-256 of the section's text: every raw entry point, linear_fwd / _bwd at one shape per branch of the GEMM dispatch,
the attention entry points, the optimizer and epoch calls, layer_fwd / _bwd of encoder and decoder layers below and from 1,024 rows, on both lanes.

The golden file was recorded ONCE, with this driver and stub, from the library sources of the commit BEFORE the training host code moved into amuse_train.hip
(one launcher per kernel, the stream a parameter, the layer pass an object, one per-device state):
`CSRC=<that commit's amuse_amd/csrc> tests/train_host/build.sh DIR && DIR/train_host sections > LOG && python tests/test_train_launch_args_cpu.py --record LOG`.
It is never regenerated from refactored host code: a change that moves a launch, an argument or a runtime call is a change of behaviour and says so.  To see WHAT
differs when a section's digest does: build both trees that way, run `DIR/train_host sections` of each and diff the two texts.

The error paths are not in the golden - the sources it was recorded from behave differently there by design (`DIR/train_host overflow` on them: the layer whose
weight-gradient partials exceed the workspace is refused after 16 launches, with the side stream forked and not joined) - the program asserts them itself: a refused
layer call (dqkv or lse missing with Win set, weight-gradient partials beyond the workspace) makes no runtime call and no launch; with the n-th runtime call or launch
failing, for every n between fork and join of the decoder layer with 1,200 rows, the call returns an error, the side stream's join record and the caller stream's wait
follow, and no launch does; without the epoch word (its allocation failing, `train_host noepoch`) every mask-drawing entry point returns AMUSE_EHIP without a launch.
What is live at exit is the per-device training state, which the library keeps for the life of the process, and nothing else."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "train_launch_args.json"
# the epoch word; per lane the weight-gradient workspace, the side stream and its two events; lane 0's split-k workspace
LIVE_AT_EXIT = 1 + 2 * (1 + 3) + 1


def sections_of(text):
    """[(name, text of the section)] of a driver log, in order; lines from the first `-- ` line on belong to no section."""
    secs = []
    for line in text.splitlines():
        if line.startswith("-- "):
            break
        if line.startswith("== "):
            secs.append((line[3:], []))
        elif secs:
            secs[-1][1].append(line)
    return [(name, "".join(l + "\n" for l in lines)) for name, lines in secs]


def to_golden(text):
    return {"sections": [[name, body.count("\n"), hashlib.sha256(body.encode()).hexdigest()] for name, body in sections_of(text)]}


def run_driver(build_dir, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(Path(build_dir) / "train_host"), *args], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0 and run.stdout.endswith("train_host ok\n"), run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    return run.stdout


@pytest.fixture(scope="module")
def train_host_build(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("train_host")
    build = subprocess.run(["bash", str(HERE / "train_host" / "build.sh"), str(out)], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-3000:]
    return out


def test_train_launches_arguments_and_runtime_calls_match_the_golden(train_host_build):
    text = run_driver(train_host_build)
    got = to_golden(text)["sections"]
    want = json.loads(GOLDEN.read_text())["sections"]
    for g, w in zip(got, want):
        assert g[0] == w[0], f"section '{g[0]}' where the golden has '{w[0]}'"
        assert g[1:] == w[1:], f"first section that differs: '{g[0]}' ({g[1]} lines, golden {w[1]}); see the module docstring for how to diff the text"
    assert len(got) == len(want) and len({g[0] for g in got}) == len(got)
    assert sum(g[1] for g in got) > 350
    # the error paths behind the sections ran to their end
    assert "failures between fork and join: all joined\n" in text
    assert text.endswith(f"live allocations at exit: {LIVE_AT_EXIT}\ntrain_host ok\n"), text[-300:]


def test_no_epoch_word_is_an_error_in_every_mask_drawing_entry_point(train_host_build):
    text = run_driver(train_host_build, "noepoch")
    assert text.endswith("-- 10 entry points refuse without the epoch word\nlive allocations at exit: 0\ntrain_host ok\n"), text[-300:]
    assert "launch " not in text


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":      # record: see the module docstring
        GOLDEN.write_text(json.dumps(to_golden(Path(sys.argv[2]).read_text()), indent=0, separators=(",", ":")) + "\n")
    else:
        sys.exit("usage: test_train_launch_args_cpu.py --record LOG")
