"""CPU: tests/beat_host/ - the beat alignment's host code (csrc/amuse_beat_host.hpp through the entry points of csrc/amuse_beat.hip: the frame plan, the
defaults, the row table, every parameter and argument refusal, the context and its reserved envelope, what a call hands to its launches) in a stand-alone
program (its own main, stand-in launchers) under AddressSanitizer / UBSan, on the stubbed HIP runtime of tests/host_asan (compiled unchanged).  Nothing loaded
into Python runs under a sanitizer.  The second test makes the calls that need no GPU on the built library itself."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def test_beat_host_program_under_asan_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("hipcc not available")
    build = subprocess.run(["bash", str(REPO / "tests" / "build_host_program.sh"), "beat", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
    run = subprocess.run([str(tmp_path / "beat_host")], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stdout.strip().endswith("beat_host ok"), run.stdout[-2000:] + run.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


def test_library_plan_defaults_and_refusals_without_a_gpu():
    from amuse_amd import _lib, beat_align as ba
    import beat_ref as br
    lib = _lib.load()
    err = lambda: lib.amuse_last_error().decode()
    for n in (0, 399, 400, 560, 3120, 32000, 170000, 1920000):
        assert ba.plan(n) == br.frames_of(n)
    with pytest.raises(_lib.AmuseHipError):
        ba.plan(-1)
    assert ba.default_params() == br.DEFAULTS and lib.amuse_beat_align_row() == ba.ROW == 166
    one = 0x1000                                              # (a non-null address that is never dereferenced: every call below fails in its checks)
    assert lib.amuse_beat_pick(one, one, 1, 0, None, one, None) != 0 and "T 0" in err()
    assert lib.amuse_beat_pick(None, one, 1, 5, None, one, None) != 0 and "envelope_dev" in err()
    assert lib.amuse_beat_align(one, one, 5, one, one, 1, 1, None, one, None, None) != 0 and "F 1" in err()
    assert lib.amuse_beat_align(one, one, 131073, one, one, 1, 2, None, one, None, None) != 0 and "131072" in err()
    assert lib.amuse_beat_onsets(None, one, None, 400, 1, None, one, one, None) != 0 and "ctx" in err()
    p = ba._params({"sigma_s": 0.0})
    assert lib.amuse_beat_pick(one, one, 1, 5, C.byref(p), one, None) != 0 and "sigma_s" in err()
    p = ba._params({"motion_order": 33})
    assert lib.amuse_beat_align(one, one, 5, one, one, 1, 2, C.byref(p), one, None, None) != 0 and "motion_order" in err()
    with pytest.raises(ValueError):
        ba._params({"sigma": 0.1})
    assert not lib.amuse_beat_create(0, None, None) and "mel_banks" in err()


def test_main_refuses_beat_align_before_anything_is_loaded(tmp_path):
    """--beat-align's argument checks, in the manner of --motion-metrics: the wrong --fn, no models directory, missing model files - each a SystemExit that names
    the switch, raised before a configuration is read (the --root does not even exist)"""
    from amuse_amd import main as cli
    base = ["--root", str(tmp_path / "no_such_tree"), "--random-init", "--beat-align"]
    for argv, word in ((["--fn", "infer_gesture"] + base, "--smplx-models"),
                       (["--fn", "infer_gesture"] + base + ["--smplx-models", str(tmp_path)], "not all found"),
                       (["--fn", "edit_gesture"] + base + ["--smplx-models", str(tmp_path)], "infer_gesture"),
                       (["--fn", "train_gesture"] + base + ["--smplx-models", str(tmp_path)], "infer_gesture")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert "--beat-align" in str(e.value) and word in str(e.value), (argv, e.value)
