"""CPU: the C ABI of the audio front-end's precision switch (include/amuse_hip.h amuse_audio_set_precision / amuse_audio_precision): declared, exported,
argument checks without a GPU - and the link constraint behind its structure: the parity mode lives in a translation unit of its own (csrc/amuse_audio_x.hip)
that amuse_audio_api.hip reaches through a weak reference, so the host-only build of tests/host_asan/build.sh (whose runtime stub defines the bf16 launchers
alone) still links, and refuses the mode there."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
HERE = REPO / "tests" / "host_asan"


def test_header_declares_and_library_exports_the_switch():
    from amuse_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include/amuse_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+amuse_audio_set_precision\s*\(\s*amuse_audio_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+amuse_audio_precision\s*\(\s*const\s+amuse_audio_ctx\s*\*\s*\w+\s*\)\s*;", hdr)
    assert int(re.search(r"#define AMUSE_ABI_VERSION (\d+)", hdr).group(1)) == 5
    lib = _lib.load()
    assert hasattr(lib, "amuse_audio_set_precision") and hasattr(lib, "amuse_audio_precision")
    assert {"amuse_audio_set_precision", "amuse_audio_precision"} <= set(_lib.EXPORTS)
    # the full library carries the mode's translation unit
    assert hasattr(lib, "amuse_audio_x_ops")


def test_null_context_is_refused_without_touching_a_gpu():
    from amuse_amd import _lib
    lib = _lib.load()
    for prec in (_lib.PREC_BF16, _lib.PREC_F32X, 7):
        assert lib.amuse_audio_set_precision(None, prec) == -1          # AMUSE_EINVAL
    assert b"NULL" in lib.amuse_last_error()
    assert lib.amuse_audio_precision(None) == -1


def test_engine_rejects_unknown_precision_names_before_any_call():
    import pytest
    from amuse_amd import audio
    assert audio.AUDIO_PREC == {"bf16": 1, "fp32x": 2}
    eng = audio.AudioEngine.__new__(audio.AudioEngine)   # no context: the name check comes first
    with pytest.raises(ValueError):
        eng.set_precision("fp16")


def test_stub_build_links_and_refuses_the_parity_mode(host_asan_build):
    """The regression check of the link constraint: tests/host_asan/build.sh (unchanged) has just linked three programs from amuse_audio_api.o and the
    stub - had that object referenced a launcher of the parity mode, the fixture would have failed.  On the same objects: AMUSE_PREC_F32X -> AMUSE_ESTATE,
    AMUSE_PREC_BF16 -> OK, anything else -> AMUSE_EINVAL (tests/host_asan/audio_precision.cpp), under ASan / UBSan."""
    out = host_asan_build
    san = "-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1".split()
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    objs = [str(out / f) for f in ("hip_stub.o", "amuse_api.o", "amuse_variants.o", "amuse_audio_api.o")]
    subprocess.run([cxx, "-std=c++17", *san, "-c", str(HERE / "audio_precision.cpp"), "-o", str(out / "audio_precision.o")], check=True, capture_output=True, timeout=600)
    link = subprocess.run([cxx, *san, str(out / "audio_precision.o"), *objs, "-o", str(out / "audio_precision")], capture_output=True, text=True, timeout=600)
    assert link.returncode == 0, link.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([str(out / "audio_precision")], capture_output=True, text=True, timeout=900, env=env, cwd=str(out))
    assert run.returncode == 0 and "AUDIO PRECISION STUB OK" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
