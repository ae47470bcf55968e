"""CPU: the train-mode sampling switch (amuse_set_sample_dropout) - exported and declared, its argument checks, the trainer's option without a
GPU, and the mask contract written into the header (tests/test_gpu_sample_dropout.py restates it against the kernels)."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def test_symbol_is_exported_and_declared():
    from amuse_amd import _lib
    lib = _lib.load()
    assert "amuse_set_sample_dropout" in _lib.EXPORTS and hasattr(lib, "amuse_set_sample_dropout")
    hdr = (REPO / "include/amuse_hip.h").read_text()
    assert re.search(r"int amuse_set_sample_dropout\(amuse_ctx\* ctx, float p, uint64_t seed\);", hdr)
    assert int(re.search(r"#define AMUSE_ABI_VERSION (\d+)", hdr).group(1)) == 5


@pytest.mark.parametrize("p", [float("nan"), -0.1, 1.0, 1.5, float("inf")])
def test_bad_probability_is_einval(p):
    from amuse_amd import _lib
    lib = _lib.load()
    assert lib.amuse_set_sample_dropout(None, p, 1) == -1          # AMUSE_EINVAL
    assert b"dropout probability" in lib.amuse_last_error()


def test_null_context_is_einval():
    from amuse_amd import _lib
    lib = _lib.load()
    for p in (0.0, 0.1, 0.999):
        assert lib.amuse_set_sample_dropout(None, p, 1) == -1
        assert b"ctx is NULL" in lib.amuse_last_error()


def test_train_hip_inner_sampler_has_no_cpu_path():
    from amuse_amd.train_gesture import build_trainer
    with pytest.raises(RuntimeError, match="train-hip"):
        build_trainer("cpu", inner="train-hip")
    with pytest.raises(ValueError, match="train-hip"):
        build_trainer("cpu", inner="bogus")


def test_header_states_the_mask_contract():
    hdr = (REPO / "include/amuse_hip.h").read_text()
    i = hdr.index("int amuse_set_sample_dropout(")
    doc = hdr[hdr.rindex("/*", 0, i):i]
    for field in ("Philox4x32-10", "(clip, step, ((l 4 + s) << 16) | (e / 4), 2 + epoch)", "(h S + q) S + k", "tok 128 + f", "tok 512 + f",
                  "(draw >> 8) >= thr", "thr = (uint32)(p 2^24)", "1 / (1 - p)", "AMUSE_ESTATE", "AMUSE_PREC_F32X", "amuse_denoise_step"):
        assert field in doc, field
    assert "AMUSE_TRAIN_INNER=eval|train|train-hip" in hdr
    assert "train-hip" in (REPO / "INTEGRATION.md").read_text()
