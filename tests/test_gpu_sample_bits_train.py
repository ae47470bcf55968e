"""GPU: the TRAIN-MODE instantiations of the 8-wave sampling kernels (set_sample_dropout: the Denoiser's encoder dropouts live in every step) produce the bits
of the build tests/golden/sample_bits_train.npz was recorded on (tools/record_sample_bits_train.py, run on the parent of the commit that moved the A waves'
last FFN units from the out_proj combine's tail into their FFN half) - they share ffn_half and the combines with the eval instantiations, which
tests/test_gpu_sample_bits.py covers.  bf16 and fp16, G = 1, 2, 3 clips per group with B = G + 1 clips (one full tile and a ragged one), DDPM with T = 3 (a
ring wrap at each step boundary), p = 0.1 (train_gesture's default).  torch.equal: a change of issue points changes no output bit.

The library's dropout epoch enters the mask key and belongs to the process, not to the engine: every launch runs as the first sampling call of a fresh
engine with the epoch set to 0, as the recording did, and two fresh engines must agree before the fixture is trusted."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN

SEED, DROP_P, DROP_SEED, T = 2024, 0.1, 2025, 3
CASES = [(p, G, G + 1) for p in ("bf16", "fp16") for G in (1, 2, 3)]


def _fixture():
    return np.load(GOLDEN / "sample_bits_train.npz")


@pytest.fixture(scope="module")
def weights():
    from amuse_amd import weights as wts
    return wts.make_denoiser_weights(0), wts.make_prior_weights(0)


def _run(weights, g, prec, G, B):
    from amuse_amd import _lib, scheduler as sch
    from amuse_amd.engine import HipEngine
    con, emo, sty = (torch.from_numpy(g[k][:B]) for k in ("con", "emo", "sty"))
    eng = HipEngine(*weights, "cuda:0")
    try:
        _lib.check(eng.lib.amuse_train_epoch_set(0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        eng.set_schedule(sch.ddpm_table(T))
        eng.set_clips_per_group(G)
        eng.set_sample_dropout(DROP_P, DROP_SEED)
        return eng.sample(con, emo, sty, prec, seed=SEED).cpu()
    finally:
        eng.set_sample_dropout(0.0, 0)
        eng.set_clips_per_group(0)
        eng.close()


def test_fixture_holds_exactly_the_cases_and_dropout_was_live():
    g, ev = _fixture(), np.load(GOLDEN / "sample_bits.npz")
    assert sorted(k for k in g.files if k.startswith("lat/")) == sorted(f"lat/{p}/G{G}/B{B}" for p, G, B in CASES)
    for k in ("con", "emo", "sty"):
        assert np.array_equal(g[k], ev[k])
    # same inputs, seed and schedule as the eval fixture: with the dropouts live every clip's latent differs from it
    for p, G, B in CASES:
        assert (g[f"lat/{p}/G{G}/B{B}"] != ev[f"lat/{p}/ddpm3/G{G}/B{B}"]).any(axis=1).all(), (p, G, B)


@pytest.mark.gpu
def test_two_fresh_engines_agree(weights):
    g = _fixture()
    a, b = _run(weights, g, "bf16", 2, 3), _run(weights, g, "bf16", 2, 3)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,G,B", CASES, ids=[f"{p}-G{G}-B{B}" for p, G, B in CASES])
def test_train_mode_sample_bits_equal_parent_build(weights, prec, G, B):
    g = _fixture()
    z = _run(weights, g, prec, G, B)
    want = torch.from_numpy(g[f"lat/{prec}/G{G}/B{B}"])
    assert z.shape == want.shape == (B, 128)
    assert torch.equal(z, want), f"{int((z != want).sum())} of {z.numel()} latent words differ from the parent build, max |d| {float((z - want).abs().max()):.3e}"
