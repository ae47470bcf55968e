"""GPU: the step tail of the bf16 / fp16 8-wave sampling kernels (final LayerNorm, scheduler update, the step's ancestral noise, the per-launch options) on the
paths tests/golden/sample_bits.npz, sample_bits_train.npz and step_head_bits.npz do not reach, held to the bits of the build tests/golden/step_tail_bits.npz
was recorded on (tools/record_step_tail_bits.py, run on the parent of the commit that moved the noise draw into the reducers' early fetch): sample with
return_traj at T = 4, G = 2, B = 3, clip_index0 = 5 (latents and trajectory); sample at T = 4, G = 3, B = 7, clip_index0 = 1000 (two full tiles and a ragged
one, noise keyed by the global clip, sigma = 0 in the last step); denoise_step at t = 981 and t = 1 (B = 3, G = 2), and with taps at B = 1.  torch.equal:
the draw's counters and arithmetic and the tail's operations are the parent's, so no output bit moves."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("record_step_tail_bits", Path(__file__).resolve().parents[1] / "tools" / "record_step_tail_bits.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

SHAPES = {"traj/{p}/latents": (3, 128), "traj/{p}/traj": (4, 3, 128), "ragged/{p}": (7, 128), "step/{p}/t981": (3, 128), "step/{p}/t1": (3, 128),
          "taps/{p}/eps": (1, 128), "taps/{p}/tap": (11, 16, 128)}


@pytest.fixture(scope="module")
def got():
    """Every recorded launch, run once on the build under test."""
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    g = np.load(GOLDEN / "step_tail_bits.npz")
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
    try:
        out = rec.run_all(eng, {k: torch.from_numpy(g[k]) for k in rec.INPUTS})
    finally:
        eng.close()
    return g, out


def test_fixture_holds_exactly_the_cases():
    g = np.load(GOLDEN / "step_tail_bits.npz")
    assert sorted(g.files) == sorted(rec.keys() + list(rec.INPUTS))
    assert sorted(rec.keys()) == sorted(k.format(p=p) for k in SHAPES for p in rec.PRECS)
    for k in SHAPES:
        for p in rec.PRECS:
            a = g[k.format(p=p)]
            assert a.shape == SHAPES[k] and a.dtype == np.float32 and np.isfinite(a).all(), k.format(p=p)
    # the recorded runs did what the cases are for: the trajectory ends in the latents, and its steps differ
    for p in rec.PRECS:
        assert np.array_equal(g[f"traj/{p}/traj"][-1], g[f"traj/{p}/latents"])
        assert not np.array_equal(g[f"traj/{p}/traj"][0], g[f"traj/{p}/traj"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("key", rec.keys())
def test_step_tail_bits_equal_parent_build(got, key):
    g, out = got
    z, want = out[key], torch.from_numpy(g[key])
    assert z.shape == want.shape and z.shape[-1] == 128
    assert torch.equal(z, want), f"{int((z != want).sum())} of {z.numel()} words differ from the parent build, max |d| {float((z - want).abs().max()):.3e}"
