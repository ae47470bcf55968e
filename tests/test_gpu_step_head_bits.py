"""GPU: token assembly of the 8-wave sampling kernels (the step's input rows, the double-buffered time token) on the paths tests/golden/sample_bits.npz
does not reach, held to the bits of the build tests/golden/step_head_bits.npz was recorded on (tools/record_step_head_bits.py, run on the parent of the
commit that moved the assembly from every wave's step head into the reducers' tail): diffusion_forward - a time token per clip - at B = G + 1 for G = 1, 2, 3 with distinct timesteps, 0 and 999 among
them, in bf16, fp16 and fp32x; DDPM with T = 5 at G = 2, B = 3 (both time-token buffers written twice); and sample with x_init and step_noise given
(T = 3, G = 3, B = 4).  torch.equal: the assembly's operands, selects and adds are the parent's, so no output bit moves."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_step_head_bits", Path(__file__).resolve().parents[1] / "tools" / "record_step_head_bits.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def got():
    """Every recorded launch, run once on the build under test."""
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    g = np.load(GOLDEN / "step_head_bits.npz")
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
    try:
        out = rec.run_all(eng, {k: torch.from_numpy(g[k]) for k in ("con", "emo", "sty", "z0", "noise", "x_init", "step_noise")})
    finally:
        eng.close()
    return g, out


def test_fixture_holds_exactly_the_cases():
    g = np.load(GOLDEN / "step_head_bits.npz")
    assert sorted(k for k in g.files if "/" in k) == sorted(rec.keys())


@pytest.mark.parametrize("key", rec.keys())
def test_step_head_bits_equal_parent_build(got, key):
    g, out = got
    z, want = out[key], torch.from_numpy(g[key])
    assert z.shape == want.shape and z.shape[1:] == (128,)
    assert torch.equal(z, want), f"{int((z != want).sum())} of {z.numel()} words differ from the parent build, max |d| {float((z - want).abs().max()):.3e}"
