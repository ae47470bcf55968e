"""GPU: Philox4x32-10 on its own.  The counter-based normals (amuse_dev.hpp counter_normal4, shared by every kernel that draws noise) for a handful of
(seed, first clip, step, stream) keys are the bits tests/golden/sample_bits.npz holds, recorded from the parent build by tools/record_sample_bits.py; and
the draws the sampling kernel makes IN its step loop are those same values: a run without step_noise equals, bit for bit, a run fed the recorded draws."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
    yield {"eng": eng, "g": np.load(GOLDEN / "sample_bits.npz")}
    eng.close()


def test_counter_normals_equal_parent_build(env):
    eng, g = env["eng"], env["g"]
    keys = g["normal_keys"]
    assert len(keys) >= 5
    for n, (seed, clip0, step, stream) in enumerate(tuple(int(v) for v in row) for row in keys):
        z = eng.counter_normal(seed, clip0, 2, step, stream).cpu()
        want = torch.from_numpy(g[f"normal/{n}"])
        assert torch.equal(z, want), (n, seed, clip0, step, stream, int((z != want).sum()))
    # the keys are told apart: no two recorded draws are the same
    assert len({g[f"normal/{n}"].tobytes() for n in range(len(keys))}) == len(keys)


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32x", "fp32"])
def test_in_kernel_draws_are_the_recorded_normals(env, prec):
    """DDPM, T = 3, two clips, seed 2024: the kernel's own ancestral noise (stream 1 of steps 0..2; the last step's sigma is 0) against step_noise
    assembled from the recorded draws."""
    from amuse_amd import scheduler as sch
    eng, g = env["eng"], env["g"]
    keys = [tuple(int(v) for v in row) for row in g["normal_keys"]]
    assert keys[:3] == [(2024, 0, 0, 1), (2024, 0, 1, 1), (2024, 0, 2, 1)]
    noise = torch.from_numpy(np.stack([g["normal/0"], g["normal/1"], g["normal/2"]]))   # (T, B, 128)
    con, emo, sty = (torch.from_numpy(g[k][:2]) for k in ("con", "emo", "sty"))
    x0 = torch.from_numpy(g["normal/3"])    # (2024, 0, 0, stream 0): the initial latent the kernel draws itself
    eng.set_schedule(sch.ddpm_table(3))
    drawn = eng.sample(con, emo, sty, prec, seed=2024).cpu()
    fed = eng.sample(con, emo, sty, prec, seed=2024, x_init=x0, step_noise=noise).cpu()
    assert torch.equal(drawn, fed), int((drawn != fed).sum())
    # and the noise matters: without it the result is another one
    assert not torch.equal(drawn, eng.sample(con, emo, sty, prec, seed=2024, x_init=x0, step_noise=torch.zeros_like(noise)).cpu())
