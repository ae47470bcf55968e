"""GPU: the sampling kernels produce the bits of the build tests/golden/sample_bits.npz was recorded on (tools/record_sample_bits.py, run on the parent of
the commit that trimmed the reducer waves' instruction stream) - every tiling (G = 1, 2, 3 clips per group; one full tile, and a second ragged one), DDPM
with T = 3 (two ring wraps at a step boundary, noise in the first two steps, none in the last) and DDIM with 2 steps, bf16 and fp16; the fp32x and fp32
kernels at one clip, because they share the Philox helper.  torch.equal: an exact pass over a kernel's instructions changes no output bit."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SEED = 2024
CASES = ([(p, s, G, B) for p in ("bf16", "fp16") for s in ("ddpm3", "ddim2") for G in (1, 2, 3) for B in (G, G + 1)]
         + [("fp32x", "ddpm3", 1, 1), ("fp32", "ddpm3", 1, 1)])


@pytest.fixture(scope="module")
def env():
    from amuse_amd import scheduler as sch
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
    g = np.load(GOLDEN / "sample_bits.npz")
    yield {"eng": eng, "g": g, "sched": {"ddpm3": sch.ddpm_table(3), "ddim2": sch.ddim_table(2)}}
    eng.set_clips_per_group(0)
    eng.close()


def test_fixture_holds_exactly_the_cases():
    g = np.load(GOLDEN / "sample_bits.npz")
    assert sorted(k for k in g.files if k.startswith("lat/")) == sorted(f"lat/{p}/{s}/G{G}/B{B}" for p, s, G, B in CASES)


@pytest.mark.parametrize("prec,smp,G,B", CASES, ids=[f"{p}-{s}-G{G}-B{B}" for p, s, G, B in CASES])
def test_sample_bits_equal_parent_build(env, prec, smp, G, B):
    eng, g = env["eng"], env["g"]
    con, emo, sty = (torch.from_numpy(g[k][:B]) for k in ("con", "emo", "sty"))
    eng.set_schedule(env["sched"][smp])
    eng.set_clips_per_group(G)
    try:
        z = eng.sample(con, emo, sty, prec, seed=SEED).cpu()
    finally:
        eng.set_clips_per_group(0)
    want = torch.from_numpy(g[f"lat/{prec}/{smp}/G{G}/B{B}"])
    assert z.shape == want.shape == (B, 128)
    assert torch.equal(z, want), f"{int((z != want).sum())} of {z.numel()} latent words differ from the parent build, max |d| {float((z - want).abs().max()):.3e}"
