"""tests/golden/step_head_bits.npz: the bits of the 8-wave sampling kernels on the paths of their step head (token assembly, the time-token buffers) that
tests/golden/sample_bits.npz does not reach - recorded on the build that is LOADED, i.e. once on a build of the commit a change of the step head starts
from (AMUSE_HIP_LIB names that build's library), never on the tree under test.  tests/test_gpu_step_head_bits.py holds every later build to them.

Usage (needs an MI355X): AMUSE_HIP_LIB=<parent build>/libamuse_hip.so PYTHONDONTWRITEBYTECODE=1 python tools/record_step_head_bits.py [out.npz]

Cases (seed 2024, inputs from torch.Generator().manual_seed(2024), stored in the fixture):
  fwd/<precision>/G<G>    : diffusion_forward (one teacher-forced step, a time token PER CLIP) at B = G + 1 for G = 1, 2, 3 with distinct timesteps
                            per clip, 0 and 999 among them; bf16, fp16, fp32x.  Two arrays each: .../noisy and .../pred
  ddpm5/<precision>       : sample, DDPM with T = 5, G = 2, B = 3 (both time-token buffers written twice behind the prologue's copy); bf16, fp32x
  given/<precision>       : sample with x_init and step_noise given, DDPM with T = 3, G = 3, B = 4; bf16, fp32x"""
import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

SEED = 2024
FWD_PRECS = ("bf16", "fp16", "fp32x")
RUN_PRECS = ("bf16", "fp32x")
FWD_TIMESTEPS = {1: (0, 999), 2: (999, 0, 417), 3: (0, 13, 999, 500)}    # G -> one timestep per clip of the G + 1


def keys():
    out = [f"fwd/{p}/G{G}/{w}" for p in FWD_PRECS for G in (1, 2, 3) for w in ("noisy", "pred")]
    return out + [f"ddpm5/{p}" for p in RUN_PRECS] + [f"given/{p}" for p in RUN_PRECS]


def inputs():
    """con, emo, sty [4, 256]; z0, noise, x_init [4, 128]; step_noise [3, 4, 128]"""
    gen = torch.Generator().manual_seed(SEED)
    cond = [torch.randn(4, 256, generator=gen) for _ in range(3)]
    lat = [torch.randn(4, 128, generator=gen) for _ in range(3)]
    return {**dict(zip(("con", "emo", "sty"), cond)), **dict(zip(("z0", "noise", "x_init"), lat)), "step_noise": torch.randn(3, 4, 128, generator=gen)}


def run_all(eng, x):
    """-> {key: CPU tensor} for every key of keys(); x: inputs() (or the fixture's copies of them)."""
    from amuse_amd import scheduler as sch
    out = {}
    try:
        for G in (1, 2, 3):
            B = G + 1
            eng.set_clips_per_group(G)
            for p in FWD_PRECS:
                o = eng.diffusion_forward(x["z0"][:B], x["noise"][:B], FWD_TIMESTEPS[G], x["con"][:B], x["emo"][:B], x["sty"][:B], p)
                out[f"fwd/{p}/G{G}/noisy"], out[f"fwd/{p}/G{G}/pred"] = o["noisy_latents"].cpu(), o["noise_pred"].cpu()
        eng.set_schedule(sch.ddpm_table(5))
        eng.set_clips_per_group(2)
        for p in RUN_PRECS:
            out[f"ddpm5/{p}"] = eng.sample(x["con"][:3], x["emo"][:3], x["sty"][:3], p, seed=SEED).cpu()
        eng.set_schedule(sch.ddpm_table(3))
        eng.set_clips_per_group(3)
        for p in RUN_PRECS:
            out[f"given/{p}"] = eng.sample(x["con"], x["emo"], x["sty"], p, seed=SEED, x_init=x["x_init"], step_noise=x["step_noise"]).cpu()
    finally:
        eng.set_clips_per_group(0)
    return out


if __name__ == "__main__":
    from amuse_amd import _lib, weights as wts
    from amuse_amd.engine import HipEngine
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "tests" / "golden" / "step_head_bits.npz"
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
    x = inputs()
    rec = {k: v.numpy() for k, v in x.items()}
    for k, v in run_all(eng, x).items():
        assert bool(torch.isfinite(v).all()), k
        rec[k] = v.numpy()
    eng.close()
    assert sorted(k for k in rec if "/" in k) == sorted(keys())
    out_path.parent.mkdir(parents=True, exist_ok=True)
    np.savez(out_path, **rec)
    print(f"recorded {len(rec)} arrays from {os.path.basename(str(_lib.LIB_PATH))} -> {out_path} ({out_path.stat().st_size} bytes)")
