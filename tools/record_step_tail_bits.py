"""tests/golden/step_tail_bits.npz: the bits of the bf16 / fp16 8-wave sampling kernels on the paths of their step tail (final LayerNorm, scheduler update,
the step's ancestral noise, the per-launch options) that tests/golden/sample_bits.npz, sample_bits_train.npz and step_head_bits.npz do not reach - recorded on
the build that is LOADED, i.e. once on a build of the commit a change of the step tail starts from (AMUSE_HIP_LIB names that build's library), never on the
tree under test.  tests/test_gpu_step_tail_bits.py holds every later build to them.

Usage (needs an MI355X): AMUSE_HIP_LIB=<parent build>/libamuse_hip.so PYTHONDONTWRITEBYTECODE=1 python tools/record_step_tail_bits.py [out.npz]

Cases (seed 2024, inputs from torch.Generator().manual_seed(2024), stored in the fixture; <p> = bf16, fp16):
  traj/<p>/latents, traj/<p>/traj : sample(..., return_traj=True), DDPM with T = 4, G = 2, B = 3, clip_index0 = 5 - the tail's option branch (the trajectory store)
  ragged/<p>                      : sample, DDPM with T = 4, G = 3, B = 7, clip_index0 = 1000 - two full tiles and a ragged one, the noise keyed by the GLOBAL
                                    clip, and a last step whose sigma is 0
  step/<p>/t981, step/<p>/t1      : denoise_step at B = 3, G = 2 - no update, the eps store
  taps/<p>/eps, taps/<p>/tap      : denoise_step(taps=True) at t = 981, B = 1 - the tap of the final LayerNorm (and of every block)"""
import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

SEED = 2024
PRECS = ("bf16", "fp16")
INPUTS = ("con", "emo", "sty", "x_t")


def keys():
    out = []
    for p in PRECS:
        out += [f"traj/{p}/latents", f"traj/{p}/traj", f"ragged/{p}", f"step/{p}/t981", f"step/{p}/t1", f"taps/{p}/eps", f"taps/{p}/tap"]
    return out


def inputs():
    """con, emo, sty [7, 256]; x_t [3, 128]"""
    gen = torch.Generator().manual_seed(SEED)
    cond = [torch.randn(7, 256, generator=gen) for _ in range(3)]
    return {**dict(zip(("con", "emo", "sty"), cond)), "x_t": torch.randn(3, 128, generator=gen)}


def run_all(eng, x):
    """-> {key: CPU tensor} for every key of keys(); x: inputs() (or the fixture's copies of them)."""
    from amuse_amd import scheduler as sch
    out = {}
    c = lambda n: (x["con"][:n], x["emo"][:n], x["sty"][:n])
    try:
        eng.set_schedule(sch.ddpm_table(4))
        for p in PRECS:
            eng.set_clips_per_group(2)
            lat, traj = eng.sample(*c(3), p, seed=SEED, clip_index0=5, return_traj=True)
            out[f"traj/{p}/latents"], out[f"traj/{p}/traj"] = lat.cpu(), traj.cpu()
            eng.set_clips_per_group(3)
            out[f"ragged/{p}"] = eng.sample(*c(7), p, seed=SEED, clip_index0=1000).cpu()
            eng.set_clips_per_group(2)
            for t in (981, 1):
                out[f"step/{p}/t{t}"] = eng.denoise_step(x["x_t"], t, *c(3), p).cpu()
            eps, tap = eng.denoise_step(x["x_t"][:1], 981, *c(1), p, taps=True)
            out[f"taps/{p}/eps"], out[f"taps/{p}/tap"] = eps.cpu(), tap.cpu()
    finally:
        eng.set_clips_per_group(0)
    return out


if __name__ == "__main__":
    from amuse_amd import _lib, weights as wts
    from amuse_amd.engine import HipEngine
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "tests" / "golden" / "step_tail_bits.npz"
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
