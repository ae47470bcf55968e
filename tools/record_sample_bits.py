"""tests/golden/sample_bits.npz: the bits the sampling kernels and the counter-based normals produce on the build that is LOADED - recorded once on a build
of the commit a kernel change starts from (AMUSE_HIP_LIB names that build's library), never on the tree under test.  tests/test_gpu_sample_bits.py and
tests/test_gpu_philox_bits.py then hold every later build to these bits with torch.equal.

Usage (needs an MI355X): AMUSE_HIP_LIB=<parent build>/libamuse_hip.so PYTHONDONTWRITEBYTECODE=1 python tools/record_sample_bits.py [out.npz]

Cases (seed 2024, inputs from torch.Generator().manual_seed(2024), stored in the fixture):
  bf16, fp16 : clips per group G = 1, 2, 3 (set_clips_per_group) x B = G (one full tile), G + 1 (a second, ragged tile) x DDPM with T = 3, DDIM with 2 steps
  fp32x, fp32: B = 1, DDPM with T = 3 (they share the Philox helper)
  normals    : counter_normal for a handful of (seed, first clip, step, stream) keys, two clips each
Keys: lat/<precision>/<sampler>/G<G>/B<B>, normal/<n> with normal_keys[n] = (seed, clip_index0, step, stream)."""
import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

SEED = 2024
SAMPLERS = ("ddpm3", "ddim2")
# the first three are the ancestral noise (stream 1) of steps 0..2 of the seed-2024 runs above; stream 0 is the initial latent
NORMAL_KEYS = ((2024, 0, 0, 1), (2024, 0, 1, 1), (2024, 0, 2, 1), (2024, 0, 0, 0), (1, 5, 999, 1), (0xDEADBEEFCAFEF00D, (1 << 32) + 7, 3, 1), (0, 0, 0, 1))


def cases():
    """(precision, sampler, G, B) of every recorded launch."""
    out = []
    for prec in ("bf16", "fp16"):
        for smp in SAMPLERS:
            for G in (1, 2, 3):
                for B in (G, G + 1):
                    out.append((prec, smp, G, B))
    out += [("fp32x", "ddpm3", 1, 1), ("fp32", "ddpm3", 1, 1)]
    return out


def schedule(name):
    from amuse_amd import scheduler as sch
    return sch.ddpm_table(3) if name == "ddpm3" else sch.ddim_table(2)


def inputs():
    gen = torch.Generator().manual_seed(SEED)
    return tuple(torch.randn(4, 256, generator=gen) for _ in range(3))


def run_case(eng, con, emo, sty, prec, smp, G, B):
    eng.set_schedule(schedule(smp))
    eng.set_clips_per_group(G)
    try:
        return eng.sample(con[:B], emo[:B], sty[:B], prec, seed=SEED).cpu()
    finally:
        eng.set_clips_per_group(0)


if __name__ == "__main__":
    from amuse_amd import _lib, weights as wts
    from amuse_amd.engine import HipEngine
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "tests" / "golden" / "sample_bits.npz"
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
    con, emo, sty = inputs()
    rec = {"con": con.numpy(), "emo": emo.numpy(), "sty": sty.numpy(), "normal_keys": np.array(NORMAL_KEYS, dtype=np.uint64)}
    for prec, smp, G, B in cases():
        z = run_case(eng, con, emo, sty, prec, smp, G, B)
        assert bool(torch.isfinite(z).all()), (prec, smp, G, B)
        rec[f"lat/{prec}/{smp}/G{G}/B{B}"] = z.numpy()
    for n, (seed, clip0, step, stream) in enumerate(NORMAL_KEYS):
        rec[f"normal/{n}"] = eng.counter_normal(seed, clip0, 2, step, stream).cpu().numpy()
    eng.close()
    out_path.parent.mkdir(parents=True, exist_ok=True)
    np.savez(out_path, **rec)
    print(f"recorded {len(rec)} arrays from {os.path.basename(str(_lib.LIB_PATH))} -> {out_path} ({out_path.stat().st_size} bytes)")
