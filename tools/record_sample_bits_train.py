"""tests/golden/sample_bits_train.npz: the bits the TRAIN-MODE instantiations of the 8-wave sampling kernels (set_sample_dropout: the Denoiser's encoder dropouts
live in every step) produce on the build that is LOADED - recorded once on a build of the commit a kernel change starts from (AMUSE_HIP_LIB names that build's
library), never on the tree under test.  tests/test_gpu_sample_bits_train.py then holds every later build to these bits with torch.equal; the eval
instantiations have tests/golden/sample_bits.npz (tools/record_sample_bits.py), whose inputs and seed this fixture shares.

Usage (needs an MI355X): AMUSE_HIP_LIB=<parent build>/libamuse_hip.so PYTHONDONTWRITEBYTECODE=1 python tools/record_sample_bits_train.py [out.npz]

Cases: bf16, fp16 x clips per group G = 1, 2, 3 (set_clips_per_group) with B = G + 1 clips (one full tile and a ragged one) x DDPM with T = 3 (a ring wrap
at each step boundary), dropout p = 0.1 (train_gesture's default) with mask seed 2025, sampling seed 2024.
The library's dropout epoch enters the mask key and is a word of the process, not of the engine: every launch runs on a FRESH engine as its first sampling
call, with the epoch set to 0 in front of it - the replay (run_case, which the test imports) does exactly the same.
Keys: lat/<precision>/G<G>/B<B>, and con / emo / sty."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

SEED = 2024          # sampling seed (initial latent, ancestral noise) and the inputs' generator seed
DROP_P = 0.1         # train_gesture.build_trainer(dropout=0.1)
DROP_SEED = 2025
T = 3


def cases():
    """(precision, G, B) of every recorded launch."""
    return [(prec, G, G + 1) for prec in ("bf16", "fp16") for G in (1, 2, 3)]


def inputs():
    gen = torch.Generator().manual_seed(SEED)
    return tuple(torch.randn(4, 256, generator=gen) for _ in range(3))


def run_case(weights, con, emo, sty, prec, G, B):
    """One launch on a fresh engine, dropout epoch 0, as that engine's first sampling call."""
    from amuse_amd import _lib, scheduler as sch
    from amuse_amd.engine import HipEngine
    eng = HipEngine(*weights, "cuda:0")
    try:
        _lib.check(eng.lib.amuse_train_epoch_set(0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        eng.set_schedule(sch.ddpm_table(T))
        eng.set_clips_per_group(G)
        eng.set_sample_dropout(DROP_P, DROP_SEED)
        return eng.sample(con[:B], emo[:B], sty[:B], prec, seed=SEED).cpu()
    finally:
        eng.set_sample_dropout(0.0, 0)
        eng.set_clips_per_group(0)
        eng.close()


if __name__ == "__main__":
    from amuse_amd import _lib, weights as wts
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "tests" / "golden" / "sample_bits_train.npz"
    weights = (wts.make_denoiser_weights(0), wts.make_prior_weights(0))
    con, emo, sty = inputs()
    rec = {"con": con.numpy(), "emo": emo.numpy(), "sty": sty.numpy()}
    for prec, G, B in cases():
        z = run_case(weights, con, emo, sty, prec, G, B)
        again = run_case(weights, con, emo, sty, prec, G, B)
        assert bool(torch.isfinite(z).all()), (prec, G, B)
        assert torch.equal(z, again), ("two fresh engines disagree", prec, G, B)
        rec[f"lat/{prec}/G{G}/B{B}"] = z.numpy()
    np.savez(out_path, **rec)
    print(f"recorded {len(rec)} arrays from {os.path.basename(str(_lib.LIB_PATH))} -> {out_path} ({out_path.stat().st_size} bytes)")
