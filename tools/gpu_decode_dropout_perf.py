"""Cost of train-mode decode (amuse_set_decode_dropout): engine.vae_decode on the staged kernels with the decoder's dropouts off (p = 0, the eval kernels,
decode path pinned to "staged" so that both rows run the same family) and live (p = 0.1, the dropout instantiations) at the in-loop sampler's shape
(32 clips) and at the throughput job's (256 clips), bf16 and fp32: warm-up, then `reps` calls timed one by one with events; median, min and max.
The trainer's it/s for the three inner samplers come from bench.py (profiles/decode_dropout_cost.txt lists the commands).
Usage: python tools/gpu_decode_dropout_perf.py [reps]"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amuse_amd import scheduler as sch, weights as wts  # noqa: E402
from amuse_amd.engine import HipEngine  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0))
eng.set_schedule(sch.ddim_table())
eng.set_decode_path("staged")
gen = torch.Generator().manual_seed(2)


def timed(B, prec, p):
    eng.set_decode_dropout(p, 7, 0)
    z = torch.randn(B, 128, generator=gen).cuda()
    for _ in range(3):
        eng.vae_decode(z, None, prec)
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        eng.set_decode_dropout(p, 7, B * i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.vae_decode(z, None, prec)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


print(f"engine.vae_decode on the staged kernels (19 launches + the cross-attention prologue), median / min / max of {reps} calls (events around each call)")
for prec in ("bf16", "fp32"):
    for B in (32, 256):
        base = None
        for p in (0.0, 0.1):
            med, mn, mx = timed(B, prec, p)
            base = med if p == 0 else base
            print(f"  {prec} B = {B:3d}  p = {p:.1f}: {med:8.3f} ms (min {mn:8.3f}, max {mx:8.3f})   x {med / base:.3f} of p = 0")
eng.close()
