"""Cost of train-mode sampling (amuse_set_sample_dropout): engine.sample in bf16 with the Denoiser's dropouts off (p = 0, the eval kernel) and live
(p = 0.1, the dropout instantiation) at the in-loop sampler's shape (B = 32, DDIM-50) and at the throughput job's (256 clips, DDPM-1000), plus the
phase timeline of one step (s_memtime stamps, amuse_profile_sample) of both instantiations: where the Philox work lands.
Usage: python tools/gpu_sample_dropout_perf.py [reps]"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amuse_amd import scheduler as sch, weights as wts  # noqa: E402
from amuse_amd.engine import HipEngine  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0))
gen = torch.Generator().manual_seed(2)


def timed(B, table, p, n):
    eng.set_schedule(table)
    eng.set_sample_dropout(p, 7)
    c, e, s = (torch.randn(B, 256, generator=gen).cuda() for _ in range(3))
    for _ in range(2):
        eng.sample(c, e, s, "bf16", seed=1)
    torch.cuda.synchronize()
    ms = []
    for i in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.sample(c, e, s, "bf16", seed=1, clip_index0=B * i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


print(f"engine.sample, bf16 (k_sample8), median / min of {reps} calls (CUDA events)")
rows = []
for B, name, table, n in ((32, "DDIM-50", sch.ddim_table(), reps), (256, "DDPM-1000", sch.ddpm_table(1000), max(3, reps // 4))):
    base = None
    for p in (0.0, 0.1):
        med, mn = timed(B, table, p, n)
        base = med if p == 0 else base
        print(f"  B = {B:3d} x {name:9s}  p = {p:.1f}: {med:9.3f} ms (min {mn:9.3f})   x {med / base:.3f} of p = 0")

eng.set_schedule(sch.ddpm_table(50))
c, e, s = (torch.randn(256, 256, generator=gen).cuda() for _ in range(3))
print("\nphase timeline of step 3 (256 clips, ticks of workgroup 0's waves; A = wave 0, B = wave 4), sums over the 9 blocks")
names = ["pre(skip)", "attn+out_proj", "combine1", "FFN", "combine2"]
for p in (0.0, 0.1):
    eng.set_sample_dropout(p, 7)
    st = eng.profile_sample(c, e, s, "bf16", prof_step=3).astype(np.int64).reshape(8, 96)
    for w in (0, 4):
        v = st[w]
        v = v[:int((v != 0).sum())]
        # stamps: step top | step start (behind the head) | 9 blocks x 5 | tail | the next step's top
        blocks = v[2:2 + 45].reshape(9, 5)
        prev = np.concatenate([[v[1]], blocks[:-1, -1]])
        seg = np.diff(np.concatenate([prev[:, None], blocks], axis=1), axis=1).sum(axis=0)
        print(f"  p = {p:.1f} wave {w}: step {int(v[47] - v[0]):7d}  head {int(v[1] - v[0]):5d}  " + "  ".join(f"{nm} {int(x):6d}" for nm, x in zip(names, seg)))
eng.close()
