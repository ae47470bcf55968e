"""Phase timeline of one denoising step of the 8-wave sampling kernels (s_memtime stamps, [8 waves][96]; the step head - token assembly and wave 4's
time-token copy - is the column `head`, and the step is timed top to top of consecutive steps): bf16 (k_sample8) or,
with a second argument fp32x, k_sample8x.  Usage: python tools/gpu_phase_profile8.py [clips] [bf16|fp32x]"""
import sys
from pathlib import Path
import numpy as np, torch
REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amuse_amd import weights as wts, scheduler as sch
from amuse_amd.engine import HipEngine
eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0))
eng.set_schedule(sch.ddpm_table(50))
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
gen = torch.Generator().manual_seed(2)
c, e, s = (torch.randn(B, 256, generator=gen).cuda() for _ in range(3))
prec = sys.argv[2] if len(sys.argv) > 2 else "bf16"
st = eng.profile_sample(c, e, s, prec, prof_step=3).astype(np.int64).reshape(8, 96)
names = ["pre(skip)", "P1", "C1", "FFN", "C2"]
names10 = ["pre(skip)", "P1", "C1", "F1a", "F1b", "geluA", "F2a", "geluB", "F2b", "C2"]   # k_sample8x stamps inside its FFN half
for w in range(8):
    v = st[w]; n = int((v != 0).sum()); v = v[:n]
    # stamps: step top | step start (the head - token assembly, wave 4's time-token copy - lies between the two) | 9 blocks x K | tail | the next step's top
    K = 10 if n in (3 + 9 * 10, 4 + 9 * 10) else 5
    assert n in (3 + 9 * K, 4 + 9 * K), n
    nm = names10 if K == 10 else names
    head = int(v[1] - v[0])
    blocks = v[2:2 + 9 * K].reshape(9, K)
    prev = np.concatenate([[v[1]], blocks[:-1, -1]])
    seg = np.diff(np.concatenate([prev[:, None], blocks], axis=1), axis=1)
    end = 2 + 9 * K
    tot = f"{int(v[end + 1] - v[0])} ticks top to top" if n == end + 2 else f"{int(v[end] - v[0])} ticks (head + phases; no next step)"
    print(f"wave {w}: step {tot}; head {head}  sums " + "  ".join(f"{n_} {int(x)}" for n_, x in zip(nm, seg.sum(axis=0))) + f"  tail {int(v[end]-v[end-1])}"
          + (f"  step barrier {int(v[end + 1] - v[end])}" if n == end + 2 else ""))
    if w in (0, 4):
        for b in range(9):
            print("    blk", b, " ".join(f"{int(x):6d}" for x in seg[b]))
        # absolute times of block 2's stamps relative to the block start of wave 0: who waits for whom
    if w in (0, 4):
        print("    blk 2 stamps relative to its first:", " ".join(str(int(x - blocks[2][0])) for x in blocks[2]), " (abs start", int(blocks[2][0] - st[0][2]), ")")
# when each wave leaves the head, relative to the first wave's step top (stamps 0 and 1 of every wave; s_memtime is one counter per XCD)
t0 = min(int(st[w][0]) for w in range(8))
print("head: top / start per wave relative to the earliest top: " + "  ".join(f"w{w} {int(st[w][0]) - t0}/{int(st[w][1]) - t0}" for w in range(8)))
