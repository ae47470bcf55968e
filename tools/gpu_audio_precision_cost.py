"""Cost of the audio front-end's parity mode: amuse_audio_features in bf16 and fp32x, timed ALTERNATELY in one process at 1, 8 and 32 clips with HIP events around
synchronised work, every shape warmed up first, N >= 20 timed calls each.  python tools/gpu_audio_precision_cost.py [--calls 20] [--out profiles/audio_fp32x_cost.txt]
--bf16-only: the bf16 figures alone, never touching the switch - the form that also runs from a checkout without the mode, for the regression check of the
existing path (boxes differ by 1-2 %, so compare runs of ONE job)."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from amuse_amd import audio_weights as aw  # noqa: E402
from amuse_amd.audio import AudioEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bf16-only", action="store_true")
    args = ap.parse_args()
    W = [aw.make_ast_weights(0, n) for n in aw.ENCODERS]
    eng = AudioEngine(*W, "cuda:0")
    modes = ["bf16"] if args.bf16_only else ["bf16", "fp32x"]
    g = torch.Generator().manual_seed(0)
    lines = [f"amuse_audio_features (fbank + 3 x AST, 159,744 samples per clip), {args.calls} timed calls per cell, modes alternating call by call; ms per call (median, min) and per clip"]
    for B in (1, 8, 32):
        w = (0.1 * torch.randn(B, 159744, generator=g)).cuda()
        for m in modes:                       # warm-up: every shape in every mode (workspaces, weight images, code objects)
            if not args.bf16_only:
                eng.set_precision(m)
            for _ in range(2):
                eng.features(w)
        torch.cuda.synchronize()
        ts = {m: [] for m in modes}
        for _ in range(args.calls):
            for m in modes:
                if not args.bf16_only:
                    eng.set_precision(m)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.features(w)
                e1.record()
                torch.cuda.synchronize()
                ts[m].append(e0.elapsed_time(e1))
        for m in modes:
            med, mn = statistics.median(ts[m]), min(ts[m])
            lines.append(f"B {B:2d}  {m:5s}  median {med:9.3f} ms  min {mn:9.3f} ms  per clip {med / B:8.3f} ms")
        if not args.bf16_only:
            lines.append(f"B {B:2d}  fp32x / bf16 = {statistics.median(ts['fp32x']) / statistics.median(ts['bf16']):.2f} x")
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
