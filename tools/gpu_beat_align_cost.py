"""GPU: the cost of the beat-alignment calls (amuse_beat_onsets / _pick / _align) beside amuse_audio_fbank on the same 256 waveforms of 10 s, and on one clip of 120 s: HIP events
around 20 calls, 3 warm-up calls, the median (min, max) of 7 such windows -> profiles/beat_align_cost.txt.

  python tools/gpu_beat_align_cost.py fbank|beat OUT.txt [package root]

`fbank` times amuse_audio_fbank alone; a package root other than this tree (a checkout of the parent commit with its library built) times that build's kernel.  Run the two modes as
separate processes, alternating, and more than once: the spread between passes is part of the result."""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
mode, out_path = sys.argv[1], sys.argv[2]
sys.path.insert(0, sys.argv[3] if len(sys.argv) > 3 else str(REPO))      # the package root: the tree, or the parent commit's copy
DEV = "cuda:0"
out = open(out_path, "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def timed(fn, iters, windows=7, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


g = torch.Generator().manual_seed(0)
t = torch.arange(160000, dtype=torch.float32) / 16000.0
waves = (0.2 * torch.sin(2 * np.pi * 220.0 * t)[None] * (1 + 0.5 * torch.sin(2 * np.pi * 3.0 * t))[None] + 0.05 * torch.randn(256, 160000, generator=g)).to(DEV).contiguous()
from amuse_amd import _lib
say("library", _lib.LIB_PATH, "mode", mode, "device", torch.cuda.get_device_name(0))
if mode == "fbank":
    from amuse_amd import audio, audio_weights as aw
    eng = audio.AudioEngine(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS), device=DEV)
    m = timed(lambda: eng.fbank(waves), 20)
    say(f"amuse_audio_fbank 256 x 10 s (998 frames + 26 pad rows each): median {m[0]:.4f} ms  min {m[1]:.4f}  max {m[2]:.4f}  (7 windows of 20 calls)")
    eng.close()
else:
    from amuse_amd import beat_align as ba
    be = ba.BeatEngine(DEV)
    m = timed(lambda: be.onsets(waves), 20)
    say(f"amuse_beat_onsets 256 x 10 s (998 frames each; envelope + pick): median {m[0]:.4f} ms  min {m[1]:.4f}  max {m[2]:.4f}  (7 windows of 20 calls)")
    env, mask = be.onsets(waves)
    fr = torch.full((256,), 998, dtype=torch.int32, device=DEV)
    m = timed(lambda: be.pick(env, fr), 20)
    say(f"amuse_beat_pick alone 256 x 998 frames: median {m[0]:.4f} ms  min {m[1]:.4f}  max {m[2]:.4f}")
    J = (torch.cumsum(torch.randn(256, 300, 55, 3, generator=g) * 0.01, 1)).to(DEV).contiguous()
    m = timed(lambda: be.align_rows(mask, fr, J), 20)
    say(f"amuse_beat_align 256 clips x 300 frames, T 998: median {m[0]:.4f} ms  min {m[1]:.4f}  max {m[2]:.4f}")
    say("onsets per clip (mean):", float(mask.sum()) / 256)
    long = (0.05 * torch.randn(1, 1920000, generator=g)).to(DEV)
    k = torch.arange(1920000, device=DEV)
    long = long * (1.0 + 8.0 * ((k % 8000) < 1600))[None]            # a burst every half second
    m = timed(lambda: be.onsets(long), 20)
    say(f"amuse_beat_onsets 1 x 120 s (11998 frames): median {m[0]:.4f} ms  min {m[1]:.4f}  max {m[2]:.4f}")
    env1, mask1 = be.onsets(long)
    J1 = (torch.cumsum(torch.randn(1, 3600, 55, 3, generator=g) * 0.01, 1)).to(DEV).contiguous()
    f1 = torch.tensor([11998], dtype=torch.int32, device=DEV)
    m = timed(lambda: be.align_rows(mask1, f1, J1), 20)
    say(f"amuse_beat_align 1 clip x 3600 frames, T 11998 ({int(mask1.sum())} onsets): median {m[0]:.4f} ms  min {m[1]:.4f}  max {m[2]:.4f}")
    be.close()
out.close()
