"""Cost of motion smoothing on the GPU (amuse_amd/smooth.py, csrc/k_smooth.hip) -> profiles/smooth_cost.txt.  HIP events around whole calls of the entry point on
preallocated outputs (no allocation inside the timed window); the four shapes alternate inside one loop, after a warm-up of each.
  256 sequences x 300 frames (a batch of 10 s clips: 8 launches of 32 sequences) and ONE sequence of 108,000 frames (an hour at 30 fps), at windows 9 and 31,
    order 3, all 56 slots filtered, beside the bytes the call has to move (every pose and translation row read once and written once) at the HBM peak
  beside them: the long-form stitch of the same hour (amuse_stitch_windows, 400 windows at hop 270) and the DDIM-50 job of ONE 10 s clip (diffusion_backward,
    fp32x and bf16, random-init weights) - what a motion costs to make, next to what it costs to smooth
Nobody set a target for these: they are recorded.
usage: python tools/gpu_smooth_cost.py [out file]"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amuse_amd import _lib, longform, smooth  # noqa: E402
from amuse_amd import weights as wts  # noqa: E402
from amuse_amd.infer_ldm import PretrainedLPDM_v1  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12   # MI355X HBM3E peak, bytes / s (data sheet)


def timed(fn, n=1):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def fmt(a):
    a = np.asarray(a)
    return f"{np.median(a):9.3f} ({a.min():.3f}) ms"


def smooth_motion(S, L, seed):
    """a smooth random motion, (S L, 55, 3) and (S L, 3): a random walk of small steps (the filter's cost does not depend on the values)"""
    g = torch.Generator().manual_seed(seed)
    p = (0.02 * torch.randn(S, L, 55, 3, generator=g)).cumsum(1) + 0.5 * torch.randn(S, 1, 55, 3, generator=g)
    t = (0.01 * torch.randn(S, L, 3, generator=g)).cumsum(1)
    return p.reshape(S * L, 55, 3).to(DEV), t.reshape(S * L, 3).to(DEV)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "smooth_cost.txt"
    lib = _lib.load()
    lines = [f"tools/gpu_smooth_cost.py on {torch.cuda.get_device_name(0)}: HIP events around whole calls, ms median (min); the shapes alternate in one loop, "
             f"200 repetitions each after 5 warm-up calls"]
    bank = torch.from_numpy(smooth.banks(3)).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    vp = lambda x: C.c_void_p(x.data_ptr())
    calls, info = {}, {}
    for name, (S, L) in {"256 x 300 frames": (256, 300), "1 x 108,000 frames": (1, 108000)}.items():
        p, t = smooth_motion(S, L, S)
        po, to = torch.empty_like(p), torch.empty_like(t)
        fr = (C.c_int * S)(*([L] * S))
        for window in (9, 31):
            hw = (C.c_ubyte * 56)(*smooth.half_windows(window))

            def call(p=p, t=t, po=po, to=to, fr=fr, hw=hw, S=S):
                _lib.check(lib.amuse_smooth_motion(vp(p), vp(t), S, fr, hw, vp(bank), vp(po), vp(to), st))
            calls[(name, window)] = call
            info[(name, window)] = (S, L)
    for call in calls.values():
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(200):
        for k, call in calls.items():
            times[k].append(timed(call)[0])
    for (name, window), ts in times.items():
        S, L = info[(name, window)]
        need = 2 * S * L * 168 * 4
        tiles = S * -(-L // 32)
        lines.append(f"smooth  {name:18s} window {window:2d} order 3: {fmt(ts)} per call ({-(-S // 32)} launch(es), {tiles} workgroups of 32 frames); it has to move "
                     f"{need / 1e6:.1f} MB = {need / HBM * 1e3:.4f} ms at the HBM peak; {np.median(ts) * 1e6 / (S * L * 56):.2f} ns per (frame, slot)")
    # ---- beside them: the stitch of the same hour, and what a clip costs to make
    L, hop, F = 108000, 270, 300
    W = -(-(L - F) // hop) + 1
    g = torch.Generator().manual_seed(0)
    poses, trans = (0.5 * torch.randn(W, F, 55, 3, generator=g)).to(DEV), torch.randn(W, F, 3, generator=g).to(DEV)
    blend = longform.blend_weights(F - hop).to(DEV)
    stitch = lambda: longform.stitch(poses, trans, [W], [L], hop, blend=blend)
    for _ in range(5):
        stitch()
    torch.cuda.synchronize()
    lines.append(f"stitch  1 x 108,000 frames, {W} windows at hop {hop}: {fmt(timed(stitch, 100))} per call through the Python wrapper (allocates its outputs)")
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    gz = torch.Generator().manual_seed(1)
    z = [torch.randn(1, 256, generator=gz).to(DEV) for _ in range(3)]
    for prec in ("fp32x", "bf16"):
        m.precision = prec
        job = lambda: m.diffusion_backward(1, *z, clip_index0=0)
        for _ in range(3):
            job()
        torch.cuda.synchronize()
        lines.append(f"DDIM-50 job, ONE 10 s clip (300 frames), {prec:5s}, random-init weights: {fmt(timed(job, 20))} (sample + decode)")
    m.engine.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
