"""Cost of long-form inference on the GPU (amuse_amd/longform.py, csrc/k_stitch.hip) -> profiles/longform_cost.txt.  HIP events; the variants of a comparison
alternate inside one loop.
  the stitch call alone at S = 1, L = 9,000 frames (five minutes of motion, 34 windows at hop 270), beside the bytes it has to move
  a 60 s waveform (7 windows at hop 270, 1,800 frames) end to end, DDIM-50, split into front-end / sample + decode / stitch, sampler and front-end in fp32x and
    in bf16 - and the same seven windows as seven separate 10 s calls (process_single_seq + diffusion_backward of one clip: the path without long-form)
  the largest per-joint angular step between consecutive frames: at seams with hop 300 (no crossfade), across the crossfades with hop 270, and inside windows.
    RANDOM-INIT WEIGHTS: indicative only - a trained model's windows are smoother inside and no closer to each other at the seams.
usage: python tools/gpu_longform_cost.py [out file]"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import stitch_ref as sr  # noqa: E402
from amuse_amd import audio_weights as aw  # noqa: E402
from amuse_amd import longform  # noqa: E402
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


def wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    return (0.2 * torch.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 0.3 * t)) + 0.05 * torch.randn(n, generator=g))[None]


def steps(poses):
    """largest per-joint geodesic angle between consecutive frames, per frame pair: (L, 55, 3) -> (L - 1,)"""
    p = poses.detach().cpu().numpy().astype(np.float64)
    return sr.geodesic(p[:-1], p[1:]).max(-1)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "longform_cost.txt"
    lines = [f"tools/gpu_longform_cost.py on {torch.cuda.get_device_name(0)}: HIP events, ms median (min); compared variants alternate in one loop"]
    # ---- the stitch alone
    L, hop, F = 9000, 270, 300
    W = -(-(L - F) // hop) + 1
    g = torch.Generator().manual_seed(0)
    poses, trans = (0.5 * torch.randn(W, F, 55, 3, generator=g)).to(DEV), torch.randn(W, F, 3, generator=g).to(DEV)
    blend = longform.blend_weights(F - hop).to(DEV)
    call = lambda: longform.stitch(poses, trans, [W], [L], hop, blend=blend)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t = timed(call, 200)
    blended = (W - 1) * (F - hop)
    need = (L + blended) * 168 * 4 + L * 168 * 4
    lines.append(f"stitch alone  S = 1, L = {L} frames, {W} windows at hop {hop} ({blended} blended frames): {fmt(t)} per call through the Python wrapper (allocates its "
                 f"outputs); it has to move {need / 1e6:.2f} MB = {need / HBM * 1e6:.2f} us at the HBM peak: the call is launch-bound, not bandwidth-bound")
    # ---- 60 s end to end
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))
    w60 = wave(960000, 1)
    a = w60 - w60.mean()
    chunks = [a[:, s:e] for s, e in longform.window_slices(960000, 270)]
    p = longform.plan(960000, 270)
    lines.append(f"60 s waveform: {p['windows']} windows at hop 270, {p['frames']} frames; DDIM-50, random-init weights; 10 repetitions per cell")
    keep = {}
    for prec in ("fp32x", "bf16"):
        m.precision = prec
        m.audio_engine.set_precision(prec)
        cat = lambda embs, k: torch.cat([e[k] for e in embs])

        def long_form(parts):
            parts["front"].append(timed(lambda: keep.__setitem__("e", m.process_seq_list(chunks, framerate=16000)))[0])
            e = keep["e"]
            parts["sample"].append(timed(lambda: keep.__setitem__("o", m.diffusion_backward(len(chunks), cat(e, 0), cat(e, 1), cat(e, 2), clip_index0=0)))[0])
            o = keep["o"]
            parts["stitch"].append(timed(lambda: keep.__setitem__("s", longform.stitch(o["poses"], o["trans"], [p["windows"]], [p["frames"]], 270)))[0])

        def separate(parts):
            def run():
                for k, c in enumerate(chunks):
                    e = m.process_single_seq(c, framerate=16000)
                    m.diffusion_backward(1, *e, clip_index0=k)
            parts["all"].append(timed(run)[0])
        lf, sep = {"front": [], "sample": [], "stitch": []}, {"all": []}
        for _ in range(2):       # warm-up of every shape both variants use
            long_form({"front": [], "sample": [], "stitch": []})
            separate({"all": []})
        for _ in range(10):
            long_form(lf)
            separate(sep)
        tot = np.array(lf["front"]) + np.array(lf["sample"]) + np.array(lf["stitch"])
        lines.append(f"  {prec:5s} long-form, one batch: front-end {fmt(lf['front'])}   sample + decode {fmt(lf['sample'])}   stitch {fmt(lf['stitch'])}   total {fmt(tot)}")
        lines.append(f"  {prec:5s} the same {len(chunks)} windows as {len(chunks)} separate 10 s calls (front-end + sample + decode each): {fmt(sep['all'])}   "
                     f"= {np.median(sep['all']) / np.median(tot):.2f} x the long-form total")
    # ---- seams (fp32x)
    m.precision = "fp32x"
    m.audio_engine.set_precision("fp32x")
    m._clip_counter = 0
    o270 = m.infer_long([w60], hop_frames=270)[0]["poses"]
    m._clip_counter = 0
    o300 = m.infer_long([w60], hop_frames=300)[0]["poses"]
    s270, s300 = steps(o270), steps(o300)
    W300 = longform.plan(960000, 300)["windows"]
    seam300 = np.array([s300[k * 300 - 1] for k in range(1, W300)])                                   # frame k 300 - 1 -> k 300: two windows meet, no crossfade
    inside300 = np.delete(s300, [k * 300 - 1 for k in range(1, W300)])
    fade = np.concatenate([s270[k * 270 - 1:k * 270 + 30] for k in range(1, p["windows"])])          # every pair that touches a blended frame
    inside270 = np.delete(s270, np.concatenate([np.arange(k * 270 - 1, k * 270 + 30) for k in range(1, p["windows"])]))
    lines.append("largest per-joint angular step between consecutive frames, rad (fp32x, RANDOM-INIT weights: indicative only)")
    lines.append(f"  hop 300, at the {seam300.size} seams (no crossfade): max {seam300.max():.4f}  median {np.median(seam300):.4f};   inside windows: max {inside300.max():.4f}  "
                 f"median {np.median(inside300):.4f}")
    lines.append(f"  hop 270, across the {p['windows'] - 1} crossfades ({fade.size} frame pairs): max {fade.max():.4f}  median {np.median(fade):.4f};   inside windows: max "
                 f"{inside270.max():.4f}  median {np.median(inside270):.4f}")
    m.audio_engine.close()
    m.engine.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
