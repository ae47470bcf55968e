"""Cost of the long-form candidates on the GPU (amuse_amd/seam.py, csrc/k_seam.hip) -> profiles/seam_cost.txt.  HIP events; the variants of a comparison alternate
inside one loop.  Records, not pass bars: the path is new, there is no parent to compare it with.
  amuse_seam_cost / _path / _select alone at F = 300, W = 40 windows (a six-minute WAV), hop 270 with K = 4, 16, 64 and hop 150 with K = 16: workspace and
    outputs allocated once, random rotations
  beside each, the K-fold diffusion_backward of those W K clips (DDIM-50, random embeddings, fp32x and bf16) against the W clips of K = 1: what K costs end to end
  the 25 s test wave (3 windows) on RANDOM-INIT weights at K = 1, 4, 16, 64: the root-mean-square seam angle per weighted joint and overlap row of the chosen
    path against the all-first-candidates path.  Random-init weights say nothing about a trained checkpoint; that measurement is open.
usage: python tools/gpu_seam_cost.py [out file]"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amuse_amd import audio_weights as aw  # noqa: E402
from amuse_amd import longform, seam  # noqa: E402
from amuse_amd import weights as wts  # noqa: E402
from amuse_amd.infer_ldm import PretrainedLPDM_v1  # noqa: E402

DEV = "cuda:0"


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
    return (0.2 * torch.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 0.3 * t)) + 0.05 * torch.randn(n, generator=g) + 0.01)[None]


def kernels(lines, W, hop, K, F=300):
    L = (W - 1) * hop + F
    g = torch.Generator(device=DEV).manual_seed(K + hop)
    poses = 0.5 * torch.randn(W * K, F, 55, 3, generator=g, device=DEV)
    trans = torch.randn(W * K, F, 3, generator=g, device=DEV)
    u, w, tw = seam.default_weights(F - hop)
    u, w = u.to(DEV), w.to(DEV)
    pl = seam.plan([W], K, hop, F)
    ws = torch.empty(pl["workspace_bytes"], device=DEV, dtype=torch.uint8)
    m = torch.empty(pl["seams"], K, K, device=DEV, dtype=torch.float64)
    po, to = torch.empty(W, F, 55, 3, device=DEV), torch.empty(W, F, 3, device=DEV)
    cost = lambda: seam.cost(poses, trans, [W], [L], K, hop, F, u, w, tw, workspace=ws, out=m)
    cost()
    choice, _ = seam.path(m, [W], K)
    path = lambda: seam.path(m, [W], K)
    select = lambda: seam.select(poses, trans, choice, poses_out=po, trans_out=to)
    for _ in range(3):
        cost(), path(), select()
    torch.cuda.synchronize()
    tc, tp, ts = [], [], []
    for _ in range(20):      # the three alternate in one loop
        tc.append(timed(cost)[0]), tp.append(timed(path)[0]), ts.append(timed(select)[0])
    lines.append(f"  hop {hop}, K = {K:2d}: {pl['seams']} seams x {K * K} pairs x {F - hop} rows; workspace {pl['workspace_bytes'] / 2 ** 20:.1f} MiB   "
                 f"cost {fmt(tc)}   path {fmt(tp)}   select {fmt(ts)}")
    del poses, trans, ws


def sampler(lines, model, W, Ks):
    g = torch.Generator().manual_seed(3)
    emb = [torch.randn(W, 256, generator=g).to(DEV) for _ in range(3)]
    for prec in ("fp32x", "bf16"):
        model.precision = prec
        run = {K: (lambda K=K: model.diffusion_backward(W * K, *(e.repeat_interleave(K, dim=0) for e in emb), clip_index0=0)) for K in Ks}
        for K in Ks:
            run[K]()
        torch.cuda.synchronize()
        t = {K: [] for K in Ks}
        for _ in range(5):       # the clip counts alternate in one loop
            for K in Ks:
                t[K].append(timed(run[K])[0])
        base = np.median(t[Ks[0]])
        lines.append(f"  {prec:5s} diffusion_backward, DDIM-50, {W} windows: " + "   ".join(f"K = {K} ({W * K} clips) {fmt(t[K])} = {np.median(t[K]) / base:.2f} x" for K in Ks))


def seams_of_the_test_wave(lines, model):
    model.precision = "fp32x"
    w = wave(400000, 1)
    a = w - w.mean()
    chunks = [a[:, s:e] for s, e in longform.window_slices(400000, 270)]
    embs = model.process_seq_list(chunks, framerate=16000)
    u, jw, _ = seam.default_weights(30)
    norm = float(u.sum() * jw.sum()) * 2          # two seams, 30 rows each, 47 weighted joints
    lines.append("the 25 s test wave (3 windows, hop 270, fp32x, DDIM-50) on RANDOM-INIT weights, clip indices from 0: root-mean-square seam angle per weighted joint "
                 "and overlap row, rad - sqrt(total cost / (2 seams x 30 rows x 47 joints))")
    for K in (1, 4, 16, 64):
        con, emo, sty = (torch.cat([e[i] for e in embs]).repeat_interleave(K, dim=0) for i in range(3))
        o = model.diffusion_backward(3 * K, con, emo, sty, clip_index0=0)
        _, _, info = seam.best_windows(o["poses"], o["trans"], [3], [750], K, 270)
        r = seam.report(info, [3], K)[0]
        lines.append(f"  K = {K:2d}: all-first-candidates path {np.sqrt(r['total_first'] / norm):.4f}   chosen path {np.sqrt(r['total'] / norm):.4f}   (choice {r['choice']})")
    lines.append("  random-init weights say NOTHING about a trained checkpoint: its candidates may differ far less (or more) where windows meet.  Whether the choice "
                 "matters on trained weights has not been measured; that measurement is open.")


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "seam_cost.txt"
    lines = [f"tools/gpu_seam_cost.py on {torch.cuda.get_device_name(0)}: HIP events, ms median (min); compared variants alternate in one loop.  Records, not pass bars."]
    W = 40
    lines.append(f"the three calls through the Python wrappers, F = 300, one sequence of W = {W} windows, 20 repetitions per cell")
    for hop, K in ((270, 4), (270, 16), (270, 64), (150, 16)):
        kernels(lines, W, hop, K)
        torch.cuda.empty_cache()
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))
    lines.append("what K costs end to end: the K-fold sampling beside it (random embeddings, 5 repetitions per cell)")
    sampler(lines, m, W, (1, 4, 16, 64))
    seams_of_the_test_wave(lines, m)
    m.audio_engine.close()
    m.engine.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
