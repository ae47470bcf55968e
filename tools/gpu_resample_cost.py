"""Cost of the resampler on the GPU (amuse_amd/resample.py, csrc/k_resample.hip) -> profiles/resample_cost.txt.  HIP events, medians.
  the resampler call alone - int16 mono PCM already in device memory, output preallocated - for a 10 s and a 60 s waveform at 48,000 and 44,100 Hz, beside the
    bytes it has to move, and the same through resample.resample from a host waveform (upload + call)
  beside them, for scale: the audio front-end (fbank + 3 x AST, random-init weights) on the same audio at 16 kHz, cut into the long-form windows, one batch
  with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1` headlines of that tree and this one, alternating, as child processes - run
    before this process opens the GPU.  No code of the default path changed; the figures are there to show it did not move.
usage: python tools/gpu_resample_cost.py [--parent DIR] [--pairs 2] [out file]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

DEV = "cuda:0"
HBM = 8.0e12   # MI355X HBM3E peak, bytes / s (data sheet)
BENCH = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-torch-baseline", "--no-audio"]


def headline(tree: Path) -> float:
    r = subprocess.run([sys.executable] + BENCH, cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed: {r.stderr[-1500:]}")
    return float(json.loads(r.stdout.strip().splitlines()[-1])["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("out", nargs="?", default=str(REPO / "profiles" / "resample_cost.txt"))
    args = ap.parse_args()
    bench_lines = []
    if args.parent:
        vals = []
        for _ in range(args.pairs):
            vals += [("parent", headline(Path(args.parent))), ("this tree", headline(REPO))]
        bench_lines.append("the default path (--resample off): python " + " ".join(BENCH) + ", the parent commit's tree and this tree alternating in one job, frames/s")
        bench_lines.append("  " + "   ".join(f"{k} {v:,.1f}" for k, v in vals) + "      (no code of that path changed)")

    import torch
    from amuse_amd import audio_weights as aw
    from amuse_amd import longform, resample
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1

    def timed(fn, n=1):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in ev])

    fmt = lambda a: f"{np.median(a):8.3f} ({np.min(a):.3f}) ms"
    lines = [f"tools/gpu_resample_cost.py on {torch.cuda.get_device_name(0)}: HIP events, ms median (min)"]
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))
    rng = np.random.default_rng(0)
    for seconds in (10, 60):
        for rate in (48000, 44100):
            n = seconds * rate
            pcm_host = (rng.standard_normal(n) * 3000).astype(np.int16)
            wave_host = torch.from_numpy(pcm_host.astype(np.float32) / 32768.0)[None]
            pcm = torch.from_numpy(pcm_host).to(DEV)
            r = resample.Resampler.get(DEV, rate)
            p = resample.plan(rate, 16000, n)
            out = torch.empty(p["n_out"], device=DEV)
            for _ in range(5):
                r(pcm, out=out)
                resample.resample(wave_host, rate, device=DEV)
            torch.cuda.synchronize()
            t_call = timed(lambda: r(pcm, out=out), 200)
            t_host = timed(lambda: resample.resample(wave_host, rate, device=DEV), 50)
            need = n * 2 + p["n_out"] * 4
            lines.append(f"{seconds:2d} s at {rate} Hz ({n} int16 samples -> {p['n_out']}, {p['taps']} taps x {p['up']} phases): the call alone {fmt(t_call)}; it has to move "
                         f"{need / 1e6:.2f} MB = {need / HBM * 1e6:.2f} us at the HBM peak (launch-bound);   from a host fp32 waveform (upload + call) {fmt(t_host)}")
        # for scale: the front-end on the same audio at 16 kHz, as the long-form windows, one batch
        w16 = r(pcm)[:, :seconds * 16000].cpu()
        a = w16 - w16.mean()
        chunks = [a[:, s:e] for s, e in longform.window_slices(a.shape[1], 270)]
        for prec in ("bf16", "fp32x"):
            m.audio_engine.set_precision(prec)
            for _ in range(2):
                m.process_seq_list(chunks, framerate=16000)
            torch.cuda.synchronize()
            t = np.array([timed(lambda: m.process_seq_list(chunks, framerate=16000))[0] for _ in range(10)])
            lines.append(f"   for scale, the audio front-end on those {seconds} s at 16 kHz ({len(chunks)} window{'s' if len(chunks) > 1 else ''}, one batch, {prec}): {fmt(t)}")
    m.audio_engine.close()
    m.engine.close()
    lines += bench_lines
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
