"""Cost of the preview video on the GPU (amuse_amd/video.py, csrc/k_mjpeg.hip) -> profiles/preview_video_cost.txt.  HIP events, medians, the variants
alternating in ONE loop (render, transform, whole encode, one after the other in every round), so that clock and cache state are shared between them.
  workload: the rendered frames of tools/gpu_render_cost.py's capsule (V = 10,475, T = 20,908, 512 x 512, ss 2), 300 frames (a 10 s clip) and the same frames
    six times over (1,800: a one-minute long-form clip), quality 90
  per size: Renderer.render of the frames; the transform alone (amuse_debug_mjpeg_coefficients); the whole encode (transform + size + scans + write, one
    amuse_mjpeg_encode into a buffer of the raw RGB size) - the entropy passes are the difference; the bytes per frame; the host's share: the copy of the files
    to the host and AviWriter writing them with 16 kHz mono PCM (wall clock)
  optionally, appended: the bench.py headline of two trees alternating (tools/gpu_video_cost.py --bench OTHER_TREE [rounds]): this tree and a checkout of the
    parent commit built beside it - the default path must not move
usage: python tools/gpu_video_cost.py [out file] [--bench OTHER_TREE [rounds]]"""
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tools"))

DEV = "cuda:0"
ROUNDS = 11


def bench_ab(other: Path, rounds: int):
    """the headline of bench.py, this tree and `other` alternating; -> lines"""
    rows = {"this tree": [], "parent tree": []}
    bench_args = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-audio", "--no-torch-baseline"]
    for _ in range(rounds):
        for name, tree in (("parent tree", other), ("this tree", REPO)):
            r = subprocess.run([sys.executable, "bench.py"] + bench_args,
                               cwd=tree, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
            rows[name].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    key = next(k for k in ("value", "clips_per_s", "throughput") if k in rows["this tree"][0])
    lines = [f"bench.py {' '.join(bench_args)} (headline '{rows['this tree'][0].get('metric', key)}', key '{key}'), {rounds} rounds, the two trees alternating:"]
    for name, rs in rows.items():
        v = np.array([float(r[key]) for r in rs])
        lines.append(f"   {name:12s} median {np.median(v):.4f}  (min {v.min():.4f}, max {v.max():.4f})  {[round(float(x), 4) for x in v]}")
    a, b = (np.median([float(r[key]) for r in rows[n]]) for n in ("this tree", "parent tree"))
    lines.append(f"   this tree / parent tree = {a / b:.4f}")
    return lines


def main():
    import torch
    import gpu_render_cost as grc
    from amuse_amd import body, render, video
    args = sys.argv[1:]
    bench = None
    if "--bench" in args:
        i = args.index("--bench")
        bench = (Path(args[i + 1]), int(args[i + 2]) if len(args) > i + 2 else 3)
        args = args[:i]
    out_path = Path(args[0]) if args else REPO / "profiles" / "preview_video_cost.txt"
    med = lambda a: f"{np.median(a):9.3f} ({np.min(a):.3f}) ms"
    lines = [f"tools/gpu_video_cost.py on {torch.cuda.get_device_name(0)}: HIP events, {ROUNDS} rounds, render / transform / encode alternating in one loop; ms median (min)",
             "workload: the rendered frames of a posed capsule (V = 10475, T = 20908, 512 x 512, ss 2: tools/gpu_render_cost.py), quality 90, no chroma subsampling"]
    model, poses = grc.capsule_model()
    eng = body.BodyEngine(DEV, model)
    eng.set_subjects(np.zeros((1, 10), np.float32))
    rot = torch.from_numpy(poses).to(DEV)
    joints, verts = eng.forward(rot)
    cam = render.Camera.front(joints.cpu().numpy(), 512, 512)
    ren = render.Renderer(DEV, model.faces, model.V, 512, 512, 2)
    enc = video.JpegEncoder(DEV, 512, 512, 90)
    pcm = (np.random.default_rng(0).standard_normal((16000 * 60, 1)) * 3000).astype(np.int16)
    for reps in (1, 6):
        v = verts[0].repeat(reps, 1, 1).contiguous()
        F = int(v.shape[0])
        rgb = ren.render(v, cam)
        out = torch.empty(rgb.numel(), dtype=torch.uint8, device=DEV)
        enc.reserve(F)
        for _ in range(2):
            ren.render(v, cam)
            enc.coefficients(rgb)
            enc.encode_into(rgb, out)
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(ROUNDS)]
        for e in ev:
            e[0].record()
            ren.render(v, cam)
            e[1].record()
            enc.coefficients(rgb)
            e[2].record()
            offsets, sizes, total = enc.encode_into(rgb, out)
            e[3].record()
        torch.cuda.synchronize()
        t_render, t_transform, t_encode = (np.array([e[i].elapsed_time(e[i + 1]) for e in ev]) for i in range(3))
        t_entropy = t_encode - t_transform
        n = int(total.item())
        assert n <= out.numel()
        host = []
        for _ in range(3):
            with tempfile.TemporaryDirectory() as d:
                t0 = time.perf_counter()
                data = out[:n].cpu().numpy().tobytes()
                off, sz = offsets.cpu().tolist(), sizes.cpu().tolist()
                t1 = time.perf_counter()
                with video.AviWriter(Path(d) / "v.avi", 512, 512, 30, (pcm[:F * 16000 // 30], 16000)) as w:
                    for o, s in zip(off, sz):
                        w.write_frame(data[o:o + s])
                t2 = time.perf_counter()
                host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        host = np.array(host)
        lines += [f"{F} frames ({F / 30:.0f} s):",
                  f"   Renderer.render -> RGB:                              {med(t_render)} = {np.median(t_render) / F * 1e3:7.1f} us per frame",
                  f"   transform (colour, DCT, quantisation) alone:         {med(t_transform)}",
                  f"   whole encode (transform, size, scans, write):        {med(t_encode)} = {np.median(t_encode) / F * 1e3:7.1f} us per frame, "
                  f"{np.median(t_encode) / np.median(t_render):.2f} x the render",
                  f"   entropy passes (encode - transform, per round):      {med(t_entropy)} = {np.median(t_entropy) / np.median(t_render):.2f} x the render",
                  f"   files: {n / F:9.0f} bytes per frame ({n / 2 ** 20:.1f} MiB in all, {n / rgb.numel():.1%} of the raw RGB); encoder workspace "
                  f"{video.plan(512, 512, F)['workspace_bytes'] / 2 ** 20:.0f} MiB",
                  f"   host: files to the host {np.median(host[:, 0]):.1f} ms, AviWriter with 16 kHz PCM to a temporary file {np.median(host[:, 1]):.1f} ms (wall clock, median of 3)"]
        del v, rgb, out
    enc.close()
    ren.close()
    eng.close()
    if bench is not None:
        lines += bench_ab(*bench)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
