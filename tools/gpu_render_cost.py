"""Cost of the preview renderer on the GPU (amuse_amd/render.py, csrc/k_render.hip) -> profiles/render_cost.txt.  HIP events, median of 20.
  workload: a 300-frame clip of a body-sized capsule - a UV sphere pulled apart, V = 10,475 / T = 20,908 as SMPL-X has them (9 unused vertices, 20 triangles
    left out), skinned to a 55-joint chain along its axis and posed by the body engine - at 512 x 512, ss 1 and ss 2, through Renderer.render (projection + tile
    kernel, RGB only: what the product runs)
  the same call with the camera 8 x further away (the mesh covers 1 / 64 of the samples): what is left is the full triangle walk of every tile
  the raster stage alone (amuse_debug_render_raster: no shading, but it writes the keys: 8 bytes per sample)
  beside them, for scale: BodyEngine.vertices for the same 300 frames, and the DDIM-50 job (sampler + decode, fp32x) of one clip
usage: python tools/gpu_render_cost.py [out file]"""
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

DEV = "cuda:0"
V_SMPLX, T_SMPLX, F = 10475, 20908, 300


def capsule_model():
    """-> (BodyModel with faces, poses [1, F, 55, 3]): radius 0.22 m, 1.7 m tall, joints spread along the axis, every vertex bound to its two nearest joints"""
    import render_cases as rc
    from amuse_amd import body
    r, stretch = 0.22, 0.63
    v, f = rc.sphere_mesh(n_lat=110, n_lon=96, r=r, stretch=stretch)             # 10,466 vertices, 20,928 triangles
    assert len(v) <= V_SMPLX and len(f) >= T_SMPLX
    v = np.concatenate([v, np.zeros((V_SMPLX - len(v), 3), np.float32)])
    f = f[:T_SMPLX]
    NJ = 55
    jy = np.linspace(-(r + stretch) * 0.95, (r + stretch) * 0.95, NJ)
    parents = np.arange(-1, NJ - 1).astype(np.int32)
    weights = np.zeros((V_SMPLX, NJ), np.float32)
    d = np.abs(v[:, 1:2] - jy[None])
    near = np.argsort(d, axis=1)[:, :2]
    w = 1.0 / (d[np.arange(V_SMPLX)[:, None], near] + 1e-3)
    weights[np.arange(V_SMPLX)[:, None], near] = (w / w.sum(1, keepdims=True)).astype(np.float32)
    J_regressor = np.zeros((NJ, V_SMPLX), np.float32)
    for j in range(NJ):                                                          # a joint = the mean of the ring of vertices nearest its height
        ring = np.argsort(np.abs(v[:len(v) - 9, 1] - jy[j]))[:96]
        J_regressor[j, ring] = 1.0 / 96
    g = np.random.default_rng(0)
    model = body.BodyModel(v, np.zeros((V_SMPLX, 3, 10), np.float32), (g.standard_normal((486, V_SMPLX * 3)) * 1e-4).astype(np.float32), J_regressor, weights, parents, f)
    t = np.arange(F)[None, :, None, None] / 30.0
    phase = g.uniform(0, 2 * np.pi, (1, 1, NJ, 3))
    poses = (0.035 * np.sin(2 * np.pi * 0.5 * t + phase)).astype(np.float32)      # a slow wobble: 55 joints x 0.035 rad bends the capsule, it does not curl up
    return model, poses


def main():
    import torch
    from amuse_amd import body, render
    from amuse_amd import scheduler as sch
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "render_cost.txt"

    def timed(fn, n=20):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in ev])

    fmt = lambda a: f"{np.median(a):9.3f} ({np.min(a):.3f}) ms"
    lines = [f"tools/gpu_render_cost.py on {torch.cuda.get_device_name(0)}: HIP events, 20 calls per cell; ms median (min)",
             f"workload: {F} frames of a posed capsule, V = {V_SMPLX}, T = {T_SMPLX}, 512 x 512, a front camera framed on the clip's joints"]
    model, poses = capsule_model()
    eng = body.BodyEngine(DEV, model)
    eng.set_subjects(np.zeros((1, 10), np.float32))
    rot = torch.from_numpy(poses).to(DEV)
    joints, verts = eng.forward(rot)
    verts = verts[0].contiguous()
    for _ in range(3):
        eng.vertices(rot)
    torch.cuda.synchronize()
    t_vert = timed(lambda: eng.vertices(rot))
    lines.append(f"BodyEngine.vertices, the same {F} frames (fp32x, includes the wrapper's output allocation): {fmt(t_vert)}")
    cam = render.Camera.front(joints.cpu().numpy(), 512, 512)
    far = render.Camera.front(joints.cpu().numpy(), 512, 512, distance=8.0 * float(cam.t[2]))
    t_render = {}
    for ss in (1, 2):
        ren = render.Renderer(DEV, model.faces, model.V, 512, 512, ss)
        p = render.plan(512, 512, ss, model.V, T_SMPLX, F)
        rgb, keys, screen = ren.render(verts, cam, keys=True, screen=True)
        cover = float((keys != -1).float().mean())
        del keys
        for _ in range(2):
            ren.render(verts, cam)
            ren.render(verts, far)
        torch.cuda.synchronize()
        t_render[ss] = timed(lambda: ren.render(verts, cam))
        t_far = timed(lambda: ren.render(verts, far))
        ren.raster(screen)
        torch.cuda.synchronize()
        t_raster = timed(lambda: ren.raster(screen), 10)
        tests = p["tiles_x"] * p["tiles_y"] * T_SMPLX
        lines.append(f"ss {ss}: {p['tiles_x']} x {p['tiles_y']} tiles, {tests / 1e6:.1f} M box tests per frame, chunks of {p['chunk_frames']} frames, workspace "
                     f"{p['workspace_bytes'] / 2 ** 20:.1f} MiB, {cover:.1%} of the samples covered")
        lines.append(f"   Renderer.render, {F} frames -> RGB:                 {fmt(t_render[ss])} = {np.median(t_render[ss]) / F * 1e3:7.1f} us per frame, "
                     f"{np.median(t_render[ss]) / np.median(t_vert):.1f} x the vertices call")
        lines.append(f"   the same, camera 8 x further (the walk alone):      {fmt(t_far)} = {np.median(t_far) / np.median(t_render[ss]):.0%} of the call above")
        lines.append(f"   raster stage alone (keys written, no shading):      {fmt(t_raster)}")
        ren.close()
    eng.close()
    # for scale: the DDIM-50 job of one clip (sampler + decode), as smoke() runs it
    he = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), DEV)
    he.set_schedule(sch.ddim_table())
    gen = torch.Generator().manual_seed(1)
    con, emo, sty, x = (torch.randn(1, n, generator=gen) for n in (256, 256, 256, 128))
    for _ in range(2):
        he.diffusion_backward(con, emo, sty, "fp32x", x_init=x)
    torch.cuda.synchronize()
    t_job = timed(lambda: he.diffusion_backward(con, emo, sty, "fp32x", x_init=x))
    he.close()
    lines.append(f"for scale, the DDIM-50 job of one clip (sampler + decode, fp32x, from host embeddings): {fmt(t_job)}; the preview of its {F} frames at ss 2 is "
                 f"{np.median(t_render[2]) / np.median(t_job):.2f} x that, at ss 1 {np.median(t_render[1]) / np.median(t_job):.2f} x")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
