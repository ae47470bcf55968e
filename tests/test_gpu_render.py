"""GPU: the preview renderer (csrc/k_render.hip through amuse_amd/render.py) against tests/render_ref.py's numpy restatement.

Bars, and where they come from.
  raster      the winning key of EVERY sample equals the int64 restatement's: coverage and depth are integer arithmetic on the snapped vertices, so there is nothing
              to tolerate and nothing to exclude.
  projection  X, Y, Zq within 1 unit of the float64 restatement and at most 1 % of the records different at all: X / Y are one fp32 rounding chain away from
              a round-to-nearest, Zq is computed in double.  tests/test_render_cases_cpu.py holds the float32 restatement to the same two conditions.
  shading     every channel within 1 level of the float64 shading of the GPU's OWN keys and vertices: one floor() of an fp32 value whose error is ~1e-5 levels.
  end to end  at most 0.5 % of the pixels differ by more than 1 level from the all-float64 restatement (body model included): a pixel can differ only where a
              snapped coordinate or a quantised depth moved."""
import functools
import os
import struct
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import render_cases as rc
import render_ref as rr

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _raster_cases(shape):
    W, H, ss = rc.SHAPES[shape]
    cases = dict(rc.crafted(W * ss, H * ss))
    cases["fuzz"] = rc.fuzz(W * ss, H * ss, seed=W + ss)
    return cases


@pytest.mark.parametrize("shape", list(rc.SHAPES))
@pytest.mark.parametrize("case", ["fuzz", "shared_edge_quad", "on_centres", "degenerate", "coincident", "interpenetrating", "invalid_vertex", "clipped", "guard_band_span"])
def test_raster_keys_are_the_restatements(shape, case):
    from amuse_amd import render
    W, H, ss = rc.SHAPES[shape]
    rec, faces = _raster_cases(shape)[case]
    ren = render.Renderer(DEV, faces, rec.shape[1], W, H, ss)
    got = _u64(ren.raster(torch.from_numpy(rec).to(DEV)))
    ren.close()
    assert got.shape == (rec.shape[0], H * ss, W * ss)
    covered = 0
    for m in range(rec.shape[0]):
        want = rr.raster(rec[m], faces, W * ss, H * ss)
        covered += int((want != rr.EMPTY).sum())
        bad = got[m] != want
        assert not bad.any(), (shape, case, m, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    print(f"{shape} {case}: {covered} covered samples, all keys equal")
    if case == "degenerate":
        tri, _ = rr.winners(got[0])
        assert not np.isin(tri, (0, 1, 3)).any()                             # zero area and the triangle that misses its sample's centre: never a winner
    elif case == "coincident":
        tri, _ = rr.winners(got[0])
        assert set(np.unique(tri)) == {-1, 0}
    elif case == "invalid_vertex":
        tri, _ = rr.winners(got[0])
        assert set(np.unique(tri)) == {-1, 3}
    elif case == "interpenetrating":
        tri, _ = rr.winners(got[0])
        assert {0, 1} <= set(np.unique(tri))
    elif case in ("clipped", "guard_band_span"):
        assert covered > 0.25 * W * ss * H * ss
    elif case == "fuzz":
        assert covered > 0.5 * rec.shape[0] * W * ss * H * ss


def test_chunking_and_frame_independence():
    """M = chunk_frames + 1 frames in one call: every frame is the frame rendered alone (7 distinct frames, repeated)"""
    from amuse_amd import render
    V, T, W, H = 30, 40, 32, 32
    rng = np.random.default_rng(5)
    faces = rc.random_faces(V, T, seed=6)
    chunk = render.plan(W, H, 1, V, T, 100000)["chunk_frames"]
    assert chunk == 256
    M = chunk + 1
    base = rng.uniform(-1.0, 1.0, (7, V, 3)).astype(np.float32)
    verts = torch.from_numpy(base[np.arange(M) % 7]).to(DEV)
    cam = render.Camera(np.diag([1.0, 1.0, -1.0]), [0.0, 0.0, 4.0], 64.0, 64.0, 16.0, 16.0, 2.0, 6.0)    # (the cloud of +-1 m fills the 32 x 32 image)
    ren = render.Renderer(DEV, faces, V, W, H, 1)
    rgb, keys, screen = ren.render(verts, cam, keys=True, screen=True)
    alone = [ren.render(torch.from_numpy(base[i:i + 1]).to(DEV), cam, keys=True, screen=True) for i in range(7)]
    plain = ren.render(verts, cam)                                           # without the optional outputs: the records live in the workspace
    torch.cuda.synchronize()
    assert torch.equal(plain, rgb)
    for m in range(M):
        a = alone[m % 7]
        assert torch.equal(rgb[m], a[0][0]) and torch.equal(keys[m], a[1][0]) and torch.equal(screen[m], a[2][0]), m
    assert len({bytes(a[0].cpu().numpy().tobytes()) for a in alone}) == 7    # the seven frames do differ
    assert (keys[0] != -1).float().mean() > 0.3
    ren.close()


@functools.lru_cache(maxsize=None)
def _body(ss):
    """the shared V = 203 case on the GPU: vertices from BodyEngine, rendered once with every output"""
    from amuse_amd import body, render
    c = rc.body_case()
    eng = body.BodyEngine(DEV, c["model"])
    eng.set_subjects(c["betas"])
    v = eng.vertices(torch.from_numpy(c["aa"]).to(DEV), torch.from_numpy(c["trans"]).to(DEV))[0].contiguous()
    ren = render.Renderer(DEV, c["faces"], 203, c["width"], c["height"], ss)
    rgb, keys, screen = ren.render(v, c["cam"], keys=True, screen=True)
    again = ren.render(v, c["cam"], keys=True, screen=True)
    torch.cuda.synchronize()
    out = dict(c, v_gpu=v.cpu().numpy(), rgb=rgb.cpu().numpy(), keys=_u64(keys), screen=screen.cpu().numpy(),
               again=(again[0].cpu().numpy(), _u64(again[1]), again[2].cpu().numpy()))
    ren.close()
    eng.close()
    return out


@pytest.mark.parametrize("ss", [1, 2])
def test_projection_against_float64(ss):
    b = _body(ss)
    want, _ = rr.project(b["v_gpu"], b["cam"], ss)
    d = np.abs(b["screen"].astype(np.int64) - want)
    share = float((d.max(-1) > 0).mean())
    print(f"ss {ss}: records {d.shape[0] * d.shape[1]}, worst difference {int(d.max())} unit (bar 1), share that differ {share:.4%} (bar 1 %)")
    assert (want[..., 2] >= 0).mean() > 0.9
    assert d.max() <= 1 and share <= 0.01


@pytest.mark.parametrize("ss", [1, 2])
def test_shading_of_the_gpus_own_keys(ss):
    b = _body(ss)
    _, view = rr.project(b["v_gpu"], b["cam"], ss)
    worst = 0
    for f in range(3):
        want = rr.shade(b["keys"][f], view[f], b["faces"], ss)
        worst = max(worst, int(np.abs(want.astype(np.int64) - b["rgb"][f]).max()))
        assert (b["keys"][f] != rr.EMPTY).mean() > 0.2 and (b["keys"][f] == rr.EMPTY).any()
    print(f"ss {ss}: worst channel difference {worst} level (bar 1)")
    assert worst <= 1
    lit = b["rgb"][(b["rgb"] != np.array(rr.DEFAULT_SHADING["bg_rgb"])).any(-1)]
    assert len(np.unique(lit[:, 0])) > 10                                    # many facets, many levels


def test_shading_parameters():
    """another light, ambient and colours through amuse_shading; ambient 1 paints the body colour flat"""
    from amuse_amd import render
    v, f = rc.sphere_mesh(n_lat=9, n_lon=12)
    cam = render.Camera(np.diag([1.0, 1.0, -1.0]), [0.0, 0.0, 6.0], 150.0, 150.0, 24.0, 24.0, 4.0, 8.0)
    ren = render.Renderer(DEV, f, len(v), 48, 48, 1)
    vd = torch.from_numpy(v[None]).to(DEV)
    sh = dict(light=(1.0, 2.0, -2.0), ambient=0.1, body_rgb=(250, 120, 30), bg_rgb=(0, 255, 7))
    rgb, keys = ren.render(vd, cam, render.Shading(**sh), keys=True)
    want = rr.shade(_u64(keys)[0], rr.project(v, cam, 1)[1], f, 1, sh)
    assert np.abs(want.astype(np.int64) - rgb[0].cpu().numpy()).max() <= 1
    flat = ren.render(vd, cam, render.Shading(ambient=1.0, body_rgb=(9, 99, 199), bg_rgb=(1, 2, 3)))[0].cpu().numpy()
    assert set(map(tuple, flat.reshape(-1, 3).tolist())) == {(9, 99, 199), (1, 2, 3)}
    ren.close()


@pytest.mark.parametrize("ss", [1, 2])
def test_end_to_end_against_the_float64_restatement(ss):
    b = _body(ss)
    bad = total = 0
    for f in range(3):
        want, _, _ = rr.render(b["v64"][f], b["faces"], b["cam"], b["width"], b["height"], ss)
        bad += int((np.abs(want.astype(np.int64) - b["rgb"][f]).max(-1) > 1).sum())
        total += want.shape[0] * want.shape[1]
    print(f"ss {ss}: {bad} of {total} pixels differ by more than 1 level ({bad / total:.3%}, cap 0.5 %)")
    assert bad <= 0.005 * total


@pytest.mark.parametrize("ss", [1, 2])
def test_two_calls_give_equal_bytes(ss):
    b = _body(ss)
    assert np.array_equal(b["rgb"], b["again"][0]) and np.array_equal(b["keys"], b["again"][1]) and np.array_equal(b["screen"], b["again"][2])


def test_sphere_known_answers_on_the_gpu():
    from amuse_amd import render
    W = H = 64
    r, d = 1.0, 12.0
    v, f = rc.sphere_mesh(r=r)
    cam = render.Camera(np.diag([1.0, 1.0, -1.0]), [0.0, 0.0, d], 4.0 * W, 4.0 * W, W / 2, H / 2, d - 2.0, d + 2.0)
    for ss in (1, 2):
        ren = render.Renderer(DEV, f, len(v), W, H, ss)
        rgb, keys = ren.render(torch.from_numpy(v[None]).to(DEV), cam, keys=True)
        rgb, keys = rgb[0].cpu().numpy(), _u64(keys)[0]
        ren.close()
        covered = int((keys != rr.EMPTY).sum())
        want = np.pi * (cam.fx * ss * r) ** 2 / (d * d - r * r)
        print(f"ss {ss}: silhouette {covered} samples, pi r^2 = {want:.1f} ({covered / want - 1:+.3%}, bar 2 %)")
        assert abs(covered / want - 1) <= 0.02
        lum = rgb.astype(np.int64).sum(-1)
        assert lum[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].max() == lum.max() and lum.max() > lum[0, 0]
        assert abs(int(rgb[H // 2, W // 2, 0]) - 200) <= 1 and (rgb[0, 0] == np.array(rr.DEFAULT_SHADING["bg_rgb"])).all()


# ------------------------------------------------------------------ the command lines
def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, colour = struct.unpack(">IIBB", data[16:26])
    assert (depth, colour) == (8, 2)
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT"
    return np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)


def _run_cli(root, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "AMUSE_RUN_STAMP")}
    env.update(AMUSE_RUN_STAMP="20260101-000000")
    r = subprocess.run([sys.executable, "-m", "amuse_amd.main", "--fn", "infer_gesture", "--root", str(root), "--random-init"] + extra,
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return sorted((root / "viz_dump/test/gesture").rglob("*.npz"))


def test_cli_preview_writes_sheets_and_leaves_the_npz_bytes(tmp_path):
    import body_cases as bc
    from conftest import make_reference_tree
    from amuse_amd import body
    models = tmp_path / "models"
    models.mkdir()
    m = body.BodyModel.from_dict(dict(bc.make_model(V=203), faces=rc.random_faces(203, 400)))
    for name in body.SMPLX_FILES.values():
        m.to_npz(models / name)
    plain = _run_cli(make_reference_tree(tmp_path / "a", n_infer_wavs=1), [])
    root = make_reference_tree(tmp_path / "b", n_infer_wavs=1)
    files = _run_cli(root, ["--preview", "--preview-frames", "--smplx-models", str(models), "--preview-size", "64", "--preview-stride", "10"])
    assert len(files) == len(plain) >= 1
    for p, q in zip(plain, files):
        assert p.name == q.name and p.read_bytes() == q.read_bytes()         # the NPZ keeps its bytes
        F = int(np.load(q)["poses"].shape[0])
        sheet = q.with_name(q.name.replace("_motion_smplx.npz", "_preview.png"))
        img = _decode_png(sheet.read_bytes())
        n = -(-F // 10)
        assert img.shape == (-(-n // 6) * 64, 6 * 64, 3)
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 10                # a picture, not a flat field
        frames = sorted(q.with_name(q.name.replace("_motion_smplx.npz", "_preview")).glob("frame_*.png"))
        assert len(frames) == F and frames[0].name == "frame_0000.png" and frames[-1].name == f"frame_{F - 1:04d}.png"
        assert np.array_equal(_decode_png(frames[0].read_bytes()), img[:64, :64]) and np.array_equal(_decode_png(frames[10].read_bytes()), img[:64, 64:128])
    assert not list((tmp_path / "a").rglob("*.png"))                         # off by default: no picture without the switch
    # the stand-alone command on that NPZ: the same sheet, byte for byte
    out = tmp_path / "again"
    r = subprocess.run([sys.executable, "-m", "amuse_amd.render", str(files[0]), "--smplx-models", str(models), "--size", "64", "--stride", "10", "--out-dir", str(out)],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    sheet = files[0].with_name(files[0].name.replace("_motion_smplx.npz", "_preview.png"))
    assert (out / sheet.name).read_bytes() == sheet.read_bytes()
