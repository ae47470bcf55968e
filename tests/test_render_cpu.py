"""CPU: the preview renderer without a GPU - the library's plan (amuse_render_plan) against tests/render_ref.py's restatement, every refusal of the entry points
(made before any HIP call), the PNG writer through a zlib decode, BodyModel with and without its triangles, Camera.front's framing, the contact sheet, and the
command lines' SystemExit paths."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest
import torch

import body_cases as bc
import render_cases as rc
import render_ref as rr
from amuse_amd import _lib, body, render


def test_plan_against_the_restatement():
    for w, h, ss in ((1, 1, 1), (32, 32, 1), (33, 31, 1), (72, 40, 1), (40, 24, 2), (512, 512, 2), (1024, 1024, 2), (2048, 16, 1), (16, 2048, 1), (1000, 7, 2)):
        for V in (1, 3, 203, 2730, 2731, 10475, 699050, 699051, 5000000):
            for frames in (1, 2, 66, 67, 255, 256, 257, 300, 100000):
                assert render.plan(w, h, ss, V, 5, frames) == rr.plan(w, h, ss, V, 5, frames), (w, h, ss, V, frames)
    p = render.plan(512, 512, 1, 10475, 20908, 300)
    assert p == {"tiles_x": 16, "tiles_y": 16, "chunk_frames": 66, "workspace_bytes": 2 * 8296448}          # 66 x 10475 x 12 = 8,296,200 -> 8,296,448
    assert render.plan(32, 32, 1, 203, 400, 1000)["chunk_frames"] == 256
    lib = _lib.load()
    assert lib.amuse_render_plan(64, 64, 1, 10, 10, 5, None, None, None, None) == 0                           # every output is optional


def test_refusals_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.amuse_last_error().decode()
    plan = lambda w=64, h=64, ss=1, V=10, T=10, fr=5: lib.amuse_render_plan(w, h, ss, V, T, fr, None, None, None, None)
    assert plan(ss=0) == -1 and "ss" in err() and plan(ss=3) == -1 and plan(ss=4) == -1
    assert plan(w=2049) == -1 and "2048" in err() and plan(h=2049) == -1 and plan(w=1025, ss=2) == -1 and plan(w=0) == -1 and plan(h=-4) == -1
    assert plan(w=2048, h=2048) == 0 and plan(w=1024, h=1024, ss=2) == 0
    assert plan(V=0) == -1 and plan(T=0) == -1 and plan(fr=0) == -1 and "frames" in err()
    with pytest.raises(_lib.AmuseHipError):
        render.plan(64, 64, 3, 10, 10, 5)
    # create: refused before the device is touched
    ip = C.POINTER(C.c_int)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    create = lambda f=faces, T=2, V=4, w=64, h=64, ss=1: lib.amuse_renderer_create(0, f.ctypes.data_as(ip) if f is not None else None, T, V, w, h, ss)
    assert create(V=3) is None and "outside 0..2" in err()                                                     # index 3 with three vertices
    bad = faces.copy()
    bad[1, 2] = -1
    assert create(f=bad) is None and "face 1" in err()
    assert create(f=None) is None and "NULL" in err()
    assert create(ss=3) is None and create(w=4096) is None and create(T=0) is None and create(V=0) is None
    # the calls' own checks come before any HIP call: a renderer's host struct is enough (the addresses are never read)

    class R(C.Structure):
        _fields_ = [("device", C.c_int), ("T", C.c_int), ("V", C.c_int), ("W", C.c_int), ("H", C.c_int), ("ss", C.c_int), ("faces", C.c_void_p), ("ws", C.c_void_p),
                    ("ws_bytes", C.c_size_t), ("retired", C.c_void_p * 3)]
    r = R(0, 2, 4, 64, 64, 1, None, None, 0)
    cam = render.Camera(np.diag([1.0, 1.0, -1.0]), [0, 0, 5], 100, 100, 32, 32, 1.0, 9.0)
    one = 0x1000

    def call(h=C.byref(r), v=one, M=2, c=cam, sh=None, rgb=one):
        cc = c.to_c() if c is not None else None
        sc = sh.to_c() if sh is not None else None
        return lib.amuse_render(h, v, M, C.byref(cc) if cc is not None else None, C.byref(sc) if sc is not None else None, rgb, None, None, None)
    assert call(h=None) == -1 and "NULL" in err()
    assert call(v=None) == -1 and call(c=None) == -1 and call(rgb=None) == -1 and "must be given" in err()
    assert call(M=0) == -1 and "M 0" in err() and call(M=-2) == -1

    def with_cam(**kw):
        c = render.Camera(cam.R, cam.t, cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.far)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert call(c=with_cam(near=0.0)) == -1 and "near_z" in err()
    assert call(c=with_cam(near=-1.0)) == -1 and call(c=with_cam(near=9.0)) == -1 and call(c=with_cam(near=10.0)) == -1
    assert call(c=with_cam(fx=float("nan"))) == -1 and "non-finite" in err() and call(c=with_cam(far=float("inf"))) == -1
    assert call(c=with_cam(t=np.array([0.0, float("inf"), 1.0]))) == -1
    assert call(sh=render.Shading(light=(0, 0, 0))) == -1 and "light" in err()
    assert call(sh=render.Shading(ambient=1.5)) == -1 and "ambient" in err() and call(sh=render.Shading(ambient=-0.1)) == -1
    r.ss = 3
    assert call() == -1 and "ss" in err()
    r.ss = 1
    raster = lambda h=C.byref(r), s=one, M=1, k=one: lib.amuse_debug_render_raster(h, s, M, k, None)
    assert raster(h=None) == -1 and raster(s=None) == -1 and raster(k=None) == -1 and raster(M=0) == -1 and "M 0" in err()
    with pytest.raises(_lib.AmuseHipError, match="no CPU fallback"):
        render.Renderer("cpu", faces, 4, 64, 64)


def _decode_png(data):
    """-> uint8 [H, W, C]: 8-bit, non-interlaced, filter 0 on every row (what write_png writes), every CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body_, crc = data[pos + 8:pos + 8 + n], struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        assert zlib.crc32(tag + body_) & 0xFFFFFFFF == crc, tag
        chunks.append((tag, body_))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, ch)


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 3), (7, 13, 3), (64, 48, 3), (5, 9)):
        a = rng.integers(0, 256, shape).astype(np.uint8)
        render.write_png(tmp_path / "a.png", a)
        data = (tmp_path / "a.png").read_bytes()
        assert data == render.png_bytes(a)
        assert np.array_equal(_decode_png(data), a.reshape(shape[0], shape[1], -1))
    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            render.png_bytes(bad)


def test_contact_sheet():
    f = np.arange(7 * 2 * 3 * 3, dtype=np.uint8).reshape(7, 2, 3, 3)
    s = render.contact_sheet(f, 3)
    assert s.shape == (6, 9, 3)
    for i in range(7):
        assert np.array_equal(s[2 * (i // 3):2 * (i // 3) + 2, 3 * (i % 3):3 * (i % 3) + 3], f[i])
    assert (s[4:, 3:] == f[0, 0, 0]).all()                                   # the two empty cells: frame 0's corner
    assert render.contact_sheet(f[:2], 6).shape == (2, 6, 3)                 # fewer frames than columns: no empty cells


def test_body_model_with_and_without_faces(tmp_path):
    d = bc.make_model(V=203)
    plain = body.BodyModel.from_dict(d)
    assert plain.faces is None
    plain.to_npz(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as z:
        assert "f" not in z.files and sorted(z.files) == sorted(body.NPZ_KEYS)
    assert body.BodyModel.from_npz(tmp_path / "plain.npz").faces is None
    faces = rc.random_faces(203, 400)
    m = body.BodyModel.from_dict(dict(d, faces=faces))
    assert m.faces.dtype == np.int32 and np.array_equal(m.faces, faces)
    m.to_npz(tmp_path / "faces.npz")
    back = body.BodyModel.from_npz(tmp_path / "faces.npz")
    assert np.array_equal(back.faces, faces) and back.faces.dtype == np.int32
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "parents"):
        assert np.array_equal(getattr(back, k), getattr(plain, k)), k
    for bad in (faces[:, :2], np.array([[0, 1, 203]]), np.array([[0, -1, 2]]), np.zeros((0, 3), np.int32)):
        with pytest.raises(ValueError, match="faces"):
            body.BodyModel.from_dict(dict(d, faces=bad))


def test_camera_front_known_answers():
    pts = np.array([[[-0.5, -1.0, 0.0], [0.5, 1.0, 0.2]], [[0.1, 0.3, 0.1], [-0.2, 0.0, 0.05]]])
    cam = render.Camera.front(pts, 512, 512)
    f = 75.0 / 36.0 * 512
    assert cam.fx == cam.fy == pytest.approx(f) and (cam.cx, cam.cy) == (256.0, 256.0)
    assert np.array_equal(cam.R, np.diag([1.0, 1.0, -1.0]))
    half = np.array([0.7, 1.25, 0.26])                                       # 0.5 x extent x 1.1 + 0.15
    dist = 1.25 * f / 256 + 0.26
    assert np.allclose(cam.t, [0.0, 0.0, 0.1 + dist])
    # the grown box's front face touches the image's top and bottom rows (the limiting axis), and is centred
    proj = lambda p: (cam.fx * (cam.R @ p + cam.t)[0] / (cam.R @ p + cam.t)[2] + cam.cx, cam.cy - cam.fy * (cam.R @ p + cam.t)[1] / (cam.R @ p + cam.t)[2])
    c = np.array([0.0, 0.0, 0.1])
    assert proj(c + half * [0, 1, 1]) == pytest.approx((256.0, 0.0)) and proj(c + half * [0, -1, 1]) == pytest.approx((256.0, 512.0))
    u_right, _ = proj(c + half * [1, 0, 1])
    assert 256 < u_right < 512                                               # world +x is image right, inside the frame
    assert 0 < cam.near < dist - 0.26 and cam.far > dist + 0.26              # the whole box lies between the planes
    wide = render.Camera.front(pts * [3.0, 0.2, 1.0], 640, 360)
    assert wide.fx == pytest.approx(75.0 / 36.0 * 640) and (wide.cx, wide.cy) == (320.0, 180.0)
    assert render.Camera.front(pts, 512, 512, distance=9.0).t[2] == pytest.approx(9.1)
    cc = cam.to_c()
    assert list(cc.R) == [1, 0, 0, 0, 1, 0, 0, 0, -1] and cc.near_z == np.float32(cam.near) and cc.fx == np.float32(f)


def _model_dir(path, with_faces=True):
    path.mkdir(parents=True, exist_ok=True)
    d = bc.make_model(V=203)
    m = body.BodyModel.from_dict(dict(d, faces=rc.random_faces(203, 400)) if with_faces else d)
    for name in body.SMPLX_FILES.values():
        m.to_npz(path / name)
    return path


def test_command_lines_refuse_before_any_gpu_work(tmp_path):
    from conftest import make_reference_tree
    from amuse_amd import main as cli
    root = make_reference_tree(tmp_path / "tree")
    base = ["--fn", "infer_gesture", "--root", str(root), "--random-init"]
    empty = tmp_path / "no_models"
    empty.mkdir()
    with pytest.raises(SystemExit, match=str(empty)):
        cli.main(base + ["--preview", "--smplx-models", str(empty)])
    with pytest.raises(SystemExit, match=str(root / "body_models" / "codebase" / "models" / "smplx")):         # the default directory, as train_gesture's
        cli.main(base + ["--preview"])
    nofaces = _model_dir(tmp_path / "nofaces", with_faces=False)
    with pytest.raises(SystemExit, match="'f'"):
        cli.main(base + ["--preview", "--smplx-models", str(nofaces)])
    with pytest.raises(SystemExit, match="'f'"):
        cli.main(["--fn", "edit_gesture", "--root", str(root), "--preview", "--smplx-models", str(nofaces)])
    with pytest.raises(SystemExit, match="--preview belongs to"):
        cli.main(["--fn", "train_gesture", "--root", str(root), "--preview"])
    with pytest.raises(SystemExit, match="--preview-frames belongs to"):
        cli.main(base + ["--preview-frames"])
    good = _model_dir(tmp_path / "models")
    with pytest.raises(SystemExit, match="--preview-size"):
        cli.main(base + ["--preview", "--smplx-models", str(good), "--preview-size", "2000"])
    with pytest.raises(SystemExit, match="--preview-stride"):
        cli.main(base + ["--preview", "--smplx-models", str(good), "--preview-stride", "0"])
    # python -m amuse_amd.render
    with pytest.raises(SystemExit, match=str(empty)):
        render.main(["x_motion_smplx.npz", "--smplx-models", str(empty)])
    with pytest.raises(SystemExit, match="'f'"):
        render.main(["x_motion_smplx.npz", "--smplx-models", str(nofaces)])
    with pytest.raises(SystemExit, match="does not exist"):
        render.main([str(tmp_path / "x_motion_smplx.npz"), "--smplx-models", str(good)])
    models = render.load_preview_models(good)
    assert sorted(models) == ["female", "male", "neutral"] and all(m.faces.shape == (400, 3) for m in models.values())
    sheet, frames_dir = render.preview_paths(tmp_path / "seq_0" / "scott_seq_0_AbC123_motion_smplx.npz")
    assert sheet == tmp_path / "seq_0" / "scott_seq_0_AbC123_preview.png" and frames_dir == tmp_path / "seq_0" / "scott_seq_0_AbC123_preview"
    assert render.preview_paths("other.npz", tmp_path)[0] == tmp_path / "other_preview.png"
