"""numpy restatement of the preview renderer's arithmetic (include/amuse_hip.h, "preview rendering"): the reference of tests/test_gpu_render.py and the subject
of tests/test_render_cases_cpu.py's known answers.  Projection in float64 (`project`) and in the kernel's own precisions (`project_f32`: fp32 fma chains for the
view position and X / Y, double for Zq); raster in int64 (Python's floor division); shading in float64.  Nothing here imports the library."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD_LO, GUARD_HI, ZMAX = -32768, 65535, (1 << 24) - 1
TILE, MAX_CHUNK, WS_BUDGET = 32, 256, 16 << 20
DEFAULT_SHADING = dict(light=(0.0, 0.0, -1.0), ambient=0.25, body_rgb=(200, 200, 208), bg_rgb=(32, 32, 36))


def plan(width, height, ss, V, T, frames):
    chunk = min(frames, MAX_CHUNK, max(1, WS_BUDGET // (24 * V)))
    section = -(-(chunk * V * 12) // 256) * 256
    return {"tiles_x": -(-(width * ss) // TILE), "tiles_y": -(-(height * ss) // TILE), "chunk_frames": chunk, "workspace_bytes": 2 * section}


def camera_f32(cam):
    """the camera as the C struct holds it: every number rounded to fp32 (an input of both restatements), as float64 arrays"""
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    return dict(R=f(cam.R).reshape(3, 3), t=f(cam.t).reshape(3), fx=float(f(cam.fx)), fy=float(f(cam.fy)), cx=float(f(cam.cx)), cy=float(f(cam.cy)),
                near=float(f(cam.near)), far=float(f(cam.far)))


def _snap(u, v, z, c, ss, finite):
    """(u, v) float, z float64 -> records int32 [..., 3]; invalid = (0, 0, -1)"""
    with np.errstate(invalid="ignore", over="ignore"):
        X, Y = np.rint(16.0 * ss * u), np.rint(16.0 * ss * v)
        ok = finite & (z >= c["near"]) & (z <= c["far"]) & (X >= GUARD_LO) & (X <= GUARD_HI) & (Y >= GUARD_LO) & (Y <= GUARD_HI)
        zs = np.where(ok, z, 1.0)
        zq = np.floor(c["far"] * (zs - c["near"]) / (zs * (c["far"] - c["near"])) * float(ZMAX) + 0.5)
    out = np.zeros(u.shape + (3,), np.int32)
    out[..., 0] = np.where(ok, X, 0)
    out[..., 1] = np.where(ok, Y, 0)
    out[..., 2] = np.where(ok, zq, -1)
    return out


def project(vertices, cam, ss):
    """all float64: vertices [..., V, 3] (fp32 values) -> (records int32 [..., V, 3], view positions float64 [..., V, 3])"""
    c = camera_f32(cam)
    x = np.asarray(vertices, np.float64)
    view = x @ c["R"].T + c["t"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = c["fx"] * view[..., 0] / view[..., 2] + c["cx"]
        v = c["cy"] - c["fy"] * view[..., 1] / view[..., 2]
    return _snap(u, v, view[..., 2], c, ss, np.isfinite(view).all(-1)), view


def _fma32(a, b, c):
    """fmaf on fp32 values: the product of two fp32 numbers is exact in double; the sum is rounded to double and then to fp32 (a double rounding that differs from
    the one rounding of a hardware fma only on ties that need more than 29 extra bits to see)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def project_f32(vertices, cam, ss):
    """the kernel's own precisions: view position and X / Y in fp32 (fma chains, t added first), Zq in double from a double z"""
    c = camera_f32(cam)
    x = np.asarray(vertices, np.float32)
    R, t = c["R"].astype(np.float32), c["t"].astype(np.float32)
    view = np.stack([_fma32(R[i, 0], x[..., 0], _fma32(R[i, 1], x[..., 1], _fma32(R[i, 2], x[..., 2], t[i]))) for i in range(3)], -1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = _fma32(np.float32(c["fx"]), view[..., 0] / view[..., 2], np.float32(c["cx"]))
        v = _fma32(np.float32(-c["fy"]), view[..., 1] / view[..., 2], np.float32(c["cy"]))
    x64 = x.astype(np.float64)
    zd = c["R"][2, 0] * x64[..., 0] + (c["R"][2, 1] * x64[..., 1] + (c["R"][2, 2] * x64[..., 2] + c["t"][2]))
    return _snap(u, v, zd, c, ss, np.isfinite(view).all(-1)), view


def _record_ok(r):
    return 0 <= r[2] <= ZMAX and GUARD_LO <= r[0] <= GUARD_HI and GUARD_LO <= r[1] <= GUARD_HI


def _edge(p, q, PX, PY):
    """int64 edge function of p -> q at the sample centres, and the top-left rule's verdict"""
    dx, dy = int(q[0] - p[0]), int(q[1] - p[1])
    E = dx * (PY - int(p[1])) - dy * (PX - int(p[0]))
    top_left = dy < 0 or (dy == 0 and dx > 0)
    return E, (E >= 0 if top_left else E > 0)


def raster(screen, faces, Ws, Hs):
    """records int [V, 3], faces int [T, 3] -> keys uint64 [Hs, Ws] (one frame)"""
    s = np.asarray(screen).astype(np.int64)
    keys = np.full((Hs, Ws), EMPTY, np.uint64)
    for t, (ia, ib, ic) in enumerate(np.asarray(faces).tolist()):
        a, b, c = s[ia], s[ib], s[ic]
        if not (_record_ok(a) and _record_ok(b) and _record_ok(c)):
            continue
        A2 = int((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
        if A2 == 0:
            continue
        if A2 < 0:
            b, c, A2 = c, b, -A2
        lox, hix = max(-((8 - int(min(a[0], b[0], c[0]))) // 16), 0), min((int(max(a[0], b[0], c[0])) - 8) // 16, Ws - 1)     # ceil, floor of (X - 8) / 16
        loy, hiy = max(-((8 - int(min(a[1], b[1], c[1]))) // 16), 0), min((int(max(a[1], b[1], c[1])) - 8) // 16, Hs - 1)
        if lox > hix or loy > hiy:
            continue
        PX = (16 * np.arange(lox, hix + 1, dtype=np.int64) + 8)[None, :]
        PY = (16 * np.arange(loy, hiy + 1, dtype=np.int64) + 8)[:, None]
        wc, okc = _edge(a, b, PX, PY)
        wa, oka = _edge(b, c, PX, PY)
        wb, okb = _edge(c, a, PX, PY)
        cover = okc & oka & okb
        if not cover.any():
            continue
        assert ((wa + wb + wc) == A2).all()
        zpix = (wa * int(a[2]) + wb * int(b[2]) + wc * int(c[2])) // A2
        key = ((zpix.astype(np.uint64) << np.uint64(32)) | np.uint64(t))
        sub = keys[loy:hiy + 1, lox:hix + 1]
        sub[cover] = np.minimum(sub[cover], key[cover])
    return keys


def winners(keys):
    """keys -> (triangle index int64, -1 where empty; zpix int64)"""
    k = np.asarray(keys).astype(np.uint64)
    empty = k == EMPTY
    return np.where(empty, -1, (k & np.uint64(0xFFFFFFFF)).astype(np.int64)), np.where(empty, -1, (k >> np.uint64(32)).astype(np.int64))


def shade(keys, view, faces, ss, shading=None):
    """keys [Hs, Ws], view positions [V, 3] -> uint8 [H, W, 3]; float64 throughout"""
    sh = dict(DEFAULT_SHADING, **(shading or {}))
    l = np.asarray(sh["light"], np.float64)
    l = (l / np.linalg.norm(l)).astype(np.float32).astype(np.float64)           # the unit vector as the kernel receives it
    amb = float(np.float32(sh["ambient"]))
    tri, _ = winners(keys)
    fc = np.asarray(faces)[np.maximum(tri, 0)]
    p = np.asarray(view, np.float64)
    n = np.cross(p[fc[..., 1]] - p[fc[..., 0]], p[fc[..., 2]] - p[fc[..., 0]])
    nn = np.linalg.norm(n, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(nn > 0, amb + (1.0 - amb) * np.abs(n @ l) / nn, amb)
    body, bg = np.asarray(sh["body_rgb"], np.float64), np.asarray(sh["bg_rgb"], np.int64)
    samples = np.where((tri >= 0)[..., None], np.minimum(255, np.floor(body * c[..., None] + 0.5)).astype(np.int64), bg)
    if ss == 1:
        return samples.astype(np.uint8)
    Hs, Ws = samples.shape[:2]
    s4 = samples.reshape(Hs // 2, 2, Ws // 2, 2, 3).sum(axis=(1, 3))
    return ((s4 + 2) >> 2).astype(np.uint8)


def render(vertices, faces, cam, width, height, ss, shading=None, f32=False):
    """one frame: vertices [V, 3] -> (rgb uint8 [H, W, 3], keys, records)"""
    rec, view = (project_f32 if f32 else project)(vertices, cam, ss)
    keys = raster(rec, faces, width * ss, height * ss)
    return shade(keys, view, faces, ss, shading), keys, rec
