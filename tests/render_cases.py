"""Inputs of the preview renderer's tests (tests/test_render_cases_cpu.py, tests/test_gpu_render.py): meshes, and integer screen records made by hand.
Coordinates are in 1/16 sample (include/amuse_hip.h, "preview rendering"): sample (sx, sy) has its centre at (16 sx + 8, 16 sy + 8)."""
import numpy as np

ZMAX = (1 << 24) - 1
# (width, height, ss) of the exact raster tests: partial tiles in both axes; supersampled; the width limit
SHAPES = {"72x40_ss1": (72, 40, 1), "40x24_ss2": (40, 24, 2), "2048x16_ss1": (2048, 16, 1)}


def random_faces(V=203, T=400, seed=11):
    """T triangles over V vertices, no repeated vertex inside a triangle"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(V, 3, replace=False) for _ in range(T)]).astype(np.int32)


def sphere_mesh(n_lat=25, n_lon=48, r=1.0, centre=(0.0, 0.0, 0.0), stretch=0.0):
    """UV sphere (poles on the y axis; stretch > 0 pulls the two halves apart along y: a capsule) -> (vertices float32 [V, 3], faces int32 [T, 3]).
    The longitudes are offset by half a step and n_lat is odd, so that ONE planar quad faces +z head on."""
    v = [(0.0, r + stretch, 0.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * (j + 0.5) / n_lon
            y = r * np.cos(th)
            v.append((r * np.sin(th) * np.sin(ph), y + (stretch if th < np.pi / 2 else -stretch), r * np.sin(th) * np.cos(ph)))
    v.append((0.0, -r - stretch, 0.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = []
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return (np.asarray(v) + np.asarray(centre)).astype(np.float32), np.asarray(f, np.int32)


def subdivide(vertices, faces):
    """every triangle into four (midpoints shared between neighbours)"""
    v = [tuple(x) for x in np.asarray(vertices, np.float64)]
    mid, out = {}, []

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            mid[k] = len(v)
            v.append(tuple(0.5 * (np.asarray(v[a]) + np.asarray(v[b]))))
        return mid[k]
    for a, b, c in np.asarray(faces).tolist():
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.asarray(v, np.float32), np.asarray(out, np.int32)


def fuzz(Ws, Hs, seed, V=150, T=200, M=3):
    """M frames of records [M, V, 3] and T faces over them: vertices on and off the screen, a quarter exactly on sample centres, repeated positions, a few invalid;
    faces: half of them small (a vertex and two near neighbours made for it), some naming a vertex twice"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((M, V, 3), np.int64)
    for m in range(M):
        x = rng.integers(-40 * 16, (Ws + 40) * 16, V)
        y = rng.integers(-40 * 16, (Hs + 40) * 16, V)
        on = rng.random(V) < 0.25
        x[on], y[on] = 16 * rng.integers(-2, Ws + 2, on.sum()) + 8, 16 * rng.integers(-2, Hs + 2, on.sum()) + 8
        far = rng.random(V) < 0.05
        x[far], y[far] = rng.integers(-32768, 65536, far.sum()), rng.integers(-32768, 65536, far.sum())
        # small triangles: vertices 3k + 1, 3k + 2 sit within 3 samples of vertex 3k (k < V / 6)
        for k in range(V // 6):
            x[3 * k + 1:3 * k + 3] = x[3 * k] + rng.integers(-48, 49, 2)
            y[3 * k + 1:3 * k + 3] = y[3 * k] + rng.integers(-48, 49, 2)
        dup = rng.choice(V, 10, replace=False)
        x[dup[:5]], y[dup[:5]] = x[dup[5:]], y[dup[5:]]                      # repeated positions
        rec[m, :, 0], rec[m, :, 1] = np.clip(x, -32768, 65535), np.clip(y, -32768, 65535)
        rec[m, :, 2] = rng.integers(0, ZMAX + 1, V)
        rec[m, rng.choice(V, 3, replace=False), 2] = -1                      # invalid vertices
    faces = rng.integers(0, V, (T, 3))
    for k in range(V // 6):
        faces[k] = (3 * k, 3 * k + 1, 3 * k + 2)
    faces[-3:, 1] = faces[-3:, 0]                                            # a vertex named twice: zero area
    return rec.astype(np.int32), faces.astype(np.int32)


def crafted(Ws, Hs):
    """name -> (records int32 [1, V, 3], faces int32 [T, 3]) for a Ws x Hs sample grid (Ws >= 16, Hs >= 16)"""
    X1, Y1 = 16 * Ws, 16 * Hs
    c = lambda k: 16 * k + 8
    out = {}
    # two triangles sharing the diagonal of a quad whose corners lie off the sample centres
    out["shared_edge_quad"] = ([(37, 21, 5000), (X1 - 43, 29, 900000), (X1 - 35, Y1 - 31, 16000000), (45, Y1 - 37, 70000)], [(0, 1, 2), (0, 2, 3)])
    # every vertex exactly on a sample centre, two triangles sharing an edge; and an axis-aligned right triangle with centres on all three edges
    out["on_centres"] = ([(c(2), c(2), 100), (c(Ws - 4), c(3), 200), (c(5), c(Hs - 2), 300), (c(Ws - 2), c(Hs - 3), 400), (c(1), c(1), 50), (c(9), c(1), 50), (c(1), c(9), 50)],
                         [(0, 1, 2), (2, 1, 3), (4, 5, 6)])
    # zero area (collinear, and a repeated position), a sliver thinner than a sample crossing the screen, a triangle inside one sample that misses its centre
    out["degenerate"] = ([(20, 40, 7), (520, 290, 7), (270, 165, 7), (20, 40, 9), (20, c(5) - 1, 1000), (X1 - 20, c(5), 2000), (20, c(5) + 1, 3000), (c(3) + 1, c(3) + 1, 5),
                          (c(3) + 6, c(3) + 2, 5), (c(3) + 2, c(3) + 7, 5)], [(0, 1, 2), (0, 3, 1), (4, 5, 6), (7, 8, 9)])
    # the same triangle three times at equal depth (once with the other winding): the lowest index wins everywhere
    out["coincident"] = ([(30, 30, 4000), (X1 - 30, 50, 4000), (X1 // 2, Y1 - 30, 4000)], [(0, 1, 2), (0, 1, 2), (2, 1, 0)])
    # two triangles whose depths cross inside the screen
    out["interpenetrating"] = ([(10, 10, 1000000), (X1 - 10, 20, 15000000), (X1 // 2, Y1 - 10, 8000000), (12, 14, 15000000), (X1 - 14, 12, 1000000), (X1 // 2 + 9, Y1 - 14, 8000000)],
                               [(0, 1, 2), (3, 4, 5)])
    # one invalid vertex skips the whole triangle (Zq = -1; Zq beyond 24 bits; X outside the guard band); the valid triangle behind them shows
    out["invalid_vertex"] = ([(10, 10, 100), (X1 - 10, 10, 100), (X1 // 2, Y1 - 10, -1), (10, 10, 100), (X1 - 10, 10, ZMAX + 1), (X1 // 2, Y1 - 10, 100), (70000, 10, 100),
                              (20, 20, 9000000), (X1 - 20, 30, 9000000), (X1 // 2, Y1 - 20, 9000000)], [(0, 1, 2), (3, 4, 5), (0, 6, 5), (7, 8, 9)])
    # one triangle cut by all four viewport edges, from deep in the guard band
    out["clipped"] = ([(-3000, -2000, 12345), (X1 + 5000, Y1 // 2, 9999999), (X1 // 2, Y1 + 7000, 500)], [(0, 1, 2)])
    # guard band to guard band: the largest doubled area and the largest depth there are (the int64 numerator's bound)
    out["guard_band_span"] = ([(-32768, -32768, ZMAX), (65535, -32768, ZMAX), (-32768, 65535, ZMAX - 1), (65535, 65535, 0)], [(0, 1, 2), (1, 3, 2)])
    return {k: (np.asarray(v, np.int32)[None], np.asarray(f, np.int32)) for k, (v, f) in out.items()}


def body_case(seed=2, width=64, height=48, frames=3):
    """The V = 203 synthetic body model with random faces, `frames` posed frames of one clip and a front camera framed on their joints: what the projection,
    shading and end-to-end tests share.  -> dict(model, faces, betas, aa, trans, v64 float64 [F, V, 3], cam); computed on the CPU (body.torch_forward)."""
    import torch
    import body_cases as bc
    from amuse_amd import body, render
    faces = random_faces(203, 400)
    model = body.BodyModel.from_dict(dict(bc.make_model(V=203), faces=faces))
    betas = bc.make_betas(S=1)
    aa, trans, _ = bc.make_motion(N=1, F=frames, seed=seed)
    j64, v64 = body.torch_forward(model, betas, torch.from_numpy(aa), torch.from_numpy(trans))
    cam = render.Camera.front(j64.numpy(), width, height)
    return dict(model=model, faces=faces, betas=betas, aa=aa, trans=trans, v64=v64[0].numpy(), cam=cam, width=width, height=height)
