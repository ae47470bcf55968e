"""CPU: known answers for tests/render_ref.py - the restatement the GPU tests compare against - that do not go through the renderer's own definitions: counted
coverage of rectangles and right triangles under the top-left rule, a sphere's silhouette and its brightest pixel, and the int64 bound of the depth numerator in
Python's unbounded integers."""
import numpy as np
import pytest

import render_cases as rc
import render_ref as rr


def _coverage(vertices, faces, Ws, Hs):
    """how many triangles cover each sample: every triangle rasterised alone"""
    rec = np.asarray([(x, y, 1000) for x, y in vertices], np.int32)
    count = np.zeros((Hs, Ws), np.int64)
    for f in faces:
        count += rr.raster(rec, [f], Ws, Hs) != rr.EMPTY
    return count


def _rect_truth(x0, y0, x1, y1, Ws, Hs):
    """top-left rule on an axis-aligned rectangle: centres with x0 <= Px < x1 and y0 <= Py < y1"""
    px, py = 16 * np.arange(Ws) + 8, 16 * np.arange(Hs) + 8
    return (((py >= y0) & (py < y1))[:, None] & ((px >= x0) & (px < x1))[None, :]).astype(np.int64)


@pytest.mark.parametrize("x0,y0,x1,y1", [(40, 24, 296, 200), (35, 21, 301, 187), (8, 8, 328, 232), (-100, -50, 1000, 90), (24, 24, 25, 300)])
def test_triangulated_rectangle_covers_every_interior_sample_once(x0, y0, x1, y1):
    Ws, Hs = 24, 16
    truth = _rect_truth(x0, y0, x1, y1, Ws, Hs)
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    mx, my = (x0 + x1) // 2, (y0 + y1) // 2
    meshes = {
        "diagonal_02": (corners, [(0, 1, 2), (0, 2, 3)]),
        "diagonal_13": (corners, [(0, 1, 3), (1, 2, 3)]),
        "other_winding": (corners, [(2, 1, 0), (3, 2, 0)]),
        "fan_from_inside": (corners + [(mx + 3, my - 2)], [(4, 0, 1), (4, 1, 2), (4, 2, 3), (4, 3, 0)]),
        "fan_from_a_centre": (corners + [(16 * (mx // 16) + 8, 16 * (my // 16) + 8)], [(4, 0, 1), (4, 1, 2), (4, 2, 3), (4, 3, 0)]),
        "strip": (corners + [(mx, y0), (mx, y1)], [(0, 4, 5), (0, 5, 3), (4, 1, 2), (4, 2, 5)]),
    }
    for name, (v, f) in meshes.items():
        if name.startswith("fan") and not (x0 < v[4][0] < x1 and y0 < v[4][1] < y1):      # (a fan needs its hub strictly inside)
            continue
        got = _coverage(v, f, Ws, Hs)
        assert np.array_equal(got, truth), (name, int(np.abs(got - truth).sum()))
    assert truth.sum() > 0 or (x1 - x0) < 16


@pytest.mark.parametrize("n", [1, 2, 5, 11])
def test_axis_aligned_right_triangles_cover_the_analytic_count(n):
    Ws = Hs = 16
    L = 16 * n
    count = lambda v: int(_coverage(v, [(0, 1, 2)], Ws, Hs).sum())
    # right angle top-left ON a centre: left and top edges count, the hypotenuse does not: i + j < n
    assert count([(8, 8), (8 + L, 8), (8, 8 + L)]) == n * (n + 1) // 2
    # its complement in the square [8, 8 + L)^2: right and bottom edges do not count, the hypotenuse (a left edge) does: i + j >= n
    assert count([(8 + L, 8), (8 + L, 8 + L), (8, 8 + L)]) == n * (n - 1) // 2
    # corner between centres: 16 (i + j) + 16 < 16 n
    assert count([(0, 0), (L, 0), (0, L)]) == n * (n - 1) // 2
    # either winding gives the same samples
    assert count([(8, 8), (8, 8 + L), (8 + L, 8)]) == n * (n + 1) // 2


def test_sphere_silhouette_and_brightest_pixel():
    from amuse_amd.render import Camera
    W = H = 64
    r, d = 1.0, 12.0
    v, f = rc.sphere_mesh(r=r)
    cam = Camera(np.diag([1.0, 1.0, -1.0]), [0.0, 0.0, d], 4.0 * W, 4.0 * W, W / 2, H / 2, d - 2.0, d + 2.0)
    for ss in (1, 2):
        rgb, keys, _ = rr.render(v, f, cam, W, H, ss)
        covered = int((keys != rr.EMPTY).sum())
        r_img = cam.fx * ss * r / np.sqrt(d * d - r * r)                 # a centred sphere's outline is a circle of this radius (in samples)
        want = np.pi * r_img ** 2
        print(f"ss {ss}: silhouette {covered} samples, pi r^2 = {want:.1f} ({covered / want - 1:+.3%}, bar 2 %)")
        assert abs(covered / want - 1) <= 0.02
        lum = rgb.astype(np.int64).sum(-1)
        assert lum[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].max() == lum.max() and lum.max() > lum[0, 0]
        assert (rgb[0, 0] == np.array(rr.DEFAULT_SHADING["bg_rgb"])).all()
        # flat shading under a headlight: the brightest level is the body colour at c ~ 1, the rim is near the ambient level
        assert abs(int(rgb[H // 2, W // 2, 0]) - 200) <= 1


def test_int64_numerator_bound_at_the_guard_band_corners():
    lo, hi, zmax = rr.GUARD_LO, rr.GUARD_HI, rr.ZMAX
    A2 = (hi - lo) * (hi - lo)                                               # the largest doubled area a triangle inside the guard band has
    assert A2 < 2 ** 35 and A2 * zmax < 2 ** 59 < 2 ** 63 - 1
    rec, faces = rc.crafted(64, 64)["guard_band_span"]
    keys = rr.raster(rec[0], faces, 64, 64)
    tri, zpix = rr.winners(keys)
    assert (tri >= 0).all()
    # the same depths in Python's own integers, at the screen's corners and centre
    for sy, sx in ((0, 0), (0, 63), (63, 0), (63, 63), (31, 32)):
        a, b, c = (tuple(int(x) for x in rec[0][i]) for i in faces[tri[sy, sx]])
        px, py = 16 * sx + 8, 16 * sy + 8
        a2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if a2 < 0:
            b, c, a2 = c, b, -a2
        e = lambda p, q: (q[0] - p[0]) * (py - p[1]) - (q[1] - p[1]) * (px - p[0])
        wa, wb, wc = e(b, c), e(c, a), e(a, b)
        assert min(wa, wb, wc) >= 0 and wa + wb + wc == a2
        num = wa * a[2] + wb * b[2] + wc * c[2]
        assert num < 2 ** 59 and num // a2 == zpix[sy, sx]


@pytest.mark.parametrize("ss", [1, 2])
def test_float32_restatement_stays_inside_the_gpu_tests_bars(ss):
    """what tests/test_gpu_render.py asks of the kernels, asked here of the float32 restatement on the same inputs (the shared V = 203 case): records within 1 unit
    of the float64 ones and at most 1 % different at all; at most 0.5 % of the pixels more than 1 level away end to end"""
    c = rc.body_case()
    v32 = c["v64"].astype(np.float32)
    r64, _ = rr.project(v32, c["cam"], ss)
    r32, _ = rr.project_f32(v32, c["cam"], ss)
    d = np.abs(r64.astype(np.int64) - r32)
    assert (r64[..., 2] >= 0).mean() > 0.9 and d.max() <= 1 and (d.max(-1) > 0).mean() <= 0.01
    bad = total = 0
    for f in range(v32.shape[0]):
        a, keys, _ = rr.render(c["v64"][f], c["faces"], c["cam"], c["width"], c["height"], ss)
        b, _, _ = rr.render(v32[f], c["faces"], c["cam"], c["width"], c["height"], ss, f32=True)
        bad += int((np.abs(a.astype(np.int64) - b).max(-1) > 1).sum())
        total += a.shape[0] * a.shape[1]
        assert 0.2 < (keys != rr.EMPTY).mean() < 1.0
    assert bad <= 0.005 * total, (bad, total)
