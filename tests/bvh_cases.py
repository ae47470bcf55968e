"""Seeded inputs of the BVH export tests (tests/test_bvh_cpu.py, tests/test_gpu_bvh.py).  Everything is computed once and handed out read-only.

Euler cases, per channel order - 2,200 rotations, which fill the 40 pose rows of three sequences of 1, 2 and 37 frames exactly:
  random        1,000 axis-angles, angles up to about 5 rad
  beyond_pi       300 angles in (pi, pi + 0.3]
  tiny            200 angles below 1e-3 (down to 1e-9), 20 exact zero vectors among them
  gimbal_exact    300 middle angle exactly +-90 degrees (as exactly as the fp32 axis-angle states it)
  gimbal_near     400 middle angle within 1e-3 degrees of +-90
Curves for the unwrap rule: `spin` (the first channel 0 -> 720 degrees over 37 frames in steps of 20, the others at 20 and 10: the principal values jump by 340) and
`fold` (the middle angle 60 -> 120 degrees over 36 frames, never exactly 90, the outer angles at 15 and 25: past 90 the principal outer channels jump by 180), each
on all 55 joints with a small per-joint offset; `wind` (150 degrees per frame: past 1000 degrees at the seventh frame)."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import bvh_ref as ref

NJ = 55
FRAMES3 = (1, 2, 37)
CLASSES = (("random", 1000), ("beyond_pi", 300), ("tiny", 200), ("gimbal_exact", 300), ("gimbal_near", 400))
assert sum(n for _, n in CLASSES) == sum(FRAMES3) * NJ


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def euler_cases(order):
    """-> {"aa": (2200, 3) float32, "cls": {name: slice}, "ref": as_euler float64 (2200, 3), "f32": the fp32 restatement's channels, "f32_geo": its worst
    geodesic distance (rad) after rounding to six decimals, "away": mask of the cases more than 1 degree from gimbal lock, "margin": 4 x the restatement's worst
    channel error (degrees, modulo 360) on those}"""
    g = np.random.default_rng(100 + ref.ORDERS.index(order))
    n = dict(CLASSES)
    unit = lambda m: (lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True))(g.standard_normal((m, 3)))
    parts = [g.standard_normal((n["random"], 3)) * 1.6,
             unit(n["beyond_pi"]) * (np.pi + g.uniform(1e-4, 0.3, (n["beyond_pi"], 1))),
             unit(n["tiny"]) * 10.0 ** g.uniform(-9, np.log10(9e-4), (n["tiny"], 1))]
    parts[2][:20] = 0.0
    sign = np.where(np.arange(n["gimbal_exact"]) % 2 == 0, 90.0, -90.0)
    parts.append(Rotation.from_euler(order, np.stack([g.uniform(-180, 180, sign.size), sign, g.uniform(-180, 180, sign.size)], -1), degrees=True).as_rotvec())
    sign = np.where(np.arange(n["gimbal_near"]) % 2 == 0, 1.0, -1.0)
    near = sign * (90.0 - 10.0 ** g.uniform(-7, -3, sign.size))
    parts.append(Rotation.from_euler(order, np.stack([g.uniform(-180, 180, sign.size), near, g.uniform(-180, 180, sign.size)], -1), degrees=True).as_rotvec())
    aa = np.concatenate(parts).astype(np.float32)
    cls, o = {}, 0
    for name, m in CLASSES:
        cls[name] = slice(o, o + m)
        o += m
    want = ref.euler_ref(aa, order)
    f32 = ref.euler_f32(aa, order)
    away = np.abs(np.abs(want[:, 1]) - 90.0) > 1.0
    err = np.abs(ref.mod360(f32.astype(np.float64) - want))[away]
    return {"aa": _ro(aa), "cls": cls, "ref": _ro(want), "f32": _ro(f32), "f32_geo": float(ref.geodesic(aa, np.round(f32.astype(np.float64), 6), order).max()),
            "away": _ro(away), "margin": 4.0 * float(err.max())}


def _curve_poses(order, curves):
    """curves (F, 55, 3) degrees in channel order -> poses (F, 55, 3) float32 axis-angle"""
    F = curves.shape[0]
    return _ro(Rotation.from_euler(order, curves.reshape(-1, 3), degrees=True).as_rotvec().reshape(F, NJ, 3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def spin(order):
    j = np.arange(NJ)[None, :]
    curves = np.stack(np.broadcast_arrays(20.0 * np.arange(37)[:, None], 20.0 + 0.5 * j, 10.0 + 0.25 * j), -1).astype(np.float64)
    return {"curves": _ro(curves), "poses": _curve_poses(order, curves)}


@functools.lru_cache(maxsize=None)
def fold(order):
    j = np.arange(NJ)[None, :]
    curves = np.stack(np.broadcast_arrays(15.0 + 0.2 * j, 60.0 + (60.0 / 35.0) * np.arange(36)[:, None], 25.0 + 0.1 * j), -1).astype(np.float64)
    assert not np.any(np.isclose(curves[..., 1], 90.0))
    return {"curves": _ro(curves), "poses": _curve_poses(order, curves)}


@functools.lru_cache(maxsize=None)
def wind(order, F=37):
    j = np.arange(NJ)[None, :]
    curves = np.stack(np.broadcast_arrays(150.0 * np.arange(F)[:, None], 20.0 + 0.0 * j, 10.0 + 0.0 * j), -1).astype(np.float64)
    return {"curves": _ro(curves), "poses": _curve_poses(order, curves)}


@functools.lru_cache(maxsize=None)
def clip300(seed=7):
    """one 300-frame motion: smooth per-joint curves of moderate speed, a translation that walks; poses (300, 55, 3), trans (300, 3) float32"""
    g = np.random.default_rng(seed)
    t = np.arange(300, dtype=np.float64)[:, None, None]
    axis = g.standard_normal((1, NJ, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    aa = axis * (g.uniform(-2.5, 2.5, (1, NJ, 1)) + 0.6 * np.sin(g.uniform(0.02, 0.1, (1, NJ, 1)) * t + g.uniform(0, 6, (1, NJ, 1)))) \
        + 0.2 * np.sin(0.05 * t + g.uniform(0, 6, (1, NJ, 3)))
    tt = np.arange(300, dtype=np.float64)[:, None]
    trans = np.array([1.5, 0.1, 0.8]) * np.sin(g.uniform(0.02, 0.08, (1, 3)) * tt + g.uniform(0, 6, (1, 3)))
    return {"poses": _ro(aa.astype(np.float32)), "trans": _ro(trans.astype(np.float32))}


@functools.lru_cache(maxsize=None)
def format_values():
    """4,096 fp32 values: random in +-1000, sixth-decimal ties k / 2^m (m <= 23), +-0, +-4e-7, +-999.99994 and the values around them"""
    g = np.random.default_rng(11)
    v = np.empty(4096, dtype=np.float32)
    v[:2048] = g.uniform(-999.9, 999.9, 2048).astype(np.float32)
    v[2048:3072] = (g.uniform(-9.9, 9.9, 1024) * 10.0 ** g.integers(-6, 0, 1024)).astype(np.float32)
    m = g.integers(7, 24, 1000)
    lim = np.minimum(2 ** 23, 999 * 2 ** m)
    k = g.integers(-lim, lim)
    v[3072:4072] = (k.astype(np.float64) / 2.0 ** m).astype(np.float32)         # exact binary fractions k / 2^m
    # x 1e6 ends in .5 exactly when x = q / 128 with q odd (1e6 / 128 = 7812.5): the true sixth-decimal ties, both parities of the digit before
    q = 2 * g.integers(-63999, 63999, 300) + 1
    v[3072:3372] = (q.astype(np.float64) / 128.0).astype(np.float32)
    assert np.all((v[3072:3372].astype(np.float64) * 1e6) % 1.0 == 0.5)
    edge = [0.0, -0.0, 4e-7, -4e-7, 5e-7, -5e-7, 999.99994, -999.99994, 0.5, -0.5, 1.5e-6, 2.5e-6, -2.5e-6, 0.0000005, 0.0000015, 9.9999995, 99.9999995, -99.9999995,
            1.0, -1.0, 10.0, -10.0, 100.0, -100.0]
    v[4072:4072 + len(edge)] = np.array(edge, dtype=np.float32)
    assert np.abs(v).max() < 999.9999995
    return _ro(v)
