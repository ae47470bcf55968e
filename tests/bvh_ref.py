"""The BVH export restated for the tests (tests/test_bvh_cpu.py, tests/test_gpu_bvh.py): scipy's Rotation in float64 as the reference of the Euler channels,
the unwrap rule of include/amuse_hip.h in numpy float64, Python's "%11.6f" as the reference of the text, a Python depth-first walk as the reference of the
layout - and the kernel's own fp32 arithmetic restated in numpy float32 (`euler_f32`), whose distance from the float64 reference sets the per-channel margin."""
import numpy as np
from scipy.spatial.transform import Rotation

ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")
COLS, FIELD = 168, 12


def dfs(parents):
    """depth-first, children in ascending index"""
    kids = {j: [] for j in range(len(parents))}
    for j in range(1, len(parents)):
        kids[int(parents[j])].append(j)
    out = []

    def walk(j):
        out.append(j)
        for k in kids[j]:
            walk(k)
    walk(0)
    return out


def fmt(values, per_row=COLS) -> bytes:
    """Python's "%11.6f" and the separators; a value outside the field's stated range (|x| rounding to 1000 or more at six decimals, NaN, infinity) is '#' x 11"""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    field = lambda x: "%11.6f" % float(x) if np.isfinite(x) and abs(float(x)) < 999.9999995 else "#" * 11
    return "".join(field(x) + ("\n" if i % per_row == per_row - 1 else " ") for i, x in enumerate(v)).encode("ascii")


def parse(block: bytes, cols=COLS) -> np.ndarray:
    return np.array(bytes(block).split(), dtype=np.float64).reshape(-1, cols)


def euler_ref(aa, order) -> np.ndarray:
    """float64: scipy's intrinsic Tait-Bryan angles of the rotations the fp32 inputs name, degrees"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # (scipy warns at gimbal lock: those cases are held to the rotation, not to the channels)
        return Rotation.from_rotvec(np.asarray(aa, dtype=np.float64).reshape(-1, 3)).as_euler(order, degrees=True)


def geodesic(aa, deg, order) -> np.ndarray:
    """rad: between the rotations the axis-angle rows name and those the Euler channels (degrees, the file's channel order) name; float64"""
    a = Rotation.from_rotvec(np.asarray(aa, dtype=np.float64).reshape(-1, 3))
    b = Rotation.from_euler(order, np.asarray(deg, dtype=np.float64).reshape(-1, 3), degrees=True)
    return (a.inv() * b).magnitude()


def geodesic_aa(a, b) -> np.ndarray:
    return (Rotation.from_rotvec(np.asarray(a, np.float64).reshape(-1, 3)).inv() * Rotation.from_rotvec(np.asarray(b, np.float64).reshape(-1, 3))).magnitude()


def mod360(d):
    return (np.asarray(d, dtype=np.float64) + 180.0) % 360.0 - 180.0


def euler_f32(aa, order) -> np.ndarray:
    """the header's arithmetic in numpy float32: half-angle quaternion, half-sum / half-difference angles, degrees, principal values"""
    f = np.float32
    aa = np.asarray(aa, dtype=f).reshape(-1, 3)
    i, j, k = ("XYZ".index(c) for c in order)
    e = f(1) if (k + 1) % 3 == j else f(-1)
    ang = np.sqrt((aa * aa).sum(-1, dtype=f)).astype(f)
    half = (f(0.5) * ang).astype(f)
    with np.errstate(all="ignore"):
        s = np.where(ang < f(1e-3), f(0.5) - ang * ang / f(48), np.sin(half) / ang).astype(f)
    w, v = np.cos(half).astype(f), (aa * s[:, None]).astype(f)
    qi, qj, qk = v[:, i], v[:, j], v[:, k]
    a, b, c, d = w - qj, qk + e * qi, qj + w, e * qi - qk
    mid = f(2) * np.arctan2(np.hypot(c, d), np.hypot(a, b)).astype(f) - f(np.pi / 2)
    ls, ld = (a == 0) & (b == 0), (c == 0) & (d == 0)
    hs, hd = np.where(ls, f(0), np.arctan2(b, a)).astype(f), np.where(ld, f(0), np.arctan2(d, c)).astype(f)
    hs, hd = np.where(ls, hd, hs), np.where(ld, hs, hd)
    kdeg = f(180.0 / np.pi)
    wrap = lambda x: (x - f(360) * np.floor((x + f(180)) / f(360))).astype(f)
    return np.stack([wrap(e * (hs + hd) * kdeg), (mid * kdeg).astype(f), wrap((hs - hd) * kdeg)], -1).astype(f)


def unwrap(principal) -> np.ndarray:
    """the header's rule, float64: principal (F, ..., 3) degrees -> the emitted curves.  Frame 0 keeps its values; frame t weighs (a, b, c) against
    (a + 180, 180 - b, c + 180), each channel moved by the multiple of 360 nearest to frame t - 1's emitted value, by the sum of absolute differences; ties
    keep the first."""
    p = np.asarray(principal, dtype=np.float64)
    out = p.copy()
    near = lambda x, prev: x + 360.0 * np.rint((prev - x) / 360.0)
    for t in range(1, p.shape[0]):
        prev = out[t - 1]
        A = near(p[t], prev)
        B = near(np.stack([p[t][..., 0] + 180.0, 180.0 - p[t][..., 1], p[t][..., 2] + 180.0], -1), prev)
        ca, cb = np.abs(A - prev).sum(-1), np.abs(B - prev).sum(-1)
        out[t] = np.where((cb < ca)[..., None], B, A)
    return out
