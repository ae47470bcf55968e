"""Seeded inputs of the motion-smoothing tests (tests/test_smooth_cpu.py, tests/test_gpu_smooth.py), and the assertions that they reach every branch of the
header's text (include/amuse_hip.h amuse_smooth_motion):
  - joints beyond pi (class 1: a rotation about 3.5 rad, stored as it is) and below 1e-6 rad (class 2), with exact zeros among them;
  - both ends of a sequence and its interior; every bank row of m = 1, 4, 15;
  - sequences of L = 2 m (not filtered), 2 m + 1 (one window: every frame an edge frame) and 2 m + 2 for those m;
  - half-windows mixed by joint, 0 included;  33 sequences: one more than a launch holds.
Every motion is a smooth curve plus a little noise, so every relative rotation inside a window stays below 3.0 rad - asserted in float64 - and the shorter-arc
sign never hangs on a rounding.  Everything is computed once and handed out read-only."""
import functools

import numpy as np

import smooth_ref as ref

TILE = 32      # output frames of a workgroup (csrc/amuse_smooth_host.hpp kSmoothTile)
CAP = 32       # sequences per launch (csrc/amuse_seq_host.hpp kSeqPerLaunch; include/amuse_hip.h states it)
ORDER = 3
MIXED_HW = tuple([0, 1, 4, 15, 4, 2][j % 6] for j in range(55)) + (4,)
# 33 sequences: L = 2 m, 2 m + 1, 2 m + 2 of m = 1, 4, 15; one frame; one tile and a frame; several tiles
MIXED_FRAMES = (70, 2, 3, 4, 8, 9, 10, 30, 31, 32, 1, 33, 45, 61, 100, 64, 65, 5, 12, 17) + tuple(20 + 3 * s for s in range(13))
assert len(MIXED_FRAMES) == CAP + 1 and len(MIXED_HW) == ref.SLOTS


def joint_class(j):
    """0: an ordinary joint; 1: beyond pi; 2: below 1e-6 rad"""
    return 1 if j % 11 == 3 else 2 if j % 11 == 7 else 0


def motion(L, seed, noise=0.0):
    """(poses (L, 55, 3), trans (L, 3)) float32: per joint a fixed axis, an angle that moves slowly about a base value, a slow wobble of the axis"""
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64)[:, None, None]
    axis = rng.standard_normal((1, 55, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    cls = np.array([joint_class(j) for j in range(55)])
    base = rng.uniform(-2.5, 2.5, (1, 55, 1))
    base[:, cls == 1] = 3.5
    w, ph = rng.uniform(0.02, 0.09, (1, 55, 1)), rng.uniform(0, 2 * np.pi, (1, 55, 1))
    aa = axis * (base + 0.25 * np.sin(w * t + ph)) + 0.05 * np.sin(0.05 * t + rng.uniform(0, 2 * np.pi, (1, 55, 3)))
    aa = aa + noise * rng.standard_normal(aa.shape)
    tiny = 5e-7 * rng.uniform(-1, 1, aa.shape) / np.sqrt(3.0)
    aa[:, cls == 2] = tiny[:, cls == 2]
    aa[L // 2, 7] = 0.0                                                # an exact zero among the tiny rotations
    tt = np.arange(L, dtype=np.float64)[:, None]
    trans = np.array([1.0, 0.1, 0.5]) * np.sin(rng.uniform(0.02, 0.08, (1, 3)) * tt + rng.uniform(0, 6, (1, 3))) + noise * rng.standard_normal((L, 3))
    return aa.astype(np.float32), trans.astype(np.float32)


def max_relative_angle(poses, frames, hw):
    """float64: the largest angle between two frames that share a window (lags up to 2 m_j), over all sequences and joints"""
    worst, f0 = 0.0, 0
    for L in frames:
        for m in sorted(set(hw[:55])):
            js = [j for j in range(55) if hw[j] == m]
            if m == 0 or L < 2 * m + 1:
                continue
            p = poses[f0:f0 + L][:, js]
            for lag in range(1, 2 * m + 1):
                worst = max(worst, float(ref.geodesic(p[:-lag], p[lag:]).max()))
        f0 += L
    return worst


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _with_refs(poses, trans, frames, hw, order=ORDER):
    bk = ref.banks(order)
    p64, t64, mask = ref.smooth(poses, trans, frames, hw, bk)
    p32, t32, _ = ref.smooth(poses, trans, frames, hw, bk, np.float32)
    mj = mask[:, :55]
    f32_dist = float(ref.geodesic(p32[mj], p64[mj]).max())
    out = dict(poses=poses, trans=trans, frames=tuple(frames), hw=tuple(hw), order=order, bank=bk, p64=p64, t64=t64, mask=mask, f32_dist=f32_dist,
               bar=max(4.0 * f32_dist, 2.0 ** -20))
    if trans is not None:
        tm = mask[:, 55]
        out["t32_dist"] = float(np.abs(t32[tm].astype(np.float64) - t64[tm]).max())
        out["tbar"] = max(4.0 * out["t32_dist"], 2.0 ** -20 * float(np.abs(trans).max()))
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def mixed():
    """33 sequences, half-windows mixed by joint; asserts what the docstring lists"""
    parts = [motion(L, 100 + s, noise=0.01) for s, L in enumerate(MIXED_FRAMES)]
    poses, trans = np.concatenate([p for p, _ in parts]), np.concatenate([t for _, t in parts])
    hw = MIXED_HW
    c = _with_refs(poses, trans, MIXED_FRAMES, hw)
    ang = np.linalg.norm(poses.astype(np.float64), axis=-1)
    assert (ang > np.pi).any() and (ang < 1e-6).any() and not poses[MIXED_FRAMES[0] // 2, 7].any()
    for k in (0, 1, 2):                    # every joint class meets m = 0 and every filtering half-window of the bank-row check
        assert {hw[j] for j in range(55) if joint_class(j) == k} >= {0, 1, 4, 15}, k
    rows = {m: set() for m in (1, 4, 15)}
    ends = {m: set() for m in (1, 4, 15)}
    for L in MIXED_FRAMES:
        for m in rows:
            if L >= 2 * m + 1:
                s, r = ref.window_of(L, m)
                rows[m] |= set(r.tolist())
                ends[m] |= {"first" if (s == 0).any() and (r < m).any() else "", "interior" if ((r == m) & (s > 0) & (s < L - 1 - 2 * m)).any() else "",
                            "last" if (r > m).any() else ""}
    for m in rows:
        assert rows[m] == set(range(2 * m + 1)), (m, rows[m])                   # every bank row
        assert ends[m] >= {"first", "interior", "last"}, (m, ends[m])
        assert {2 * m, 2 * m + 1, 2 * m + 2} <= set(MIXED_FRAMES)
    assert set(hw) >= {0, 1, 4, 15} and len(MIXED_FRAMES) > CAP and max(MIXED_FRAMES) > 2 * TILE
    assert c["mask"].any() and (~c["mask"]).any()
    worst = max_relative_angle(poses, MIXED_FRAMES, hw)
    assert worst < 3.0, worst
    return c


@functools.lru_cache(maxsize=None)
def cubic(L=61, m=4):
    """a fixed-axis rotation whose angle is a cubic in time (peak 3.95 rad, span inside a window below 2 rad): a cubic is what an order-3 fit reproduces, so the
    analytic rotations themselves are the known answer.  One axis per joint; poses only."""
    rng = np.random.default_rng(7)
    axis = rng.standard_normal((1, 55, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    u = np.arange(L, dtype=np.float64) / (L - 1)
    theta = 3.95 * (3.0 * u ** 2 - 2.0 * u ** 3) - 0.4 * u * (1.0 - u)        # 0 at the first frame, 3.95 rad at the last, a skewed rise between
    exact = axis * theta[:, None, None]
    span = max(float(np.abs(theta[lag:] - theta[:-lag]).max()) for lag in range(1, 2 * m + 1))
    assert abs(theta.max() - 3.95) < 1e-12 and span < 2.0, span
    poses = exact.astype(np.float32)
    c = _with_refs(poses, None, (L,), (m,) * 56)
    c = dict(c)
    c["exact"] = exact
    # the bar of the known answer: the float32 restatement's distance from the ANALYTIC rotations (the inputs' own rounding to fp32 is part of it)
    p32, _, _ = ref.smooth(poses, None, (L,), (m,) * 56, c["bank"], np.float32)
    c["f32_dist_exact"] = float(ref.geodesic(p32, exact).max())
    c["bar_exact"] = max(4.0 * c["f32_dist_exact"], 2.0 ** -20)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def noisy(L=61, m=4, sigma=0.02):
    """a smooth motion and the same motion plus `sigma` rad of noise per component; joints of class 0 only are scored (tiny joints are all noise)"""
    clean, tclean = motion(L, 11)
    rng = np.random.default_rng(12)
    poses = (clean.astype(np.float64) + sigma * rng.standard_normal(clean.shape)).astype(np.float32)
    trans = (tclean.astype(np.float64) + sigma * rng.standard_normal(tclean.shape)).astype(np.float32)
    score = np.array([joint_class(j) == 0 for j in range(55)])
    c = dict(_with_refs(poses, trans, (L,), (m,) * 56))
    c.update(clean=clean, score=score)
    assert max_relative_angle(poses, (L,), (m,) * 56) < 3.0
    return _freeze(c)


def second_difference(aa):
    """mean geodesic second difference of (L, J, 3) axis-angle rows: the angle between R_{f-1}^T R_f and R_f^T R_{f+1}"""
    R = ref.rotmat(aa)
    d = np.swapaxes(R[:-1], -1, -2) @ R[1:]
    rel = np.swapaxes(d[:-1], -1, -2) @ d[1:]
    sk = np.stack([rel[..., 2, 1] - rel[..., 1, 2], rel[..., 0, 2] - rel[..., 2, 0], rel[..., 1, 0] - rel[..., 0, 1]], -1)
    return float(np.arctan2(0.5 * np.linalg.norm(sk, axis=-1), 0.5 * (np.trace(rel, axis1=-2, axis2=-1) - 1.0)).mean())


def noisy_inequalities(c, out):
    """the two inequalities of the noisy case on a filter output `out` (L, 55, 3): less jitter than the input, and closer to the clean motion"""
    sc = c["score"]
    j_in, j_out = second_difference(c["poses"][:, sc]), second_difference(out[:, sc])
    d_in, d_out = float(ref.geodesic(c["poses"][:, sc], c["clean"][:, sc]).mean()), float(ref.geodesic(out[:, sc], c["clean"][:, sc]).mean())
    return (j_in, j_out), (d_in, d_out)
