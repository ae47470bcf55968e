"""Seeded inputs of the motion-metric tests (tests/test_motion_metrics_cpu.py, tests/test_gpu_motion_metrics.py): joint sequences [N, F, 55, 3] float32 with
coordinates within +-4 m, and the crafted cases of the issue.  Every case is built once (lru_cache) and never written to by a test."""
from functools import lru_cache

import numpy as np

NJ = 55
SHAPES = ((1, 2), (3, 5), (5, 67), (2, 300))
GRID = 1024.0               # crafted values are multiples of 2^-10: sums, shifts by grid constants and the 1000 m offset stay exact in fp32
OFFSET = np.array([1000.0, -1000.0, 1000.0], np.float32)
SHIFT = np.array([0.25, -0.5, 0.125], np.float32)


def _ro(a):
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def random_pair(N, F, seed=0):
    g = np.random.default_rng(1000 * seed + 10 * N + F)
    return _ro(g.uniform(-4, 4, (N, F, NJ, 3)).astype(np.float32)), _ro(g.uniform(-4, 4, (N, F, NJ, 3)).astype(np.float32))


@lru_cache(maxsize=None)
def grid_pair(N, F, seed=1):
    """values on the 2^-10 grid within +-3 m"""
    g = np.random.default_rng(2000 * seed + 10 * N + F)
    mk = lambda: _ro((g.integers(-3 * int(GRID), 3 * int(GRID) + 1, (N, F, NJ, 3)) / GRID).astype(np.float32))
    return mk(), mk()


def full_lengths(N, F):
    return np.full(N, F, np.int32)


@lru_cache(maxsize=None)
def constant_shift(N, F):
    """G = R + c with c on the grid: exact in fp32, so APE = |c| L and the velocities / accelerations of both are the same numbers"""
    R = grid_pair(N, F)[1]
    G = _ro((R + SHIFT).astype(np.float32))
    assert np.array_equal(G.astype(np.float64), R.astype(np.float64) + SHIFT.astype(np.float64))
    return G, R


@lru_cache(maxsize=None)
def static_pair(N, F):
    """every frame of a clip is its first frame (G and R differ from each other)"""
    G, R = random_pair(N, F, seed=3)
    return _ro(np.repeat(G[:, :1], F, 1).copy()), _ro(np.repeat(R[:, :1], F, 1).copy())


@lru_cache(maxsize=None)
def mixed_lengths(N, F):
    """lengths cycle through {2, 3, F} (cut at F); every frame at or beyond a clip's length is NaN in both sets"""
    G, R = (a.copy() for a in random_pair(N, F, seed=4))
    L = np.array([min((2, 3, F)[n % 3], F) for n in range(N)], np.int32)
    for n in range(N):
        G[n, L[n]:] = np.nan
        R[n, L[n]:] = np.nan
    return _ro(G), _ro(R), _ro(L)


@lru_cache(maxsize=None)
def offset_pair(N, F):
    """(G, R, G + 1000 m, R + 1000 m): grid values, so that the shifted sets are exactly representable in fp32 - the shift cancels exactly in every difference"""
    G, R = grid_pair(N, F, seed=5)
    Go, Ro = _ro((G + OFFSET).astype(np.float32)), _ro((R + OFFSET).astype(np.float32))
    for a, b in ((G, Go), (R, Ro)):
        assert np.array_equal(b.astype(np.float64), a.astype(np.float64) + OFFSET.astype(np.float64))
    return G, R, Go, Ro


@lru_cache(maxsize=None)
def alone_and_in_batch(F):
    """one clip alone, and as clip 3 of a batch of 5 with other lengths around it: (G1, R1, L1, G5, R5, L5, index)"""
    G5, R5 = random_pair(5, F, seed=6)
    L5 = np.array([F, 2, min(3, F), max(2, F - 1), F], np.int32)
    return _ro(G5[3:4].copy()), _ro(R5[3:4].copy()), _ro(L5[3:4].copy()), G5, R5, _ro(L5), 3


@lru_cache(maxsize=None)
def bad_lengths(F):
    """a batch of 4 with one clip of length 1 and one of length F + 1: exactly rows 1 and 2 are NaN"""
    G, R = random_pair(4, F, seed=7)
    return G, R, _ro(np.array([F, 1, F + 1, min(3, F)], np.int32)), (1, 2)


@lru_cache(maxsize=None)
def latents(n, seed=0, rank=None):
    """two sets of n latents [n, 128] with different means and covariances (rank: the rank of their spread, None = full)"""
    g = np.random.default_rng(300 + seed)
    k = 128 if rank is None else rank
    A, B = g.standard_normal((k, 128)), g.standard_normal((k, 128)) * 1.3
    return _ro(g.standard_normal((n, k)) @ A / np.sqrt(k)), _ro(g.standard_normal((n, k)) @ B / np.sqrt(k) + 0.2)
