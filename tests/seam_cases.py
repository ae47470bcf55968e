"""Inputs of the seam-cost tests (tests/test_seam_cases_cpu.py, tests/test_gpu_seam.py): candidate windows whose overlap rows pair up as joint classes, mixed
in one tensor by joint index as tests/test_gpu_longform.py `_make` mixes them (class = joint index mod 7).  With R a seam's base rows, a_c the overlap rows of
candidate c of the earlier window (rows i + hop) and b_c those of candidate c of the later one (rows i):
  0  independent rotations up to 3.6 rad for every candidate on both sides (beyond pi occurs)
  1  a_c == b_c' == R for all c, c'
  2  a_c = R, b_c = R + 1e-4 noise_c
  3  a_c = R + 1e-2 noise_c, b_c = R + 1e-2 noise'_c
  4  a_c = R, b_c = the 2 pi - theta alias of R (the same rotation, the other hemisphere)
  5  both sides below 1e-6 rad
  6  exact zeros on the a side for even c and on the b side for c % 3 == 0 (so: one side, the other, both), small rotations elsewhere
Some joint weights are 0 and row_weight is not uniform.  Everything is computed once per case and shared read-only."""
import functools

import numpy as np

import seam_ref as ref

CAP = 32      # sequences per launch (csrc/amuse_seq_host.hpp kSeqPerLaunch)
N_CLASSES = 7

# (F, hop, windows, frames, K, with translation)
CASES = {
    "two_sequences": (12, 9, (3, 1), (30, 12), 2, True),
    "cut_short": (12, 9, (3, 2, 4), (25, 10, 28), 5, True),            # cut-short last windows; O_k = 1 for the last seams of sequences 1 and 2
    "capacity_plus_one": (4, 2, tuple(1 + s % 3 for s in range(CAP + 1)), tuple((s % 3) * 2 + 4 - (s % 2) * (s % 3 > 0) for s in range(CAP + 1)), 3, True),
    "one_candidate": (12, 9, (2,), (21,), 1, False),
    "product_hop270": (300, 270, (3,), (840,), 16, True),
    "product_hop150": (300, 150, (3,), (600,), 4, True),
    "k64": (12, 9, (3,), (27,), 64, True),
}


def rand_aa(rng, shape, max_angle):
    ax = rng.standard_normal(shape + (3,))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    return ax * rng.uniform(0, max_angle, shape + (1,))


def weights(F, hop):
    """(row_weight (F - hop,), joint_weight (55,), trans_weight): non-uniform rows, some joints at 0"""
    O = F - hop
    u = (0.25 + 0.75 * np.sin(np.pi * (np.arange(O) + 1.0) / (O + 1.0)) ** 2).astype(np.float32)
    w = (0.5 + 1.5 * ((np.arange(55) * 7) % 11) / 10.0).astype(np.float32)
    w[[1, 2, 4, 5, 20, 34]] = 0.0                       # four of the joints the NPZ writer freezes, and two of class 6 (20, 34)
    return u, w, 0.5


def make(F, hop, windows, frames, K, seed):
    """-> (poses (sum W K, F, 55, 3), trans (sum W K, F, 3)) float32"""
    rng = np.random.default_rng(seed)
    nw = sum(windows)
    poses = rand_aa(rng, (nw * K, F, 55), 3.6)
    O = F - hop
    cls = np.arange(55) % N_CLASSES
    g = 0
    for W in windows:
        for k in range(W - 1):
            R = rand_aa(rng, (O, 55), 3.0) + 1e-3          # (|R| stays away from 0, so the alias below is defined)
            th = np.linalg.norm(R, axis=-1, keepdims=True)
            alias = -(R / th) * (2 * np.pi - th)
            for c in range(K):
                a = poses[(g + k) * K + c, hop:hop + O]    # views: the assignments below write the batch
                b = poses[(g + k + 1) * K + c, :O]
                n = lambda s, sel: s * rng.standard_normal(R[:, sel].shape)
                a[:, cls == 1], b[:, cls == 1] = R[:, cls == 1], R[:, cls == 1]
                a[:, cls == 2], b[:, cls == 2] = R[:, cls == 2], R[:, cls == 2] + n(1e-4, cls == 2)
                a[:, cls == 3], b[:, cls == 3] = R[:, cls == 3] + n(1e-2, cls == 3), R[:, cls == 3] + n(1e-2, cls == 3)
                a[:, cls == 4], b[:, cls == 4] = R[:, cls == 4], alias[:, cls == 4]
                a[:, cls == 5] = 5e-7 * rng.uniform(-1, 1, R[:, cls == 5].shape)
                b[:, cls == 5] = 5e-7 * rng.uniform(-1, 1, R[:, cls == 5].shape)
                a[:, cls == 6] = 0.0 if c % 2 == 0 else 0.3 * rng.uniform(-1, 1, R[:, cls == 6].shape)
                b[:, cls == 6] = 0.0 if c % 3 == 0 else 0.3 * rng.uniform(-1, 1, R[:, cls == 6].shape)
        g += W
    trans = rng.standard_normal((nw * K, F, 3)) * np.array([1.0, 0.1, 30.0])
    return poses.astype(np.float32), trans.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs, both restatements of the angles, the float64 cost and the GPU bar of a case, computed once and shared (read-only)"""
    F, hop, windows, frames, K, with_trans = CASES[name]
    assert all((W - 1) * hop < L <= (W - 1) * hop + F for W, L in zip(windows, frames)), name
    poses, trans = make(F, hop, windows, frames, K, seed=sum(map(ord, name)))
    u, w, tw = weights(F, hop)
    if not with_trans:
        trans, tw = None, 0.0
    th64 = ref.thetas(poses, windows, frames, K, hop)
    th32 = ref.thetas(poses, windows, frames, K, hop, np.float32)
    f32_dist = max((float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(th32, th64)), default=0.0)
    delta = max(4.0 * f32_dist, 2.0 ** -20)
    cost64 = ref.cost(poses, trans, windows, frames, K, hop, u, w, tw)
    bar = ref.cost_bar(th64, delta, u, w, trans, tw, windows, frames, K, hop, F)
    out = dict(F=F, hop=hop, windows=windows, frames=frames, K=K, poses=poses, trans=trans, row_weight=u, joint_weight=w, trans_weight=tw, th64=th64,
               f32_dist=f32_dist, delta=delta, cost64=cost64, bar=bar)
    for v in out.values():
        for x in (v if isinstance(v, list) else [v]):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return out


def int_matrices():
    """small integer-valued cost matrices with ties: [(windows, K, cost (seams, K, K) float64), ...]"""
    rng = np.random.default_rng(11)
    out = []
    for windows, K in (((4,), 3), ((3, 1, 5), 2), ((2, 6), 3), ((5,), 4), ((1,), 5), ((3,), 1)):
        seams = sum(W - 1 for W in windows)
        out.append((windows, K, rng.integers(0, 3, (seams, K, K)).astype(np.float64)))       # values 0..2: many equal totals
    out.append(((4,), 3, np.zeros((3, 3, 3))))                                                # everything ties: candidate 0 throughout
    return out
