"""A numpy RESTATEMENT of the long-form candidates' seam cost, best path and gather (include/amuse_hip.h amuse_seam_plan / amuse_seam_cost / amuse_seam_path /
amuse_seam_select), written from the header's text, not from the kernels.  `thetas(..., dtype=np.float64)` / `cost(...)` are the reference of the GPU tests; the
SAME angle arithmetic in np.float32 tells how far fp32 rounding alone moves an angle on a test's own inputs, which sets the GPU bars (4 x that distance, at least
2^-20 rad: the project's rule).  `best_path` is the header's dynamic programme with its association ((best + cost), summed from window 0) and its tie rule
(replace on `<` only, from (+inf, 0)), so its choices and totals are what the kernel must give BIT FOR BIT."""
import itertools

import numpy as np

from stitch_ref import aa_to_quat


def plan(windows, K, F, hop):
    """-> (seams, workspace bytes)"""
    seams = sum(W - 1 for W in windows)
    return seams, seams * 2 * K * (F - hop) * 55 * 16


def overlap_rows(F, hop, L, k):
    """O_k: the overlap rows of seam k that reach the output"""
    return min(F - hop, L - (k + 1) * hop)


def quat_conj_mul(a, b):
    """conj(a) b, (..., 4) in (w, x, y, z)"""
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw + ax * bx + ay * by + az * bz,
                     aw * bx - ax * bw - ay * bz + az * by,
                     aw * by + ax * bz - ay * bw - az * bx,
                     aw * bz - ax * by + ay * bx - az * bw], -1)


def angle(a, b, dtype=np.float64):
    """a, b (..., 3) axis-angle -> (...) the header's theta: 2 atan2(|r.xyz|, |r.w|) of r = conj(q_a) q_b, every step in `dtype`"""
    r = quat_conj_mul(aa_to_quat(a, dtype), aa_to_quat(b, dtype)).astype(dtype)
    n = np.sqrt((r[..., 1:] * r[..., 1:]).sum(-1, dtype=dtype))
    return (dtype(2.0) * np.arctan2(n, np.abs(r[..., 0]))).astype(dtype)


def seams_of(windows, frames, F, hop):
    """[(global window g of the seam's first window, O_k), ...] in cost_out's order"""
    out, g = [], 0
    for W, L in zip(windows, frames):
        assert W >= 1 and (W - 1) * hop < L <= (W - 1) * hop + F
        out += [(g + k, overlap_rows(F, hop, L, k)) for k in range(W - 1)]
        g += W
    return out


def thetas(poses, windows, frames, K, hop, dtype=np.float64):
    """poses (sum W K, F, 55, 3) -> a list, per seam, of theta (K, K, O_k, 55): [a][b][i][j] between candidate a of the seam's first window, row i + hop, and
    candidate b of the next window, row i"""
    poses = np.asarray(poses, np.float32)
    F = poses.shape[1]
    out = []
    for g, Ok in seams_of(windows, frames, F, hop):
        a = poses[g * K:(g + 1) * K, hop:hop + Ok]
        b = poses[(g + 1) * K:(g + 2) * K, :Ok]
        out.append(angle(a[:, None], b[None, :], dtype))
    return out


def trans_sq(trans, windows, frames, K, hop, F):
    """per seam (K, K, O_k, 3): the fp32 differences t_a(i + hop) - t_b(i), as float64"""
    trans = np.asarray(trans, np.float32)
    out = []
    for g, Ok in seams_of(windows, frames, F, hop):
        out.append((trans[g * K:(g + 1) * K, None, hop:hop + Ok] - trans[None, (g + 1) * K:(g + 2) * K, :Ok]).astype(np.float64))
    return out


def cost(poses, trans, windows, frames, K, hop, row_weight, joint_weight, trans_weight, dtype=np.float64):
    """-> (seams, K, K) float64.  The angles in `dtype`; squares, weights and sums in float64 (the header's split)."""
    poses = np.asarray(poses, np.float32)
    F = poses.shape[1]
    u, w = np.asarray(row_weight, np.float32).astype(np.float64), np.asarray(joint_weight, np.float32).astype(np.float64)
    th = thetas(poses, windows, frames, K, hop, dtype)
    dt = trans_sq(trans, windows, frames, K, hop, F) if trans is not None else None
    out = np.zeros((len(th), K, K))
    for s, t in enumerate(th):
        Ok = t.shape[2]
        rows = (t.astype(np.float64) ** 2 * w).sum(-1)
        if dt is not None:
            rows = rows + float(np.float32(trans_weight)) * (dt[s] ** 2).sum(-1)
        out[s] = (rows * u[:Ok]).sum(-1)
    return out


def cost_bar(th64, delta, row_weight, joint_weight, trans=None, trans_weight=0.0, windows=None, frames=None, K=None, hop=None, F=None):
    """the GPU bar per pair, (seams, K, K): sum_i u_i sum_j w_j (2 theta64 delta + delta^2), plus the translation term with every component of the difference
    allowed 4 ulp (fp32) of the larger input"""
    u, w = np.asarray(row_weight, np.float32).astype(np.float64), np.asarray(joint_weight, np.float32).astype(np.float64)
    out = np.zeros((len(th64), K, K))
    for s, t in enumerate(th64):
        out[s] = (((2.0 * t * delta + delta * delta) * w).sum(-1) * u[:t.shape[2]]).sum(-1)
    if trans is not None and trans_weight:
        trans = np.asarray(trans, np.float32)
        dt = trans_sq(trans, windows, frames, K, hop, F)
        for s, (g, Ok) in enumerate(seams_of(windows, frames, F, hop)):
            big = np.maximum(np.abs(trans[g * K:(g + 1) * K, None, hop:hop + Ok]), np.abs(trans[None, (g + 1) * K:(g + 2) * K, :Ok]))
            e = 4.0 * np.spacing(big).astype(np.float64)
            out[s] += float(np.float32(trans_weight)) * ((2.0 * np.abs(dt[s]) * e + e * e).sum(-1) * u[:Ok]).sum(-1)
    return out


def best_path(cost_matrix, windows, K):
    """-> (choice (sum W,) int: the batch row g K + c of every window, total (S,) float64).  The header's rule, candidate by candidate."""
    m = np.asarray(cost_matrix, np.float64).reshape(-1, K, K)
    choice, total = [], []
    s0 = g0 = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for W in windows:
            best, back = np.zeros(K), []
            for k in range(1, W):
                nb, arg = np.full(K, np.inf), np.zeros(K, int)
                for a in range(K):
                    v = best[a] + m[s0 + k - 1, a]
                    v = np.where(np.isfinite(v), v, np.inf)
                    upd = v < nb
                    nb[upd], arg[upd] = v[upd], a
                back.append(arg)
                best = nb
            tot, c = np.inf, 0
            for b in range(K):
                if best[b] < tot:
                    tot, c = best[b], b
            total.append(0.0 if W == 1 else tot)
            cs = [c]
            for k in range(W - 1, 0, -1):
                c = int(back[k - 1][c])
                cs.append(c)
            choice += [(g0 + k) * K + c for k, c in enumerate(reversed(cs))]
            s0, g0 = s0 + W - 1, g0 + W
    return np.array(choice, np.int32), np.array(total, np.float64)


def path_total(cost_matrix, K, seam0, cands):
    """the total of ONE path of a sequence (candidates per window), summed as the dynamic programme sums it: ((0 + c_0) + c_1) + ..."""
    m = np.asarray(cost_matrix, np.float64).reshape(-1, K, K)
    t = 0.0
    for k in range(1, len(cands)):
        t = t + m[seam0 + k - 1, cands[k - 1], cands[k]]
    return t


def brute_force(cost_matrix, W, K, seam0=0):
    """every one of the K^W paths of one sequence (finite matrices only) -> (candidates, total) of the winner: the least total; among equals the path that is
    lexicographically least read from its END - what `<`-only replacement from the last window backwards selects when the sums are exact"""
    best = None
    for p in itertools.product(range(K), repeat=W):
        key = (path_total(cost_matrix, K, seam0, p), p[::-1])
        if best is None or key < best:
            best = key
    return list(best[1][::-1]), best[0]


def select(poses, trans, choice):
    poses = np.asarray(poses, np.float32)
    return poses[choice], (None if trans is None else np.asarray(trans, np.float32)[choice])
