"""A numpy RESTATEMENT of motion smoothing (include/amuse_hip.h amuse_smooth_banks / amuse_smooth_motion), written from the header's text, not from the kernel.
`smooth(..., dtype=np.float64)` is the reference of the GPU tests; the SAME arithmetic in np.float32 tells how far fp32 rounding alone moves a result on a
test's own inputs, which sets the GPU bars (4 x that distance, at least 2^-20 rad: the stitch's and the body model's rule).  The axis-angle <-> quaternion steps
are the decode tail's, as tests/stitch_ref.py restates them."""
import numpy as np

from stitch_ref import aa_to_quat, geodesic, quat_to_aa, rotmat  # noqa: F401  (geodesic / rotmat: re-exported for the tests)

MAX_HALF, MAX_ORDER, SLOTS, BANK_FLOATS = 15, 5, 56, 5455


def bank_offset(m):
    return sum((2 * i + 1) ** 2 for i in range(1, m))


def hat(m, p):
    """H_m = A (A^T A)^-1 A^T in float64, A[i][d] = (i - m)^d, d = 0 .. min(p, 2 m).  Through the QR factorisation of A on the abscissae scaled to [-1, 1]:
    A = Q R gives H = Q Q^T, the same matrix, without squaring A's condition number."""
    assert 1 <= m <= MAX_HALF and 0 <= p <= MAX_ORDER
    pm = min(p, 2 * m)
    x = (np.arange(2 * m + 1, dtype=np.float64) - m) / m
    Q, _ = np.linalg.qr(np.vander(x, pm + 1, increasing=True))
    return Q @ Q.T


def hat_normal_equations(m, p):
    """the header's formula taken literally (float64): what `hat` must agree with where A^T A is still well conditioned"""
    pm = min(p, 2 * m)
    A = np.vander(np.arange(2 * m + 1, dtype=np.float64) - m, pm + 1, increasing=True)
    return A @ np.linalg.solve(A.T @ A, A.T)


def banks(order):
    """the fp32 bank as amuse_smooth_banks lays it out: H_1 .. H_15 back to back, (5455,) float32"""
    return np.concatenate([hat(m, order).astype(np.float32).ravel() for m in range(1, MAX_HALF + 1)])


def bank_of(bk, m):
    n = 2 * m + 1
    return np.asarray(bk[bank_offset(m):bank_offset(m) + n * n]).reshape(n, n)


def qmul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], -1)


def qconj(q):
    return q * np.array([1, -1, -1, -1], q.dtype)


def window_of(L, m):
    """-> (s, r) per frame: window start clamp(f - m, 0, L - 1 - 2 m) and bank row f - s"""
    f = np.arange(L)
    s = np.clip(f - m, 0, L - 1 - 2 * m)
    return s, f - s


def filter_rotations(aa, H, dtype=np.float64):
    """aa (L, J, 3) axis-angle of ONE sequence (the kernel's inputs are fp32; a float64 array is taken as it is), L >= 2 m + 1; H (2 m + 1, 2 m + 1) the fp32
    bank -> (L, J, 3) in dtype: the header's steps."""
    n = H.shape[0]
    m = (n - 1) // 2
    L = aa.shape[0]
    assert L >= n
    H = np.asarray(H, np.float32).astype(dtype)
    q = aa_to_quat(np.asarray(aa).astype(dtype), dtype)
    s, r = window_of(L, m)
    qc = q
    v = np.zeros(aa.shape, dtype)
    for k in range(n):
        d = qmul(qconj(qc), q[s + k]).astype(dtype)
        d = np.where(d[..., :1] < 0, -d, d)
        nv = np.sqrt((d[..., 1:] * d[..., 1:]).sum(-1, keepdims=True, dtype=dtype))
        small = nv < dtype(1e-6)
        fac = np.where(small, dtype(2.0), dtype(2.0) * np.arctan2(nv, d[..., :1]) / np.where(small, dtype(1.0), nv))
        v = v + (H[r, k][:, None, None] * fac) * d[..., 1:]
    out = qmul(qc, aa_to_quat(v.astype(dtype), dtype)).astype(dtype)
    out = out / np.sqrt((out * out).sum(-1, keepdims=True, dtype=dtype))
    out = np.where(out[..., :1] < 0, -out, out)
    return quat_to_aa(out.astype(dtype), dtype)


def filter_vectors(x, H, dtype=np.float64):
    """x (L, C) float32 of ONE sequence -> (L, C) in dtype: sum over k, in that order, of H[r][k] x[s + k]"""
    n = H.shape[0]
    m = (n - 1) // 2
    L = x.shape[0]
    assert L >= n
    H = np.asarray(H, np.float32).astype(dtype)
    x = np.asarray(x, np.float32).astype(dtype)
    s, r = window_of(L, m)
    out = np.zeros(x.shape, dtype)
    for k in range(n):
        out = out + H[r, k][:, None] * x[s + k]
    return out


def smooth(poses, trans, frames, half_window, bk, dtype=np.float64):
    """poses (sum L, 55, 3), trans (sum L, 3) or None, float32; half_window: 56 values; bk: the fp32 bank (5455,) -> (poses, trans or None, filtered (sum L, 56)
    bool) in dtype.  Slots with m = 0 and sequences shorter than 2 m + 1 keep the input's values (its fp32 bits, whatever dtype the filter runs in)."""
    poses = np.asarray(poses, np.float32)
    hw = [int(m) for m in half_window]
    assert len(hw) == SLOTS and all(0 <= m <= MAX_HALF for m in hw) and poses.shape == (sum(frames), 55, 3)
    po = poses.astype(dtype)
    to = None if trans is None else np.asarray(trans, np.float32).astype(dtype)
    mask = np.zeros((poses.shape[0], SLOTS), bool)
    f0 = 0
    for L in frames:
        assert L >= 1
        for m in sorted(set(hw)):
            if m == 0 or L < 2 * m + 1:
                continue
            H = bank_of(bk, m)
            js = [j for j in range(55) if hw[j] == m]
            if js:
                po[f0:f0 + L, js] = filter_rotations(poses[f0:f0 + L][:, js], H, dtype)
                mask[f0:f0 + L, js] = True
            if to is not None and hw[55] == m:
                to[f0:f0 + L] = filter_vectors(trans[f0:f0 + L], H, dtype)
                mask[f0:f0 + L, 55] = True
        f0 += L
    return po, to, mask
