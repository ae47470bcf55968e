"""A numpy RESTATEMENT of long-form inference's window plan, crossfade weights and join (include/amuse_hip.h amuse_longform_plan / amuse_stitch_windows),
written from the header's text, not from the kernel.  `join(..., dtype=np.float64)` is the reference of the GPU tests; the SAME arithmetic in np.float32 tells
how far fp32 rounding alone moves a result on a test's own inputs, which sets the GPU bars (4 x that distance, at least 2^-20 rad: the body model's rule)."""
import numpy as np

F_CLIP, N_CLIP = 300, 160000


def plan(n, h):
    """-> (W, L, hop_samples)"""
    assert n >= 0 and h % 3 == 0 and 150 <= h <= 300
    L = max(F_CLIP, (3 * n) // 1600)
    W = 1 if L <= F_CLIP else -(-(L - F_CLIP) // h) + 1
    return W, L, h // 3 * 1600


def window_slices(n, h):
    W, _, hs = plan(n, h)
    return [(w * hs, min(w * hs + N_CLIP, n)) for w in range(W)]


def blend_weights(O):
    i = np.arange(O, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 1.0) / (O + 1.0))).astype(np.float32)


def aa_to_quat(aa, dtype=np.float64):
    aa = np.asarray(aa, dtype)
    ang = np.sqrt((aa * aa).sum(-1, keepdims=True, dtype=dtype))
    half = dtype(0.5) * ang
    small = ang < dtype(1e-6)
    s = np.where(small, dtype(0.5) - ang * ang / dtype(48.0), np.sin(half) / np.where(small, dtype(1.0), ang))
    return np.concatenate([np.cos(half), aa * s], -1).astype(dtype)


def quat_to_aa(q, dtype=np.float64):
    q = np.asarray(q, dtype)
    nrm = np.sqrt((q[..., 1:] * q[..., 1:]).sum(-1, keepdims=True, dtype=dtype))
    half = np.arctan2(nrm, q[..., :1])
    ang = dtype(2.0) * half
    small = np.abs(ang) < dtype(1e-6)
    s = np.where(small, dtype(0.5) - ang * ang / dtype(48.0), np.sin(half) / np.where(small, dtype(1.0), ang))
    return (q[..., 1:] / s).astype(dtype)


def blend_joints(a, b, w, dtype=np.float64):
    """a, b (..., 3) axis-angle, w broadcastable to (..., 1) -> (..., 3): the header's six steps."""
    qa, qb = aa_to_quat(a, dtype), aa_to_quat(b, dtype)
    w = np.asarray(w, dtype)
    d = (qa * qb).sum(-1, keepdims=True, dtype=dtype)
    neg = d < 0
    qb, d = np.where(neg, -qb, qb), np.where(neg, -d, d)
    r = qb - d * qa
    omega = np.arctan2(np.sqrt((r * r).sum(-1, keepdims=True, dtype=dtype)), d)
    so = np.sin(omega)
    lin = so < dtype(1e-4)
    den = np.where(lin, dtype(1.0), so)
    ca = np.where(lin, dtype(1.0) - w, np.sin((dtype(1.0) - w) * omega) / den)
    cb = np.where(lin, w, np.sin(w * omega) / den)
    q = ca * qa + cb * qb
    q = q / np.sqrt((q * q).sum(-1, keepdims=True, dtype=dtype))
    q = np.where(q[..., :1] < 0, -q, q)
    return quat_to_aa(q.astype(dtype), dtype)


def join(poses, trans, windows, frames, hop, blend, dtype=np.float64):
    """poses (sum W, F, 55, 3), trans (sum W, F, 3) or None -> (poses (sum L, 55, 3), trans (sum L, 3) or None, blended (sum L,) bool).  Frames outside the
    overlaps are copies of the input rows (their fp32 bits, whatever dtype the blend runs in)."""
    poses = np.asarray(poses, np.float32)
    F = poses.shape[1]
    O = F - hop
    blend = np.asarray(blend, np.float32)
    assert blend.shape == (O,)
    po, to, mask = [], [], []
    w0 = 0
    for W, L in zip(windows, frames):
        assert W >= 1 and (W - 1) * hop < L <= (W - 1) * hop + F
        for f in range(L):
            k = min(f // hop, W - 1)
            i = f - k * hop
            if k == 0 or i >= O:
                po.append(poses[w0 + k, i].astype(dtype))
                if trans is not None:
                    to.append(np.asarray(trans[w0 + k, i], np.float32).astype(dtype))
                mask.append(False)
            else:
                w = dtype(blend[i])
                po.append(blend_joints(poses[w0 + k - 1, i + hop], poses[w0 + k, i], w, dtype))
                if trans is not None:
                    ta, tb = (np.asarray(trans[w0 + q, r], np.float32).astype(dtype) for q, r in ((k - 1, i + hop), (k, i)))
                    to.append((dtype(1.0) - w) * ta + w * tb)
                mask.append(True)
        w0 += W
    return np.stack(po), (np.stack(to) if trans is not None else None), np.array(mask)


def rotmat(aa):
    """float64 Rodrigues, (..., 3) -> (..., 3, 3)"""
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa, axis=-1)[..., None, None]
    k = aa / np.where(th[..., 0] < 1e-300, 1.0, th[..., 0])
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def geodesic(aa1, aa2):
    """the angle of R1^T R2, per joint (float64; atan2 form, good near 0 and near pi)"""
    R = np.swapaxes(rotmat(aa1), -1, -2) @ rotmat(aa2)
    sk = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    return np.arctan2(0.5 * np.linalg.norm(sk, axis=-1), 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0))
