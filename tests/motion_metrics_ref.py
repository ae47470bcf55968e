"""Plain numpy float64 restatement of the motion metrics (include/amuse_hip.h amuse_motion_metrics; amuse_amd/motion_metrics.py): the per-clip row, the two
compute()s and the Frechet distance.  Written from the definitions, not from the product code: the row is built block by block with its own offsets."""
import numpy as np

NJ = 55
ROW = 442
# (block, offset, length): the table of include/amuse_hip.h, typed out a second time
BLOCKS = (("ape_root", 0, 1), ("ape_traj", 1, 1), ("ape_pose", 2, 54), ("ape_joints", 56, 55), ("ave_root", 111, 1), ("ave_traj", 112, 1),
          ("ave_pose", 113, 54), ("ave_joints", 167, 55), ("vel_gen", 222, 55), ("vel_ref", 277, 55), ("acc_gen", 332, 55), ("acc_ref", 387, 55))
SL = {k: slice(o, o + n) for k, o, n in BLOCKS}


def variance(x, T):
    """MLD's variance(x, T, dim=0), as recollected: two-pass, over the first axis, divided by T - 1"""
    mean = x.mean(0)
    return ((x - mean) ** 2).sum(0) / (T - 1)


def l2(a, b, axis):
    return np.sqrt(((a - b) ** 2).sum(axis))


def clip_row(G, R, L, F=None):
    """G, R [F, 55, 3] (any float dtype; converted to float64 first, as the kernel converts its fp32 loads), L frames -> [442]; NaN when L is outside 2..F"""
    F = G.shape[0] if F is None else F
    row = np.full(ROW, np.nan)
    if L < 2 or L > F:
        return row
    G, R = np.asarray(G[:L], np.float64), np.asarray(R[:L], np.float64)
    rg, rr = G[:, 0], R[:, 0]
    tg, tr = rg[:, [0, 2]], rr[:, [0, 2]]
    lg, lr = G[:, 1:] - rg[:, None], R[:, 1:] - rr[:, None]
    row[SL["ape_root"]] = l2(rg, rr, 1).sum()
    row[SL["ape_traj"]] = l2(tg, tr, 1).sum()
    row[SL["ape_pose"]] = l2(lg, lr, 2).sum(0)
    row[SL["ape_joints"]] = l2(G, R, 2).sum(0)
    row[SL["ave_root"]] = l2(variance(rg, L), variance(rr, L), 0)
    row[SL["ave_traj"]] = l2(variance(tg, L), variance(tr, L), 0)
    row[SL["ave_pose"]] = l2(variance(lg, L), variance(lr, L), 1)
    row[SL["ave_joints"]] = l2(variance(G, L), variance(R, L), 1)
    for tag, X in (("gen", G), ("ref", R)):
        row[SL[f"vel_{tag}"]] = np.sqrt(((X[1:] - X[:-1]) ** 2).sum(2)).sum(0)
        row[SL[f"acc_{tag}"]] = np.sqrt(((X[2:] - 2 * X[1:-1] + X[:-2]) ** 2).sum(2)).sum(0)
    return row


def rows(G, R, lengths):
    """[N, F, 55, 3] x 2, lengths [N] -> [N, 442]"""
    return np.stack([clip_row(G[n], R[n], int(lengths[n]), G.shape[1]) for n in range(len(lengths))])


def joint_compute(rows_, lengths, fps=30.0):
    """val_metrics.py:63-92 written out: APE over the frames counted, AVE over the clips counted; velocity / acceleration per second, over the differences counted"""
    rows_, lengths = np.asarray(rows_, np.float64), np.asarray(lengths)
    s = rows_.sum(0)
    count, count_seq = int(lengths.sum()), len(lengths)
    out = {"APE_root": s[0] / count, "APE_traj": s[1] / count, "APE_mean_pose": s[2:56].mean() / count, "APE_mean_joints": s[56:111].mean() / count,
           "AVE_root": s[111] / count_seq, "AVE_traj": s[112] / count_seq, "AVE_mean_pose": s[113:167].mean() / count_seq,
           "AVE_mean_joints": s[167:222].mean() / count_seq}
    nv, na = (lengths - 1).sum(), (lengths - 2).sum()
    out["vel_gen"], out["vel_ref"] = s[222:277].mean() * fps / nv, s[277:332].mean() * fps / nv
    out["acc_gen"], out["acc_ref"] = s[332:387].mean() * fps ** 2 / na, s[387:442].mean() * fps ** 2 / na
    return out


def frechet_sqrtm(mu1, cov1, mu2, cov2):
    """the standard formula in scipy.linalg.sqrtm's form (tests only): |mu1 - mu2|^2 + tr C1 + tr C2 - 2 tr sqrtm(C1 C2), the real part taken"""
    from scipy import linalg
    covmean = linalg.sqrtm(cov1 @ cov2)
    if isinstance(covmean, tuple):
        covmean = covmean[0]
    covmean = np.real(covmean)
    d = mu1 - mu2
    return float(d @ d + np.trace(cov1) + np.trace(cov2) - 2 * np.trace(covmean))


def frechet_eig(mu1, cov1, mu2, cov2):
    """the same trace from the eigenvalues of C1 C2 itself (non-symmetric, real non-negative spectrum): a second route that needs no matrix square root"""
    ev = np.linalg.eigvals(cov1 @ cov2)
    d = mu1 - mu2
    return float(d @ d + np.trace(cov1) + np.trace(cov2) - 2 * np.sqrt(np.clip(ev.real, 0, None)).sum())
