"""The backward pass of SMPL-X linear blend skinning restated in numpy, in the order of operations of csrc/k_body_bwd.hip: the gradient of
S = sum SmoothL1(x_cand - x_ref) (beta 1) with respect to the candidate's 6D feature rows [N,F,333].  The reference motion gets no gradient.

  g_v    = clamp(x_cand - x_ref, -1, 1)                      translation columns: sum_v g_v
  dp_v   = T_v.R^T g_v                                        dpf = posedirs . dp   (the transposed pose-blend product, 486 values per frame)
  dA_j   = sum_v w_vj [g_v p_v^T | g_v]                       dG_j = [dA_j.R - dA_j.t J_j^T | dA_j.t]
  chain in reverse (parents[j] < j): dR_j += G_p.R^T dG_j.R;  dG_p.R += dG_j.R R_j^T + dG_j.t l_j^T;  dG_p.t += dG_j.t;  root: dR_0 += dG_0.R
  dR_1..54 += dpf;  Gram-Schmidt backward (a clamped norm, max(norm, 1e-12), passes no gradient)

Everything runs in `dtype`; `blend` replaces the forward pose-blend product (tests/body_ref.py) and `tblend` the transposed one (the emulations below), which
is how the distances that set the GPU bars are made.  Nothing here is pinned against the `smplx` package, which is absent: the oracle is the float64 autograd of
the differentiable torch twin (amuse_amd.body.torch_loss_sums(..., differentiable=True))."""
import numpy as np

import body_ref as br

NJ = 55
DP_SHIFT = 10   # csrc/amuse_body_bwd.hpp kBodyDpShift


def _gs_forward(d6, dtype):
    a1, a2 = d6[..., :3], d6[..., 3:]
    n1r = np.sqrt((a1 * a1).sum(-1, keepdims=True))
    n1 = np.maximum(n1r, dtype(1e-12))
    b1 = a1 / n1
    dt = (b1 * a2).sum(-1, keepdims=True)
    u = a2 - dt * b1
    n2r = np.sqrt((u * u).sum(-1, keepdims=True))
    n2 = np.maximum(n2r, dtype(1e-12))
    b2 = u / n2
    R = np.stack([b1, b2, np.cross(b1, b2)], -2).astype(dtype)
    return R, (a2, b1, b2, dt, n1r, n1, n2r, n2)


def _gs_backward(dR, cache, dtype):
    a2, b1, b2, dt, n1r, n1, n2r, n2 = cache
    d1, d2, d3 = dR[..., 0, :], dR[..., 1, :], dR[..., 2, :]
    d1 = d1 + np.cross(b2, d3)
    d2 = d2 + np.cross(d3, b1)
    k2 = np.where(n2r >= dtype(1e-12), (b2 * d2).sum(-1, keepdims=True), dtype(0))
    du = (d2 - b2 * k2) / n2
    ddt = -(b1 * du).sum(-1, keepdims=True)
    g2 = du + ddt * b1
    d1 = d1 - dt * du + ddt * a2
    k1 = np.where(n1r >= dtype(1e-12), (b1 * d1).sum(-1, keepdims=True), dtype(0))
    g1 = (d1 - b1 * k1) / n1
    return np.concatenate([g1, g2], -1).astype(dtype)


def tblend_split(dp, posedirs):
    """dpf = Ptl.dh + Pth.dl + Pth.dh with exact products: posedirs pre-scaled by 2^shift, dp by 2^DP_SHIFT, both cut into fp16 hi | lo"""
    s = br.posedirs_shift(posedirs)
    ph, pl = br._split(posedirs.astype(np.float32) * np.float32(2.0 ** s))
    dh, dl = br._split(np.asarray(dp, np.float32) * np.float32(2.0 ** DP_SHIFT))
    return (dh @ pl.T + dl @ ph.T + dh @ ph.T) * 2.0 ** -(s + DP_SHIFT)


def tblend_f16(dp, posedirs):
    s = br.posedirs_shift(posedirs)
    ph, _ = br._split(posedirs.astype(np.float32) * np.float32(2.0 ** s))
    dh, _ = br._split(np.asarray(dp, np.float32) * np.float32(2.0 ** DP_SHIFT))
    return (dh @ ph.T) * 2.0 ** -(s + DP_SHIFT)


def loss_grad(model, betas, ref_rows, rows, dtype=np.float64, blend=None, tblend=None):
    """betas [N,B] (one row per clip); ref_rows / rows: feature rows [N,F,333] -> (S, dS/d rows [N,F,333]) in `dtype`."""
    rows = np.asarray(rows, dtype)
    ref_rows = np.asarray(ref_rows, dtype)
    N, F = rows.shape[:2]
    V = model["v_template"].shape[0]
    parents = model["parents"]
    P, W = model["posedirs"].astype(dtype), model["weights"].astype(dtype)
    shaped = br.shape(model, betas, dtype)
    vs, J = shaped
    x_ref = br.forward(model, betas, ref_rows[..., :330].reshape(N, F, NJ, 6), ref_rows[..., 330:], "6d", dtype, blend, shaped)[1]
    # the candidate's forward pass, with what the way back needs
    R, cache = _gs_forward(rows[..., :330].reshape(N, F, NJ, 6), dtype)
    pf = (R[:, :, 1:] - np.eye(3, dtype=dtype)).reshape(N * F, 486)
    off = (pf @ P) if blend is None else blend(pf, model["posedirs"]).astype(dtype)
    vp = vs[:, None] + off.reshape(N, F, V, 3)
    GR, Gt = br.chain(R, J[:, None], parents, dtype)
    At = Gt - (GR @ np.broadcast_to(J[:, None, :, :, None], (N, F, NJ, 3, 1)))[..., 0]
    A = np.concatenate([GR, At[..., None]], -1).reshape(N, F, NJ, 12)
    T = (W @ A.transpose(2, 0, 1, 3).reshape(NJ, N * F * 12)).reshape(V, N, F, 3, 4).transpose(1, 2, 0, 3, 4)
    x = ((T[..., :3] * vp[..., None, :]).sum(-1) + T[..., 3] + rows[:, :, None, 330:]).astype(dtype)
    d = x - x_ref
    ad = np.abs(d.astype(np.float64))
    S = float(np.where(ad < 1.0, 0.5 * ad * ad, ad - 0.5).sum())
    # ---- backward
    g = np.clip(d, dtype(-1), dtype(1)).astype(dtype)                            # [N,F,V,3]
    grad = np.zeros((N, F, 333), dtype)
    grad[..., 330:] = g.sum(2)
    dp = (T[..., :3] * g[..., :, None]).sum(-2).astype(dtype)                    # T.R^T g
    dpf = (dp.reshape(N * F, V * 3) @ P.T) if tblend is None else tblend(dp.reshape(N * F, V * 3), model["posedirs"])
    dpf = np.asarray(dpf, dtype).reshape(N, F, 54, 3, 3)
    M = np.concatenate([g[..., :, None] * vp[..., None, :], g[..., None]], -1).reshape(N, F, V, 12).astype(dtype)
    dA = (W.T @ M.transpose(2, 0, 1, 3).reshape(V, N * F * 12)).reshape(NJ, N, F, 3, 4).transpose(1, 2, 0, 3, 4).astype(dtype)
    dGR = (dA[..., :3] - dA[..., 3:4] * J[:, None, :, None, :]).astype(dtype)    # dA.R - dA.t J^T
    dGt = dA[..., 3].copy()
    dGR = [dGR[:, :, j] for j in range(NJ)]
    dGt = [dGt[:, :, j] for j in range(NJ)]
    dR = [None] * NJ
    for j in range(NJ - 1, 0, -1):
        p = int(parents[j])
        l = (J[:, j] - J[:, p])[:, None]                                          # [N,1,3]
        dR[j] = np.swapaxes(GR[:, :, p], -1, -2) @ dGR[j]
        dGR[p] = dGR[p] + dGR[j] @ np.swapaxes(R[:, :, j], -1, -2) + dGt[j][..., :, None] * l[..., None, :]
        dGt[p] = dGt[p] + dGt[j]
    dR[0] = dGR[0]
    dR = np.stack(dR, 2).astype(dtype)
    dR[:, :, 1:] += dpf
    grad[..., :330] = _gs_backward(dR, cache, dtype).reshape(N, F, 330)
    return S, grad
