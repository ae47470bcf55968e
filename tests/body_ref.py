"""The SMPL-X body model restated in numpy (no `smplx` package exists here: this is a RESTATEMENT of the published algorithm, not a pin; the known answers in
tests/test_body_cases_cpu.py are what stands behind it).  What the reference's LatentPriorLosses._get_vertices gets from SMPLX(num_betas=300, use_pca=False,
flat_hand_mean=True) with expression = 0, per frame:

  1. v_shaped = v_template + shapedirs . betas
  2. J = J_regressor . v_shaped                                       [55][3]
  3. R_j = Rodrigues(pose_j), angle = |pose_j + 1e-8|                 (a zero vector gives the identity)
  4. pose_feature = (R_1..R_54 - I) row-major [486]; v_posed = v_shaped + pose_feature . posedirs
  5. the kinematic chain: G_j = G_parent . [R_j | J_j - J_parent]; posed joint = G_j.t; A_j = [G_j.R | G_j.t - G_j.R J_j]
  6. vertex_v = (sum_j w[v][j] A_j) . [v_posed_v; 1] + transl
  7. SmoothL1(beta 1) over all N F V 3 coordinates

A model is a dict: v_template [V,3], shapedirs [V,3,B], posedirs [486,V*3], J_regressor [55,V], weights [V,55], parents [55] (parents[0] = -1).
Everything runs in `dtype` (float64: the reference; float32: the distance that sets the GPU bars); `blend` replaces the pose-blend product of step 4
(the split-fp16 emulations below)."""
import numpy as np

NJ = 55


def rodrigues(rv, dtype=np.float64):
    rv = np.asarray(rv, dtype=dtype)
    angle = np.sqrt(((rv + dtype(1e-8)) ** 2).sum(-1, keepdims=True)).astype(dtype)
    d = rv / angle
    c, s = np.cos(angle)[..., None].astype(dtype), np.sin(angle)[..., None].astype(dtype)
    rx, ry, rz = d[..., 0], d[..., 1], d[..., 2]
    z = np.zeros_like(rx)
    K = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], -1).reshape(rv.shape[:-1] + (3, 3))
    eye = np.eye(3, dtype=dtype)
    return (eye + s * K + (dtype(1) - c) * (K @ K)).astype(dtype)


def rot6d_to_matrix(d6, dtype=np.float64):
    """rotation_6d_to_matrix (pytorch3d): Gram-Schmidt of the two 3-vectors, rows b1, b2, b1 x b2."""
    d6 = np.asarray(d6, dtype=dtype)
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(-1, keepdims=True)), dtype(1e-12))
    b2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = b2 / np.maximum(np.sqrt((b2 * b2).sum(-1, keepdims=True)), dtype(1e-12))
    return np.stack([b1, b2, np.cross(b1, b2)], -2).astype(dtype)


def matrix_to_rot6d(R):
    return R[..., :2, :].reshape(R.shape[:-2] + (6,))


def shape(model, betas, dtype=np.float64):
    """betas [N,B] -> v_shaped [N,V,3], J [N,55,3]."""
    b = np.asarray(betas, dtype)
    v = model["v_template"].astype(dtype)[None] + np.einsum("vcb,nb->nvc", model["shapedirs"].astype(dtype), b)
    return v, np.einsum("jv,nvc->njc", model["J_regressor"].astype(dtype), v)


def chain(R, J, parents, dtype=np.float64):
    """R [...,55,3,3], J [...,55,3] (broadcastable) -> G rotation [...,55,3,3], G translation [...,55,3]."""
    GR, Gt = [None] * NJ, [None] * NJ
    for j in range(NJ):
        p = int(parents[j])
        if p < 0:
            GR[j], Gt[j] = R[..., j, :, :], np.broadcast_to(J[..., j, :], R.shape[:-3] + (3,)).astype(dtype)
        else:
            GR[j] = GR[p] @ R[..., j, :, :]
            Gt[j] = (GR[p] @ (J[..., j, :] - J[..., p, :])[..., None])[..., 0] + Gt[p]
    return np.stack(GR, -3), np.stack(Gt, -2)


def forward(model, betas, rot, trans=None, kind="aa", dtype=np.float64, blend=None, shaped=None):
    """betas [N,B]; rot [N,F,55,3] axis-angle or [N,F,55,6] 6D; trans [N,F,3] or None -> joints [N,F,55,3], vertices [N,F,V,3] (einsum form)."""
    rot = np.asarray(rot, dtype)
    N, F = rot.shape[:2]
    V = model["v_template"].shape[0]
    tr = np.zeros((N, F, 3), dtype) if trans is None else np.asarray(trans, dtype)
    vs, J = shape(model, betas, dtype) if shaped is None else shaped   # (shaped: shape()'s result, for callers that pass many frame chunks)
    R = rodrigues(rot, dtype) if kind == "aa" else rot6d_to_matrix(rot, dtype)
    pf = (R[:, :, 1:] - np.eye(3, dtype=dtype)).reshape(N * F, 486)
    off = (pf @ model["posedirs"].astype(dtype)) if blend is None else blend(pf, model["posedirs"]).astype(dtype)
    vp = vs[:, None] + off.reshape(N, F, V, 3)
    GR, Gt = chain(R, J[:, None], model["parents"], dtype)
    joints = Gt + tr[:, :, None]
    At = Gt - (GR @ np.broadcast_to(J[:, None, :, :, None], (N, F, NJ, 3, 1)))[..., 0]
    A = np.concatenate([GR, At[..., None]], -1).reshape(N, F, NJ, 12)
    T = (model["weights"].astype(dtype) @ A.transpose(2, 0, 1, 3).reshape(NJ, N * F * 12)).reshape(V, N, F, 3, 4).transpose(1, 2, 0, 3, 4)   # sum_j w[v][j] A_j
    verts = (T[..., :3] * vp[..., None, :]).sum(-1) + T[..., 3] + tr[:, :, None]
    return joints.astype(dtype), verts.astype(dtype)


def forward_loop(model, betas, rot, trans=None, kind="aa"):
    """The same in float64, one frame and one vertex at a time (the definition, spelled out)."""
    N, F = rot.shape[:2]
    V = model["v_template"].shape[0]
    W, P, par = model["weights"].astype(np.float64), model["posedirs"].astype(np.float64), model["parents"]
    joints, verts = np.zeros((N, F, NJ, 3)), np.zeros((N, F, V, 3))
    for n in range(N):
        vs = model["v_template"].astype(np.float64) + model["shapedirs"].astype(np.float64) @ np.asarray(betas[n], np.float64)
        J = model["J_regressor"].astype(np.float64) @ vs
        for f in range(F):
            t = np.zeros(3) if trans is None else np.asarray(trans[n, f], np.float64)
            R = [rodrigues(rot[n, f, j]) if kind == "aa" else rot6d_to_matrix(rot[n, f, j]) for j in range(NJ)]
            pf = np.concatenate([(R[j] - np.eye(3)).reshape(9) for j in range(1, NJ)])
            vp = vs + (pf @ P).reshape(V, 3)
            G = [None] * NJ
            for j in range(NJ):
                L = np.eye(4)
                L[:3, :3], L[:3, 3] = R[j], J[j] - (J[par[j]] if par[j] >= 0 else 0.0)
                G[j] = L if par[j] < 0 else G[par[j]] @ L
            A = []
            for j in range(NJ):
                joints[n, f, j] = G[j][:3, 3] + t
                Aj = G[j].copy()
                Aj[:3, 3] = G[j][:3, 3] - G[j][:3, :3] @ J[j]
                A.append(Aj)
            for v in range(V):
                T = sum(W[v, j] * A[j] for j in range(NJ) if W[v, j] != 0.0)
                verts[n, f, v] = T[:3, :3] @ vp[v] + T[:3, 3] + t
    return joints, verts


def smooth_l1_sum(a, ref):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64))
    return float(np.where(d < 1.0, 0.5 * d * d, d - 0.5).sum())


# ------------------------------------------------------------------ the split-fp16 pose-blend product (csrc/amuse_body_pack.hpp, k_body.hip)
def posedirs_shift(posedirs):
    m = float(np.abs(posedirs).max())
    if not m > 0:
        return 0
    return int(min(max(14 - np.frexp(np.float32(m))[1], 0), 24))


def _split(x):
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def blend_split(prescale=True):
    """Pl.fh + Ph.fl + Ph.fh with exact products (fp32 accumulation on the GPU is part of what the bar's factor covers); posedirs pre-scaled by 2^shift or not."""
    def f(pf, posedirs):
        s = posedirs_shift(posedirs) if prescale else 0
        ph, pl = _split(posedirs.astype(np.float32) * np.float32(2.0 ** s))
        fh, fl = _split(pf)
        return (fh @ pl + fl @ ph + fh @ ph) * 2.0 ** -s
    return f


def blend_f16(pf, posedirs):
    s = posedirs_shift(posedirs)
    ph, _ = _split(posedirs.astype(np.float32) * np.float32(2.0 ** s))
    fh, _ = _split(pf)
    return (fh @ ph) * 2.0 ** -s


def loss_sums(model, betas, ref, a, b, kind, dtype=np.float64, blend=None, frames_per_pass=64):
    """SmoothL1 sums of (a, ref) and (b, ref) over the vertices, frame chunks at a time (a full-size model never holds all its vertices).
    ref / a / b: (rot [N,F,55,3|6], trans [N,F,3])."""
    N, F = ref[0].shape[:2]
    out = [0.0, 0.0]
    model = dict(model, posedirs=model["posedirs"].astype(dtype), weights=model["weights"].astype(dtype))
    shaped = shape(model, betas, dtype)
    for f0 in range(0, F, frames_per_pass):
        sl = slice(f0, min(F, f0 + frames_per_pass))
        vr = forward(model, betas, ref[0][:, sl], ref[1][:, sl], kind, dtype, blend, shaped)[1]
        for i, c in enumerate((a, b)):
            if c is not None:
                out[i] += smooth_l1_sum(forward(model, betas, c[0][:, sl], c[1][:, sl], kind, dtype, blend, shaped)[1], vr)
    return out
