"""Synthetic SMPL-X-shaped body models and motions from a seed (the licensed assets are not needed to exercise the algorithm: linear blend skinning is generic in
the vertex count).  V = 203 by default: 812 padded outputs are ragged against every tile of the kernel."""
import numpy as np

import body_ref as br
from body_ref import matrix_to_rot6d, rodrigues

NJ = 55


def make_model(V=203, n_betas=300, seed=0, dense_rows=3):
    g = np.random.default_rng(seed)
    parents = np.zeros(NJ, np.int32)
    parents[0] = -1
    for j in range(1, NJ):
        parents[j] = j - 1 if j <= 11 else g.integers(0, j)      # joints 0..11: a chain 11 deep (SMPL-X's finger depth), then a random tree
    v_template = g.uniform(-0.9, 0.9, (V, 3)).astype(np.float32)
    shapedirs = (g.standard_normal((V, 3, n_betas)) * 2e-3).astype(np.float32)
    mag = 10.0 ** g.uniform(-7, -2, (486, V * 3))               # realistic scale: 1e-2 down to 1e-7
    posedirs = (mag * g.choice([-1.0, 1.0], mag.shape)).astype(np.float32)
    J_regressor = np.zeros((NJ, V), np.float32)
    for j in range(NJ):
        idx = g.choice(V, 8, replace=False)
        w = g.uniform(0.1, 1.0, 8)
        J_regressor[j, idx] = (w / w.sum()).astype(np.float32)
    weights = np.zeros((V, NJ), np.float32)
    for v in range(V):
        k = NJ if v < dense_rows else 1 + (v % 4)                # a few fully dense rows, then rows of 1 to 4 non-zeros
        idx = g.choice(NJ, k, replace=False)
        w = g.uniform(0.05, 1.0, k)
        weights[v, idx] = (w / w.sum()).astype(np.float32)
    return {"v_template": v_template, "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": J_regressor, "weights": weights, "parents": parents}


def make_betas(S=3, n_betas=300, seed=1):
    return (np.random.default_rng(seed).standard_normal((S, n_betas)) * 0.5).astype(np.float32)


def make_motion(N=3, F=5, seed=2):
    """Axis-angle poses [N,F,55,3] with zero vectors and angles beyond pi, translation [N,F,3]; the same rotations as 6D [N,F,55,6]."""
    g = np.random.default_rng(seed)
    aa = (g.standard_normal((N, F, NJ, 3)) * 0.4).astype(np.float32)
    aa[:, 0, 3] = 0.0                                            # zero vectors
    aa[0, :, 7] = 0.0
    big = g.standard_normal((N, F, 3))
    aa[:, :, 20] = (big / np.linalg.norm(big, axis=-1, keepdims=True) * g.uniform(3.3, 4.6, (N, F, 1))).astype(np.float32)   # beyond pi
    trans = (g.standard_normal((N, F, 3)) * 0.5).astype(np.float32)
    d6 = matrix_to_rot6d(rodrigues(aa.astype(np.float64))).astype(np.float32)
    return aa, trans, d6


def make_loss_sets(N=3, F=5, seed=3):
    """(ref, a, b), each (aa [N,F,55,3], trans [N,F,3], d6 [N,F,55,6]): candidates = the reference motion perturbed; clip 0 of `a` is translated by 1.5 m, so
    that SmoothL1's linear branch runs (every other difference stays in the quadratic branch)."""
    g = np.random.default_rng(seed)
    aa, trans, _ = make_motion(N, F, seed)
    sets = []
    for i in range(3):
        p = aa + (0.0 if i == 0 else 0.05 * i) * g.standard_normal(aa.shape).astype(np.float32)
        t = trans + (0.0 if i == 0 else 0.02 * i) * g.standard_normal(trans.shape).astype(np.float32)
        if i == 1:
            t[0] += np.float32(1.5)
        p, t = p.astype(np.float32), t.astype(np.float32)
        sets.append((p, t, matrix_to_rot6d(rodrigues(p.astype(np.float64))).astype(np.float32)))
    return sets


def feats_rows(d6, trans):
    """the project's feature rows [N,F,333] = 55 x 6D | translation"""
    return np.concatenate([d6.reshape(d6.shape[:2] + (330,)), trans], -1).astype(np.float32)


def motion_rows(aa, trans):
    """the trainer's ld_motion rows [N,F,168] = 55 x 3 axis-angle | translation"""
    return np.concatenate([aa.reshape(aa.shape[:2] + (165,)), trans], -1).astype(np.float32)


def forward_distances(model, betas, rot, trans, kind="aa"):
    """The distances that set the GPU bars, from the SAME inputs the GPU gets: max abs vertex (and joint) distance from the float64 restatement of the restatement run
    in float32 (d32), of the float32 restatement with the split-fp16 pose-blend product (dx; dx_noscale: without the packer's power-of-two pre-scale) and with the
    one-product fp16 form (d16).  Returns (float64 joints, float64 vertices, {name: distance})."""
    j64, v64 = br.forward(model, betas, rot, trans, kind)
    out = {}
    for name, blend in (("d32", None), ("dx", br.blend_split(True)), ("dx_noscale", br.blend_split(False)), ("d16", br.blend_f16)):
        j, v = br.forward(model, betas, rot, trans, kind, np.float32, blend)
        out[name] = float(np.abs(v - v64).max())
        out[name + "_joints"] = float(np.abs(j - j64).max())
    return j64, v64, out


def loss_distances(model, betas, sets, kind="aa", frames_per_pass=64, names=("r32", "rx", "r16")):
    """(float64 sums [2], {"r32" | "rx" | "r16": max relative distance of the two sums}) for loss sets as make_loss_sets returns them."""
    i = 0 if kind == "aa" else 2
    pick = [(s[i], s[1]) for s in sets]
    s64 = br.loss_sums(model, betas, *pick, kind, frames_per_pass=frames_per_pass)
    out = {}
    for name, blend in (("r32", None), ("rx", br.blend_split(True)), ("r16", br.blend_f16)):
        if name not in names:
            continue
        s = br.loss_sums(model, betas, *pick, kind, np.float32, blend, frames_per_pass)
        out[name] = max(abs(x - y) / y for x, y in zip(s, s64))
    return s64, out
