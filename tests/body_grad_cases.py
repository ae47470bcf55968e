"""Cases and bars of the body model's gradient tests: the float64 oracle (autograd of the differentiable torch twin) and the distances of the emulations of
tests/body_grad_ref.py from it, which set the GPU bars - computed from the same inputs the GPU gets, never from its output."""
import numpy as np
import torch

import body_cases as bc
import body_grad_ref as bg
import body_ref as br
from amuse_amd import body as body_mod

FLOOR = 2.0 ** -20


def rows_of(sets):
    """make_loss_sets -> feature rows [N,F,333] of (ref, a, b)"""
    return [bc.feats_rows(s[2], s[1]) for s in sets]


def oracle(model, betas, ref, a, b=None, subject=None):
    """float64 autograd of the twin: (sums [2], grad_a, grad_b | None) as numpy float64; betas [S,B], subject [N] (default n % S)"""
    bm = body_mod.BodyModel.from_dict(model)
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    ta, tb = t(a).requires_grad_(True), (t(b).requires_grad_(True) if b is not None else None)
    s = body_mod.torch_loss_sums(bm, betas, t(ref), ta, tb, subject=subject, kind="6d", differentiable=True)
    s.sum().backward()
    return s.detach().numpy(), ta.grad.numpy(), (tb.grad.numpy() if b is not None else None)


def clip_betas(betas, N, subject=None):
    sub = np.arange(N) % betas.shape[0] if subject is None else np.asarray(subject)
    return betas[sub]


def rel(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / np.abs(ref).max())


def grad_distances(model, betas, ref, cand, g64, subject=None):
    """{"d32" | "dx" | "d16": distance of the emulation's gradient from g64, relative to max|g64|}"""
    cb = clip_betas(betas, ref.shape[0], subject)
    out = {}
    for name, blend, tblend in (("d32", None, None), ("dx", br.blend_split(True), bg.tblend_split), ("d16", br.blend_f16, bg.tblend_f16)):
        out[name] = rel(bg.loss_grad(model, cb, ref, cand, np.float32, blend, tblend)[1], g64)
    return out


def bars(d):
    """4 x the emulation's distance, floored at 2^-20: {"fp32x", "fp16"}"""
    return {"fp32x": max(4 * max(d["d32"], d["dx"]), FLOOR), "fp16": max(4 * d["d16"], FLOOR)}
