"""CPU: the backward pass of the body model without a GPU - the numpy restatement of the backward formulas (tests/body_grad_ref.py) against the float64 autograd
of the differentiable torch twin and against central differences; LatentPriorLosses(vtex_grad=True) on the CPU; the --vtex-grad flag."""
import numpy as np
import pytest
import torch

import body_cases as bc
import body_grad_cases as gc
import body_grad_ref as bg
from amuse_amd import body

ATTR = [("scott", "male"), ("miranda", "female"), ("wayne", "male"), ("sophie", "female")]


@pytest.mark.parametrize("V", [37, 203])
def test_restatement_vs_float64_autograd(V):
    model, betas = bc.make_model(V), bc.make_betas(3)
    ref, a, b = gc.rows_of(bc.make_loss_sets(3, 5))
    s, ga, gb = gc.oracle(model, betas, ref, a, b)
    cb = gc.clip_betas(betas, 3)
    for i, (cand, g64) in enumerate(((a, ga), (b, gb))):
        S, g = bg.loss_grad(model, cb, ref, cand)
        assert abs(S - s[i]) <= 1e-12 * s[i]
        assert gc.rel(g, g64) <= 1e-12, gc.rel(g, g64)
    # both SmoothL1 branches are in `a` (clip 0 is 1.5 m off): its translation gradient saturates at V per coordinate there, and nowhere else
    assert np.abs(ga[0, :, 330:]).max() == V and np.abs(ga[1:, :, 330:]).max() < V
    # central differences in float64 at a handful of coordinates: a 6D column of the root, of a chain joint, of a leaf, and a translation column
    h = 1e-6
    for n, f, k in ((0, 0, 2), (1, 3, 6 * 5 + 4), (2, 4, 6 * 54 + 1), (1, 1, 331), (0, 2, 6 * 20 + 3)):
        ap, am = a.astype(np.float64).copy(), a.astype(np.float64).copy()
        ap[n, f, k] += h
        am[n, f, k] -= h
        q = (bg.loss_grad(model, cb, ref, ap)[0] - bg.loss_grad(model, cb, ref, am)[0]) / (2 * h)
        assert abs(q - ga[n, f, k]) <= 1e-6 * max(abs(ga[n, f, k]), 1.0), (n, f, k, q, ga[n, f, k])


def test_emulations_are_close_and_distinct():
    """the distances that set the GPU bars: float32 and split-fp16 within a few 1e-7 of float64, the one-product form an order worse - a bar from one does not
    cover a kernel that silently ran the other"""
    model, betas = bc.make_model(203), bc.make_betas(3)
    ref, a, _ = gc.rows_of(bc.make_loss_sets(3, 5))
    _, g64, _ = gc.oracle(model, betas, ref, a)
    d = gc.grad_distances(model, betas, ref, a, g64)
    print(d)
    assert 0 < d["d32"] < 2e-6 and 0 < d["dx"] < 2e-6 and d["d16"] < 1e-4
    bars = gc.bars(d)
    assert bars["fp32x"] >= gc.FLOOR and bars["fp16"] >= bars["fp32x"] * 0.5


def _rs_set(seed=0):
    sets = bc.make_loss_sets(4, 3, seed=seed)
    g = torch.Generator().manual_seed(seed)
    return {"m_ref": torch.from_numpy(bc.feats_rows(sets[0][2], sets[0][1])), "m_rst": torch.from_numpy(bc.feats_rows(sets[1][2], sets[1][1])).requires_grad_(True),
            "gen_m_rst": torch.from_numpy(bc.feats_rows(sets[2][2], sets[2][1])), "noise": torch.randn(4, 1, 128, generator=g),
            "noise_pred": torch.randn(4, 1, 128, generator=g), "attr": ATTR}


def test_latent_prior_losses_vtex_grad():
    """m_rst.grad after update(...).backward() = the gradient of the other terms + LAMBDA_REC / (B F V 3) x the twin's gradient; off: today's values and gradients"""
    from amuse_amd.train_gesture import LatentPriorLosses
    models = {g: body.BodyModel.from_dict(bc.make_model(V=37, seed=20 + i)) for i, g in enumerate(("male", "female", "neutral"))}
    bl = body.BodyLosses(models, "cpu", version="v0")
    cfg = {"LAMBDA_KL": 0.0, "LAMBDA_REC": 0.7, "vtex_displacement": True}
    L_on, L_off, L_none = (LatentPriorLosses(cfg, "cpu", body=bl, vtex_grad=True), LatentPriorLosses(cfg, "cpu", body=bl, vtex_grad=False),
                           LatentPriorLosses(dict(cfg, vtex_displacement=False)))
    g = {}
    totals = {}
    for name, L in (("on", L_on), ("off", L_off), ("none", L_none)):
        rs = _rs_set()
        total = L.update(rs)
        total.backward()
        g[name], totals[name] = rs["m_rst"].grad.clone(), total.detach().clone()
    assert torch.equal(g["off"], g["none"])                                   # the reference's behaviour: a value, no gradient
    assert torch.equal(totals["on"], totals["off"])                           # the same value either way
    for k in L_off.losses:
        assert torch.equal(L_on.sums[k], L_off.sums[k]), k
    # the twin's gradient, clip by clip through the clip's own model and betas
    rs = _rs_set()
    rows = bl.subject_rows(ATTR)
    want = np.zeros((4, 3, 333))
    for i, gname in enumerate(bl.genders):
        idx = np.nonzero(rows[i] >= 0)[0]
        a = rs["m_rst"].detach()[idx].double().requires_grad_(True)
        s = body.torch_loss_sums(models[gname], bl.betas, rs["m_ref"][idx], a, None, subject=rows[i][idx], kind="6d", differentiable=True)
        s[0].backward()
        want[idx] = a.grad.numpy()
    extra = (g["on"].double() - g["off"].double()).numpy()
    scale = 0.7 / (4 * 3 * 37 * 3)
    assert np.abs(want).max() > 0
    err = np.abs(extra - scale * want).max()
    bar = 4 * 2.0 ** -24 * float(g["on"].abs().max())                         # float32 storage: of the term's own gradient, of its sum with the others'
    print(f"vertex term's gradient: max {np.abs(scale * want).max():.3e}, distance {err:.3e}, bar {bar:.3e}")
    assert np.abs(scale * want).max() > 100 * bar and err <= bar, (err, bar)
    assert rs["gen_m_rst"].grad is None
    # a generation that requires grad gets its gradient too
    rs2 = _rs_set()
    rs2["gen_m_rst"] = rs2["gen_m_rst"].clone().requires_grad_(True)
    LatentPriorLosses(cfg, "cpu", body=bl, vtex_grad=True).update(rs2).backward()
    rs3 = _rs_set()
    rs3["gen_m_rst"] = rs3["gen_m_rst"].clone().requires_grad_(True)
    LatentPriorLosses(cfg, "cpu", body=bl, vtex_grad=False).update(rs3).backward()
    assert float((rs2["gen_m_rst"].grad - rs3["gen_m_rst"].grad).abs().max()) > 0


def test_twin_default_is_unchanged():
    """differentiable=False: the values of the differentiable mode, and nothing reaches the inputs"""
    model, betas = body.BodyModel.from_dict(bc.make_model(37)), bc.make_betas(3)
    ref, a, b = (torch.from_numpy(x) for x in gc.rows_of(bc.make_loss_sets(3, 5)))
    a = a.clone().requires_grad_(True)
    s0 = body.torch_loss_sums(model, betas, ref, a, b, kind="6d")
    s1 = body.torch_loss_sums(model, betas, ref, a, b, kind="6d", differentiable=True)
    assert not s0.requires_grad and s1.requires_grad
    assert float((s0 - s1.detach()).abs().max()) <= 1e-12 * float(s0.max())


@pytest.mark.parametrize("entry", ["train_gesture", "main"])
def test_vtex_grad_needs_smplx_models(entry, tmp_path):
    if entry == "train_gesture":
        from amuse_amd import train_gesture
        with pytest.raises(SystemExit, match="--vtex-grad"):
            train_gesture.main(["--device", "cpu", "--epochs", "1", "--vtex-grad", "--out", str(tmp_path)])
    else:
        from amuse_amd import main
        with pytest.raises(SystemExit, match="--vtex-grad"):
            main.main(["--fn", "train_gesture", "--synthetic", "--device", "cpu", "--vtex-grad", "--skip-vtex-loss"])
