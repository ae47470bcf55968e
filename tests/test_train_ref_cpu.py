"""CPU: the float64 AdamW restatement of tests/train_ref.py against torch.optim.AdamW itself on float64 parameters - the reference the GPU tests of
tests/test_gpu_train_graph.py hold k_train_adamw / k_train_adamw_dev to must not drift."""
import math

import numpy as np
import torch

import train_ref

LR, WD = 3e-3, 0.01
SHAPES = [(128, 128), (128,), (384, 128), (7,)]          # tests/test_gpu_train_ops.py _flat_setup


def test_adamw_ref_equals_torch_adamw_in_float64():
    """Five steps, lr 3e-3, weight decay 0.01, fresh seeded gradients per step: parameters to 1e-12 of the largest parameter (the same arithmetic up to operation
    order), and both moments, read from torch's state, to 1e-12 of their largest entry."""
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in SHAPES]
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD)
    grp = opt.param_groups[0]
    assert not grp["amsgrad"] and not grp.get("maximize", False)
    p = np.concatenate([q.detach().numpy().ravel() for q in params])
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, 6):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES]
        for q, gr in zip(params, grads):
            q.grad = gr.clone()
        opt.step()
        p, m, v = train_ref.adamw_ref(p, np.concatenate([gr.numpy().ravel() for gr in grads]), m, v, t, LR, grp["betas"], grp["eps"], WD)
    want_p = np.concatenate([q.detach().numpy().ravel() for q in params])
    want_m = np.concatenate([opt.state[q]["exp_avg"].numpy().ravel() for q in params])
    want_v = np.concatenate([opt.state[q]["exp_avg_sq"].numpy().ravel() for q in params])
    for name, got, want in (("p", p, want_p), ("m", m, want_m), ("v", v, want_v)):
        err = float(np.abs(got - want).max() / np.abs(want).max())
        assert err < 1e-12, (name, err)
    assert all(float(opt.state[q]["step"]) == 5.0 for q in params)
    # the update is not a no-op at this learning rate: a skipped step would be ~1e-3 of the largest parameter away
    p4 = train_ref.adamw_ref(want_p, np.ones_like(p), want_m, want_v, 6, LR, grp["betas"], grp["eps"], WD)[0]
    assert float(np.abs(p4 - want_p).max() / np.abs(want_p).max()) > 1e-4


def test_adamw_ref_leaves_its_inputs_alone_and_takes_float32_arrays():
    rng = np.random.default_rng(1)
    p, g = rng.standard_normal(33).astype(np.float32), rng.standard_normal(33).astype(np.float32)
    m, v = np.zeros(33, np.float32), np.zeros(33, np.float32)
    keep = [a.copy() for a in (p, g, m, v)]
    out = train_ref.adamw_ref(p, g, m, v, 1, LR, (0.9, 0.999), 1e-8, WD)
    assert all(o.dtype == np.float64 and o.shape == (33,) for o in out)
    assert all(np.array_equal(a, b) for a, b in zip((p, g, m, v), keep))
    # step 1 in closed form: m = 0.1 g, v = 0.001 g^2, m^ = g, v^ = g^2 -> p (1 - lr wd) - lr g / (|g| + eps)
    gd, pd = g.astype(np.float64), p.astype(np.float64)
    want = pd * (1 - LR * WD) - LR * gd / (np.abs(gd) + 1e-8)
    assert float(np.abs(out[0] - want).max()) < 1e-12


def test_adamw_scalars_in_closed_form():
    for t in (1, 2, 1000, 100_000):
        s0, s1 = train_ref.adamw_scalars(t, LR, (0.9, 0.999))
        assert abs(s0 * (1.0 - 0.9 ** t) - LR) < 1e-15 and abs(s1 * s1 * (1.0 - 0.999 ** t) - 1.0) < 1e-12
    s0, s1 = train_ref.adamw_scalars(1, LR, (0.9, 0.999))
    assert abs(s0 - LR / 0.1) < 1e-12 and abs(s1 - 1.0 / math.sqrt(0.001)) < 1e-9
