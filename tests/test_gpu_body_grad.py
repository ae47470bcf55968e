"""GPU: the backward pass of SMPL-X linear blend skinning (include/amuse_hip.h amuse_body_enable_grad / amuse_body_vertex_loss_grad, csrc/k_body_bwd.hip) through
amuse_amd/body.py against the float64 autograd of the differentiable torch twin.  `smplx` is not installed: nothing here is a pin against that package.

Bars (tests/body_grad_cases.py), computed on the CPU in the same test from the same inputs, never from the GPU's output:
  fp32x   max(4 x max(d32, dx), 2^-20): d32 = the numpy restatement of the backward formulas in float32, dx = float32 with the split-fp16 products in the forward
          recompute and in the transposed product
  fp16    max(4 x d16, 2^-20): the one-product forms
every distance relative to max|grad| of that output."""
import numpy as np
import pytest
import torch

import body_cases as bc
import body_grad_cases as gc
import body_grad_ref as bg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine(model, betas, grad=True):
    from amuse_amd.body import BodyEngine, BodyModel
    eng = BodyEngine(DEV, BodyModel.from_dict(model), "fp32x")
    eng.set_subjects(betas)
    if grad:
        eng.enable_grad()
    return eng


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _check(name, model, betas, eng, ref, a, b, subject=None):
    """grad_a (and grad_b) of both precisions against the oracle, each within its own bar; returns the oracle's gradients"""
    N = ref.shape[0]
    _, ga64, gb64 = gc.oracle(model, betas, ref, a, b, subject)
    sub = _dev(np.arange(N) % betas.shape[0] if subject is None else subject, torch.int32)
    want = [(a, ga64)] + ([(b, gb64)] if b is not None else [])
    bars = [gc.bars(gc.grad_distances(model, betas, ref, c, g, subject)) for c, g in want]
    for prec in ("fp32x", "fp16"):
        got = eng.vertex_loss_grad(_dev(ref), _dev(a), _dev(b) if b is not None else None, sub, precision=prec)
        for i, (c, g64) in enumerate(want):
            e = gc.rel(got[i].cpu().numpy(), g64)
            print(f"{name} {prec} grad_{'ab'[i]}: distance {e:.3e} bar {bars[i][prec]:.3e} max|grad| {np.abs(g64).max():.4g}")
            assert e <= bars[i][prec], (name, prec, i, e, bars[i][prec])
    return ga64, gb64


@pytest.fixture(scope="module")
def small():
    model, betas = bc.make_model(203), bc.make_betas(3)
    eng = _engine(model, betas)
    yield model, betas, eng
    eng.close()


@pytest.fixture(scope="module")
def rows17():
    return gc.rows_of(bc.make_loss_sets(3, 17))   # N = 3, F = 17: across a frame tile; clip 0 of `a` is 1.5 m off, so both SmoothL1 branches run


@pytest.mark.parametrize("V", [203, 208])
def test_gradient_vs_float64_autograd(small, rows17, V):
    model, betas, eng = small if V == 203 else (bc.make_model(V, seed=5), bc.make_betas(3), None)
    own = eng is None
    if own:
        eng = _engine(model, betas)
    _check(f"V {V}", model, betas, eng, *rows17)
    if own:
        eng.close()


def test_transposed_product_alone(rows17):
    """every skinning weight on joint 0: joints 1..54 move the vertices through the pose-blend offsets only, so their gradient rows are the transposed product's"""
    model = bc.make_model(203, seed=11)
    model["weights"] = np.zeros_like(model["weights"])
    model["weights"][:, 0] = 1.0
    betas = bc.make_betas(3)
    eng = _engine(model, betas)
    ga64, _ = _check("weights on joint 0", model, betas, eng, *rows17)
    sub = _dev(np.arange(3), torch.int32)
    got = eng.vertex_loss_grad(_dev(rows17[0]), _dev(rows17[1]), None, sub)[0].cpu().numpy()
    eng.close()
    rest, rest64 = got[..., 6:330], ga64[..., 6:330]
    assert np.abs(rest64).max() > 0 and np.abs(rest).max() > 0
    dist = gc.grad_distances(model, betas, rows17[0], rows17[1], ga64)
    # the rows of joints 1..54 against THEIR OWN maximum: the emulation's distance on the same rows
    cb = gc.clip_betas(betas, 3)
    emu = [bg.loss_grad(model, cb, rows17[0], rows17[1], np.float32, bl, tb)[1][..., 6:330] for bl, tb in ((None, None), (gc.br.blend_split(True), bg.tblend_split))]
    bar = max(4 * max(gc.rel(e, rest64) for e in emu), gc.FLOOR)
    e = gc.rel(rest, rest64)
    print(f"joints 1..54 alone: distance {e:.3e} bar {bar:.3e} max {np.abs(rest64).max():.4g} (whole-row distances {dist})")
    assert e <= bar


def test_chain_alone(rows17):
    """zero posedirs, joints 0..11 a chain 11 deep: the chain's backward pass by itself"""
    model = bc.make_model(203, seed=12)
    model["posedirs"] = np.zeros_like(model["posedirs"])
    betas = bc.make_betas(3)
    eng = _engine(model, betas)
    assert all(model["parents"][j] == j - 1 for j in range(1, 12))
    _check("zero posedirs", model, betas, eng, *rows17)
    eng.close()


def test_edges(small, rows17):
    from amuse_amd import _lib
    model, betas, eng = small
    ref, a, b = rows17
    sub = _dev(np.arange(3), torch.int32)
    ga, gb = eng.vertex_loss_grad(_dev(ref), _dev(a), _dev(b), sub)
    ga2, gb2 = eng.vertex_loss_grad(_dev(ref), _dev(a), _dev(b), sub)
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)                                  # deterministic: the same call twice, bit for bit
    g1, none = eng.vertex_loss_grad(_dev(ref), _dev(a), None, sub)                        # b = NULL
    assert none is None and torch.equal(g1, ga)
    gs = eng.vertex_loss_grad(_dev(ref), _dev(a), None, sub, scale=(0.25, 1.0))[0]        # a power of two: exact
    assert torch.equal(gs, ga * 0.25)
    _check("F 16", model, betas, eng, ref[:, :16], a[:, :16], None)                      # F = 16 exactly (N F = 48)
    _check("N F 51", model, betas, eng, ref, a, None)                                     # N F no multiple of 16
    # a skipped clip keeps a sentinel; the others' rows are bitwise those of the call without the skip
    skip = _dev(np.array([0, -1, 2]), torch.int32)
    out = torch.full((3, 17, 333), 7.0, device=DEV), torch.full((3, 17, 333), 7.0, device=DEV)
    eng.vertex_loss_grad(_dev(ref), _dev(a), _dev(b), skip, out=out)
    for o, g in zip(out, (ga, gb)):
        assert bool((o[1] == 7.0).all()) and torch.equal(o[0], g[0]) and torch.equal(o[2], g[2])
    # errors
    rc = eng.lib.amuse_body_vertex_loss_grad(eng.ctx, _dev(ref).data_ptr(), _dev(a).data_ptr(), None, _lib.BODY_ROT_AA, sub.data_ptr(), 3, 17, _lib.PREC_F32X, 1.0, 1.0,
                                             ga.data_ptr(), None, None)
    assert rc == -1                                                                       # AMUSE_EINVAL: axis-angle rows
    cold = _engine(model, betas, grad=False)
    assert cold.info()["grad"] == 0 and eng.info()["grad"] == 1
    rc = cold.lib.amuse_body_vertex_loss_grad(cold.ctx, _dev(ref).data_ptr(), _dev(a).data_ptr(), None, _lib.BODY_ROT_6D, sub.data_ptr(), 3, 17, _lib.PREC_F32X, 1.0, 1.0,
                                              ga.data_ptr(), None, None)
    assert rc == -4                                                                       # AMUSE_ESTATE before enable_grad
    cold.enable_grad()
    assert torch.equal(cold.vertex_loss_grad(_dev(ref), _dev(a), None, sub)[0], ga)       # another context: the same bits
    cold.close()


def test_real_vertex_count_grad():
    """V = 10,475, N = 2, F = 300 with a period of 20 distinct frames: the float64 oracle differentiates 40 frames, the GPU's 600 rows equal them period by period
    (a frame, tile, chunk or pair index gone wrong reads another phase: 20 against tiles of 16)"""
    model, betas = bc.make_model(10475, seed=7), bc.make_betas(2, seed=8)
    ref, a, _ = gc.rows_of(bc.make_loss_sets(2, 20, seed=9))
    _, g64, _ = gc.oracle(model, betas, ref, a)
    bars = gc.bars(gc.grad_distances(model, betas, ref, a, g64))
    eng = _engine(model, betas)
    sub = _dev(np.arange(2), torch.int32)
    for prec in ("fp32x", "fp16"):
        got = eng.vertex_loss_grad(_dev(np.tile(ref, (1, 15, 1))), _dev(np.tile(a, (1, 15, 1))), None, sub, precision=prec)[0].cpu().numpy()
        assert got.shape == (2, 300, 333)
        e = max(gc.rel(got[:, 20 * k:20 * k + 20], g64) for k in range(15))
        print(f"V 10475 {prec}: distance {e:.3e} bar {bars[prec]:.3e} max|grad| {np.abs(g64).max():.4g}")
        assert e <= bars[prec]
    eng.close()


def test_directional_derivative_through_the_abi(small, rows17):
    """<grad_a, u> against the difference quotient of amuse_body_vertex_loss's double sums at a +- eps u; the bar: 4 x the error the float32 restatement makes on
    the same quotient (against the float64 oracle's <grad, u>)"""
    model, betas, eng = small
    ref, a, _ = rows17
    _, g64, _ = gc.oracle(model, betas, ref, a)
    u = (g64 / np.linalg.norm(g64)).astype(np.float32)   # along the gradient: the quotient is as large as a unit step makes it
    eps = np.float32(2.0 ** -4)
    ap, am = (a + eps * u).astype(np.float32), (a - eps * u).astype(np.float32)
    step = (ap.astype(np.float64) - am.astype(np.float64))
    cb = gc.clip_betas(betas, 3)
    q64 = (bg.loss_grad(model, cb, ref, ap)[0] - bg.loss_grad(model, cb, ref, am)[0])
    q32 = (bg.loss_grad(model, cb, ref, ap, np.float32)[0] - bg.loss_grad(model, cb, ref, am, np.float32)[0])
    lin64 = float((g64 * step).sum())
    bar = 4 * abs(q32 - lin64) / abs(lin64)
    sub = _dev(np.arange(3), torch.int32)
    sp = float(eng.vertex_loss(_dev(ref), _dev(ap), None, sub, "6d")[0])
    sm = float(eng.vertex_loss(_dev(ref), _dev(am), None, sub, "6d")[0])
    g = eng.vertex_loss_grad(_dev(ref), _dev(a), None, sub)[0].cpu().numpy().astype(np.float64)
    lin = float((g * step).sum())
    e = abs((sp - sm) - lin) / abs(lin)
    print(f"quotient {sp - sm:.9g} <grad, step> {lin:.9g} relative {e:.3e} bar {bar:.3e} (float64 quotient {q64:.9g}, float32 {q32:.9g}, float64 <grad, step> {lin64:.9g})")
    assert e <= bar


def test_vertex_loss_fn(small, rows17):
    from amuse_amd.body import VertexLossFn
    model, betas, eng = small
    ref, a, b = (_dev(x) for x in rows17)
    sub = _dev(np.arange(3), torch.int32)
    ga, gb = eng.vertex_loss_grad(ref, a, b, sub)
    la, lb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    s = VertexLossFn.apply([(eng, sub)], ref, la, lb, None)
    assert torch.equal(s.detach(), eng.vertex_loss(ref, a, b, sub, "6d"))
    w = torch.tensor([0.5, -3.0], dtype=torch.float64, device=DEV)
    (s * w).sum().backward()
    assert torch.equal(la.grad, ga * 0.5) and torch.equal(lb.grad, gb * -3.0)
    # only b requires grad: a gets none and is not computed - the one backward pass runs on b as the first candidate
    calls = []
    orig = eng.vertex_loss_grad
    eng.vertex_loss_grad = lambda *args, **kw: (calls.append(args), orig(*args, **kw))[1]
    try:
        lb2 = b.clone().requires_grad_(True)
        s = VertexLossFn.apply([(eng, sub)], ref, a, lb2, None)
        s[1].backward()
    finally:
        del eng.vertex_loss_grad
    assert len(calls) == 1 and calls[0][1].data_ptr() == lb2.data_ptr() and calls[0][2] is None
    assert torch.equal(lb2.grad, eng.vertex_loss_grad(ref, b, None, sub)[0])
    assert not a.requires_grad and a.grad is None
