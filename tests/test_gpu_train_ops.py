"""GPU: the train_gesture step's fused layers (amuse_amd/train_ops.py on csrc/k_train.hip) against the eager layers of nn_modules.py - the
autograd twins that tests/test_train_cpu.py pins to the reference modules' goldens (utils/cross_attention.py:259-272,323-345)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@pytest.fixture()
def eager_switch():
    old = os.environ.get("AMUSE_TRAIN_FUSED")
    yield lambda on: os.environ.__setitem__("AMUSE_TRAIN_FUSED", "1" if on else "0")
    if old is None:
        os.environ.pop("AMUSE_TRAIN_FUSED", None)
    else:
        os.environ["AMUSE_TRAIN_FUSED"] = old


def test_raw_kernels_against_torch():
    from amuse_amd import train_ops as T
    g = torch.Generator(device=DEV).manual_seed(0)
    for rows in (1, 7, 160, 9664):
        x, y = (torch.randn(rows, 128, device=DEV, generator=g) for _ in range(2))
        bias, ga, be = (torch.randn(128, device=DEV, generator=g) for _ in range(3))
        out, zhat, rstd = T.ln_fwd(x, y, bias, ga, be, 0.0, 1, 1)
        ref = torch.nn.functional.layer_norm(x + y + bias, (128,), ga, be)
        assert float((out - ref).abs().max()) < 2e-5, rows
        xr, yr, gr, br, bb = (t.clone().requires_grad_(True) for t in (x, y, ga, be, bias))
        dout = torch.randn(rows, 128, device=DEV, generator=g)
        torch.nn.functional.layer_norm(xr + yr + bb, (128,), gr, br).backward(dout)
        dx, dy, dg, db, dbias = T.ln_bwd(dout * 0.25, zhat, rstd, ga, 0.0, 1, 1, dout2=dout * 0.75)   # (two addends: exact in fp32)
        assert torch.equal(dx, dy)                                           # p = 0: the mask is all ones
        for got, want in ((dx, xr.grad), (dg, gr.grad), (db, br.grad), (dbias, bb.grad)):
            assert _rel(got, want) < 2e-5, rows
        # FFN activation
        h, b1 = torch.randn(rows, 512, device=DEV, generator=g) * 2, torch.randn(512, device=DEV, generator=g)
        a = T.bias_gelu_drop_fwd(h, b1, 0.0, 1, 2)
        assert float((a - torch.nn.functional.gelu(h + b1)).abs().max()) < 2e-6
        hr, b1r = h.clone().requires_grad_(True), b1.clone().requires_grad_(True)
        da = torch.randn(rows, 512, device=DEV, generator=g)
        torch.nn.functional.gelu(hr + b1r).backward(da)
        dh, db1 = T.bias_gelu_drop_bwd(da, h, b1, 0.0, 1, 2)
        assert _rel(dh, hr.grad) < 2e-6 and _rel(db1, b1r.grad) < 2e-5, rows
        # column sums (in_proj's bias gradient: 384 columns), deterministic
        q = torch.randn(rows, 384, device=DEV, generator=g)
        s = T.colsum(q)
        assert _rel(s, q.double().sum(0).float()) < 1e-5 and torch.equal(s, T.colsum(q))


def test_dropout_masks_are_regenerated_by_the_backward_kernels():
    from amuse_amd import train_ops as T
    rows, p = 4096, 0.1
    one = torch.ones(128, device=DEV)
    zero = torch.zeros(128, device=DEV)
    # FFN activation: large positive h -> gelu(h) = h, so out / h is the mask / (1 - p)
    h = torch.full((rows, 512), 30.0, device=DEV)
    a = T.bias_gelu_drop_fwd(h, torch.zeros(512, device=DEV), p, 7, 3)
    m = a / 30.0
    kept = m > 0
    assert abs(float(kept.float().mean()) - (1 - p)) < 3e-3 and float((m[kept] - 1 / (1 - p)).abs().max()) < 1e-6
    dh, db = T.bias_gelu_drop_bwd(torch.ones_like(h), h, torch.zeros(512, device=DEV), p, 7, 3)
    assert torch.equal(dh > 0, kept) and float((dh[kept] - 1 / (1 - p)).abs().max()) < 1e-5 and _rel(db, dh.sum(0)) < 1e-5
    assert not torch.equal(T.bias_gelu_drop_fwd(h, torch.zeros(512, device=DEV), p, 7, 4) > 0, kept)       # another offset: another mask
    assert not torch.equal(T.bias_gelu_drop_fwd(h, torch.zeros(512, device=DEV), p, 8, 3) > 0, kept)       # another seed
    # LayerNorm: x = 0, y = 1: the row is a two-level signal, high where kept
    y = torch.ones(rows, 128, device=DEV)
    out, zhat, rstd = T.ln_fwd(None, y, None, one, zero, p, 7, 5)
    keptl = out > 0
    assert abs(float(keptl.float().mean()) - (1 - p)) < 5e-3
    ref = torch.nn.functional.layer_norm(keptl.float() / (1 - p), (128,))
    ok = keptl.float().sum(1) < 128                                          # (a row with nothing dropped is constant: LayerNorm of it is 0 / eps)
    assert float((out - ref)[ok].abs().max()) < 1e-4
    dout = torch.randn(rows, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    dx, dy, *_ = T.ln_bwd(dout, zhat, rstd, one, p, 7, 5)
    assert torch.equal(dy != 0, keptl & (dx != 0)) and float((dy - dx * keptl / (1 - p)).abs().max()) < 1e-6


def _layers(kind, seed):
    from amuse_amd import nn_modules as nm
    torch.manual_seed(seed)
    m = (nm.EncoderLayer if kind == "enc" else nm.DecoderLayer)(p=0.1).to(DEV)
    for p in m.parameters():                                                # non-trivial LayerNorm parameters and biases
        if p.dim() == 1:
            p.data.normal_(1.0 if p.data.mean() > 0.5 else 0.0, 0.2)
    return m


@pytest.mark.parametrize("kind,B,S", [("enc", 3, 302), ("enc", 32, 5), ("dec", 3, 300), ("dec", 1, 1)])
def test_fused_layer_equals_the_eager_layer_in_eval_mode(kind, B, S, eager_switch):
    m = _layers(kind, 1).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(B, S, 128, device=DEV, generator=g)
    mem = torch.randn(B, 1, 128, device=DEV, generator=g)
    dout = torch.randn(B, S, 128, device=DEV, generator=g)
    res = {}
    for on in (False, True):
        eager_switch(on)
        xr, mr = x.clone().requires_grad_(True), mem.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = m(xr) if kind == "enc" else m(xr, mr)
        out.backward(dout)
        res[on] = (out.detach(), xr.grad, mr.grad if kind == "dec" else None, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    (o0, dx0, dm0, g0), (o1, dx1, dm1, g1) = res[False], res[True]
    assert float((o0 - o1).abs().max()) < 2e-5
    assert _rel(dx1, dx0) < 2e-4
    if kind == "dec":
        assert _rel(dm1, dm0) < 2e-4
    assert set(g0) == set(g1)
    for n in g0:
        assert g1[n].shape == g0[n].shape and _rel(g1[n], g0[n]) < 2e-4, n        # the bar of the round-3 brief: gradients <= 2e-4 . max


@pytest.mark.parametrize("kind", ["enc", "dec"])
def test_fused_layer_in_train_mode_is_consistent_and_unbiased(kind, eager_switch):
    """Dropout live (p = 0.1 everywhere, attention dropout inside the vendor kernel): the backward pass must see the forward pass's masks -
    checked by a directional derivative in float32 on a re-seeded replay - and the mean over many masks approaches the eval output."""
    from amuse_amd import train_ops as T
    eager_switch(True)
    m = _layers(kind, 3).train()
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(2, 40, 128, device=DEV, generator=g)
    mem = torch.randn(2, 1, 128, device=DEV, generator=g)

    def run(xin, off0):
        T._OFFSET[0] = off0                                                  # replay the same masks (the vendor kernel's come from torch's generator)
        torch.manual_seed(11)
        return m(xin) if kind == "enc" else m(xin, mem)

    xr = x.clone().requires_grad_(True)
    out = run(xr, 1000)
    w = torch.randn_like(out)
    (out * w).sum().backward()
    assert torch.equal(run(x, 1000), out.detach())                           # same offsets + seed: same masks, bitwise
    assert not torch.equal(run(x, 2000), out.detach())
    d = torch.randn_like(x)
    eps = 1e-2
    fd = float(((run(x + eps * d, 1000) - run(x - eps * d, 1000)) * w).sum().double()) / (2 * eps)
    an = float((xr.grad * d).sum().double())
    assert abs(fd - an) < 2e-2 * max(1.0, abs(an)), (fd, an)
    m.eval()
    ref = m(x) if kind == "enc" else m(x, mem)
    m.train()
    acc = torch.zeros_like(ref)
    n = 200
    for i in range(n):
        acc += m(x) if kind == "enc" else m(x, mem)
    # post-norm layers are not linear in the masks; the mean stays within a few percent of the eval output
    assert float((acc / n - ref).abs().mean() / ref.abs().mean()) < 0.08


def test_trainer_step_on_fused_layers_matches_the_eager_step_without_dropout(eager_switch):
    """One whole train_gesture iteration (prior encode / decode + epsilon loss + AdamW) with dropout 0 on both paths: losses and the flat gradient."""
    from amuse_amd import train_gesture as tg
    res = {}
    for on in (False, True):
        eager_switch(on)
        torch.manual_seed(5)
        tr = tg.build_trainer(DEV, seed=5, use_hip_sampler=False, dropout=0.0)
        batch = tg.synthetic_batch(4, 7, DEV)
        noise = torch.randn(4, 1, 128, generator=torch.Generator().manual_seed(1)).to(DEV)
        ts = torch.tensor([3, 500, 998, 17], device=DEV)
        eps = torch.randn(1, 4, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
        loss = tr.forward_losses(batch, noise=noise, timesteps=ts, eps_enc=eps, eps_inf=eps)
        tr.backward_into_bucket(loss)
        res[on] = (float(loss), tr.flat_grad.clone())
    assert abs(res[True][0] - res[False][0]) < 1e-5 * max(1.0, abs(res[False][0]))
    assert _rel(res[True][1], res[False][1]) < 2e-4


def test_gradient_sink_fills_the_bucket_like_autograd_does(monkeypatch):
    """grads_mode "sink" (the layer calls write their parameter gradients straight into the trainer's bucket, train_ops.sink_begin) against
    "steal" (autograd hands out fresh gradients, one copy packs them) and "views": the same kernels compute the same numbers, so the bucket is BITWISE the
    same - dropout live, the same seeds - and the parameters after two optimizer steps are too."""
    from amuse_amd import train_gesture as tg, train_ops
    res = {}
    for mode in ("sink", "steal", "views"):
        torch.manual_seed(9)
        train_ops._OFFSET[0] = 0
        tr = tg.build_trainer(DEV, seed=2, use_hip_sampler=False, grads_mode=mode)
        assert tr.grads_mode == mode
        buckets = []
        for i in range(2):
            batch = tg.synthetic_batch(4, 20 + i, DEV)
            noise = torch.randn(4, 1, 128, generator=torch.Generator().manual_seed(1 + i)).to(DEV)
            ts = torch.tensor([3, 500, 998, 17], device=DEV)
            eps = torch.randn(1, 4, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
            tr.train_step(batch, noise=noise, timesteps=ts, eps_enc=eps, eps_inf=eps)
            buckets.append(tr.flat_grad.clone())
        res[mode] = (buckets, tr.flat_param.clone())
        assert train_ops._SINK is None                                      # (the sink is closed outside a backward pass)
    assert float(res["sink"][0][0].abs().max()) > 0
    used = res["steal"][0][0] != 0
    assert float(used.float().mean()) > 0.9                                 # (the bucket really is filled: all but the parameters the step never reaches)
    for other in ("steal", "views"):
        for a, b in zip(res["sink"][0], res[other][0]):
            assert torch.equal(a, b), other
        assert torch.equal(res["sink"][1], res[other][1]), other


def test_flat_adamw_equals_torch_adamw_and_keeps_its_state_layout():
    """train_ops.FlatAdamW (one launch per contiguous run of the flat buffers) against torch.optim.AdamW on the same parameters and gradients, five
    steps; a parameter outside the optimizer (the trainer's never-reached mem_pos.pe) is not touched; state_dict() has torch's structure."""
    from amuse_amd.train_ops import FlatAdamW
    g = torch.Generator(device=DEV).manual_seed(0)
    shapes = [(128, 128), (128,), (500, 1, 128), (384, 128), (7,)]
    n = sum(int(np.prod(s)) for s in shapes)
    flat_p, flat_g = torch.randn(n, device=DEV, generator=g), torch.zeros(n, device=DEV)
    params, layout, off = [], [], 0
    for s in shapes:
        k = int(np.prod(s))
        p = torch.nn.Parameter(flat_p[off:off + k].view(s))
        p.grad = flat_g[off:off + k].view(s)
        params.append(p)
        layout.append((p, off, k))
        off += k
    skip = params[2]
    ref_p = [p.detach().clone().requires_grad_(True) for p in params]
    ref = torch.optim.AdamW([p for p, q in zip(ref_p, params) if q is not skip], lr=3e-3)
    opt = FlatAdamW([p for p in params if p is not skip], flat_p, flat_g, layout, lr=3e-3)
    assert len(opt._ranges) == 2
    before = skip.detach().clone()
    for it in range(5):
        flat_g.copy_(torch.randn(n, device=DEV, generator=g))
        for p, q in zip(ref_p, params):
            p.grad = q.grad.clone()
        opt.step()
        ref.step()
    for p, q in zip(ref_p, params):
        if q is skip:
            assert torch.equal(q.detach(), before)
        else:
            assert _rel(q.detach(), p.detach()) < 2e-6
    sd, rsd = opt.state_dict(), ref.state_dict()
    assert sd["param_groups"][0]["params"] == rsd["param_groups"][0]["params"] and set(sd["state"]) == set(rsd["state"])
    for k in sd["state"]:
        assert float(sd["state"][k]["step"]) == 5.0 and _rel(sd["state"][k]["exp_avg"], rsd["state"][k]["exp_avg"]) < 2e-6
        assert _rel(sd["state"][k]["exp_avg_sq"], rsd["state"][k]["exp_avg_sq"]) < 2e-6


def _flat_setup(seed, dev=None):
    dev = dev or DEV
    g = torch.Generator(device=dev).manual_seed(seed)
    shapes = [(128, 128), (128,), (384, 128), (7,)]
    n = sum(int(np.prod(s)) for s in shapes)
    flat_p, flat_g = torch.randn(n, device=dev, generator=g), torch.zeros(n, device=dev)
    params, layout, off = [], [], 0
    for s in shapes:
        k = int(np.prod(s))
        p = torch.nn.Parameter(flat_p[off:off + k].view(s))
        p.grad = flat_g[off:off + k].view(s)
        params.append(p)
        layout.append((p, off, k))
        off += k
    return g, n, flat_p, flat_g, params, layout


def test_flat_adamw_resumes_from_a_saved_state_like_torch_adamw():
    """optimizer_state_dict round trip (the checkpoint writer stores it, trainer.py:468-496): 3 steps, save, load into a FRESH FlatAdamW and a fresh
    torch AdamW, 3 more steps on the same gradients -> same parameters; the loaded moments live in the flat buffers the kernel reads, the bias correction
    continues at step 4, zero_grad keeps the gradient views attached to the bucket."""
    from amuse_amd.train_ops import FlatAdamW
    g, n, flat_p, flat_g, params, layout = _flat_setup(3)
    opt = FlatAdamW(params, flat_p, flat_g, layout, lr=3e-3)
    for _ in range(3):
        flat_g.copy_(torch.randn(n, device=DEV, generator=g))
        opt.step()
    saved = {"opt": opt.state_dict(), "p": flat_p.clone()}
    grads = [torch.randn(n, device=DEV, generator=g) for _ in range(3)]
    # torch's own optimizer resumed from the same dict
    ref_p = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.AdamW(ref_p, lr=3e-3)
    ref.load_state_dict(saved["opt"])
    # a fresh flat optimizer (new buffers, as after a restart)
    _, _, fp2, fg2, params2, layout2 = _flat_setup(99)
    fp2.copy_(saved["p"])
    opt2 = FlatAdamW(params2, fp2, fg2, layout2, lr=3e-3)
    opt2.load_state_dict(saved["opt"])
    assert opt2._t == 3
    for p in params2:
        st = opt2.state[p]
        assert st["exp_avg"].data_ptr() >= opt2._m.data_ptr() and st["exp_avg"].data_ptr() < opt2._m.data_ptr() + 4 * n   # still views of the flat buffer
    assert _rel(opt2._m, opt._m) == 0 and _rel(opt2._v, opt._v) == 0
    for gr in grads:
        opt2.zero_grad(set_to_none=True)
        assert all(p.grad is not None and p.grad.data_ptr() >= fg2.data_ptr() for p in params2) and float(fg2.abs().max()) == 0
        fg2.copy_(gr)
        off = 0
        for p in ref_p:
            p.grad = gr[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        opt2.step()
        ref.step()
    for p, q in zip(ref_p, params2):
        assert _rel(q.detach(), p.detach()) < 2e-6
    assert float(opt2.state_dict()["state"][0]["step"]) == 6.0


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_layers_on_a_non_current_device():
    """The library calls run on the TENSORS' device (device guard in train_ops), not on the process's current device: a layer on cuda:1 while cuda:0 is current
    gives the bits of the same layer on cuda:0."""
    from amuse_amd import train_ops as T
    from amuse_amd.nn_modules import EncoderLayer
    torch.manual_seed(0)
    m0 = EncoderLayer().to("cuda:0").eval()
    m1 = EncoderLayer().to("cuda:1").eval()
    m1.load_state_dict(m0.state_dict())
    x = torch.randn(3, 5, 128)
    torch.cuda.set_device(0)
    outs = []
    for m, d in ((m0, "cuda:0"), (m1, "cuda:1")):
        xx = x.to(d).requires_grad_(True)
        y = T.encoder_layer(m, xx)
        y.square().sum().backward()
        outs.append((y.detach().cpu(), xx.grad.cpu(), m.linear1.weight.grad.cpu()))
    assert torch.cuda.current_device() == 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rows,K,N", [(9664, 333, 128), (9600, 256, 128), (32, 256, 128), (5, 128, 384),
                                      # the library's own weight-gradient kernel (k_train_wgrad: reductions from 1,024 rows, both widths multiples of 64, N x K < 65,536) - a
                                      # ragged last chunk of 192 rows, one chunk + 4 rows, its streaming instantiation (384 x 128), and its neighbours on rocBLAS
                                      (9664, 128, 128), (1028, 128, 128), (9664, 128, 384), (2000, 64, 64), (9664, 128, 512), (1020, 128, 128)])
def test_linear_fn_equals_f_linear(rows, K, N):
    from amuse_amd import train_ops as T
    g = torch.Generator(device=DEV).manual_seed(rows)
    m = torch.nn.Linear(K, N).to(DEV)
    x = torch.randn(2, rows // 2 if rows % 2 == 0 else rows, K, device=DEV, generator=g) if rows % 2 == 0 else torch.randn(rows, K, device=DEV, generator=g)
    dout = torch.randn(*x.shape[:-1], N, device=DEV, generator=g)
    res = []
    for fn in (lambda t: torch.nn.functional.linear(t, m.weight, m.bias), lambda t: T.linear(m, t)):
        xr = x.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = fn(xr)
        out.backward(dout)
        res.append((out.detach(), xr.grad, m.weight.grad.clone(), m.bias.grad.clone()))
    for a, b in zip(res[1], res[0]):
        assert a.shape == b.shape and _rel(a, b) < 2e-5


def test_weight_gradient_kernel_is_deterministic_and_matches_the_vendor_gemm():
    """dW = dy^T x on the library's chunked kernel: against float64, the same bits run after run (ordered sums, no atomics), and torch's (vendor) GEMM within
    fp32 summation noise."""
    from amuse_amd import train_ops as T, _lib
    st = T._st(torch.device(DEV))
    rows, N, K = 9664, 128, 128
    g = torch.Generator().manual_seed(3)
    dy, x = torch.randn(rows, N, generator=g).to(DEV), torch.randn(rows, K, generator=g).to(DEV)
    W = torch.zeros(N, K, device=DEV)

    def run():
        dW = torch.full((N, K), float("nan"), device=DEV)
        _lib.check(st["lib"].amuse_train_linear_bwd(dy.data_ptr(), x.data_ptr(), W.data_ptr(), rows, K, N, dW.data_ptr(), None, None, 0, st["ws"].data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream))
        return dW
    a, b = run(), run()
    ref = dy.double().T @ x.double()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert float((a.double() - ref).abs().max() / ref.abs().max()) < 2e-6
    v = dy.T @ x                                                             # the vendor library through torch
    assert not torch.equal(v, a)                                             # (really another implementation)
    assert float((v - a).abs().max() / ref.abs().max()) < 1e-5                 # (torch's library GEMM is itself 4e-6 from float64 here; the own kernel 1e-6)


def _linear_calls(lib, st, rows, N, K, seed, misalign=0):
    """amuse_train_linear_fwd (with / without bias), _bwd's dx (fresh / accumulating), dW and db for one shape -> {name: (result, float64 reference)};
    the third entry is torch's fp32 result (the vendor GEMM); every output carries a NaN guard row behind it."""
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g).to(DEV)
    Wb = (torch.randn(N * K + misalign, generator=g) / K ** 0.5).to(DEV)
    W = Wb[misalign:].view(N, K)
    b, dy, dx0 = torch.randn(N, generator=g).to(DEV), torch.randn(rows, N, generator=g).to(DEV), torch.randn(rows, K, generator=g).to(DEV)
    xd, Wd, bd, dyd = x.double(), W.double(), b.double(), dy.double()
    res = {}
    for bias in (True, False):
        out = torch.full((rows + 1, N), float("nan"), device=DEV)
        _lib_check(lib.amuse_train_linear_fwd(x.data_ptr(), W.data_ptr(), b.data_ptr() if bias else None, rows, K, N, out.data_ptr(), s))
        res[f"fwd bias={bias}"] = (out, xd @ Wd.T + (bd if bias else 0.0), x @ W.T + (b if bias else 0.0))
    for acc in (0, 1):
        dx = torch.cat([dx0, torch.full((1, K), float("nan"), device=DEV)])
        _lib_check(lib.amuse_train_linear_bwd(dy.data_ptr(), x.data_ptr(), W.data_ptr(), rows, K, N, None, None, dx.data_ptr(), acc, st["ws"].data_ptr(), s))
        res[f"dx acc={acc}"] = (dx, dyd @ Wd + (dx0.double() if acc else 0.0), dy @ W + (dx0 if acc else 0.0))
    dW, db = torch.full((N + 1, K), float("nan"), device=DEV), torch.full((N + 1,), float("nan"), device=DEV)
    _lib_check(lib.amuse_train_linear_bwd(dy.data_ptr(), x.data_ptr(), W.data_ptr(), rows, K, N, dW.data_ptr(), db.data_ptr(), None, 0, st["ws"].data_ptr(), s))
    res["dW"], res["db"] = (dW, dyd.T @ xd, dy.T @ x), (db, dyd.sum(0), dy.sum(0))
    return res


def _lib_check(rc):
    from amuse_amd import _lib
    _lib.check(rc)


# the tall projections of the 27 transformer layers (k_train_gemm_tall) | every other shape of the step on the generic kernel (k_train_gemm_any): the 333-wide
# embedding / output layers (no 16-byte rows), the Denoiser's 32-row condition projections and 160-row layers, a 1-row call, ragged everything
# (13,444 and 38,400 rows: more than 64 chunks of the weight-gradient kernel - a workgroup goes on with every 64th chunk: batches beyond 12,288 rows)
_LINEAR_SHAPES = [(9664, 128, 128), (9600, 384, 128), (9600, 512, 128), (9600, 128, 512), (9600, 128, 256), (1030, 256, 384), (1024, 128, 32),
                  (9600, 128, 333), (9600, 333, 128), (13444, 128, 128), (38400, 512, 128), (32, 128, 256), (32, 128, 128), (160, 384, 128), (160, 128, 512), (1, 5, 3), (77, 130, 67), (3000, 65, 1000)]


@pytest.mark.parametrize("rows,N,K", _LINEAR_SHAPES)
def test_linear_entry_points_against_float64_and_the_vendor_gemm(rows, N, K):
    """out = x W^T (+ b), dx (+)= dy W, dW = dy^T x and db on the library's OWN fp32-MFMA GEMMs (csrc/k_train_gemm.hip: the LDS-staged tall kernel, the generic kernel for
    every other shape - no vendor BLAS in the library) against float64, and against torch's (vendor) GEMM within fp32 summation noise; rows / columns past the end of
    the arrays are not touched; twice the same bits (ordered reductions)."""
    from amuse_amd import train_ops as T
    st = T._st(torch.device(DEV))
    a = _linear_calls(st["lib"], st, rows, N, K, rows + N + K)
    b = _linear_calls(st["lib"], st, rows, N, K, rows + N + K)
    differ = 0
    for key, (got, ref, ven) in a.items():
        n = ref.shape[0]
        assert bool(torch.isnan(got[n:]).all()), key                          # the guard row behind the array
        scale = float(ref.abs().max())
        err = float((got[:n].double() - ref).abs().max()) / scale
        assert err < 3e-6, (key, err)
        assert torch.equal(got[:n], b[key][0][:n]), key
        assert float((ven.double() - got[:n].double()).abs().max()) / scale < 1e-5, key   # (the library GEMM's own distance from float64 is up to ~5e-6)
        differ += int(not torch.equal(ven, got[:n]))
    assert differ > 0 or rows * N * K < 1000                                  # (really two implementations)


def test_linear_entry_points_take_weights_on_a_4_byte_boundary():
    """The Denoiser's weights are views into the trainer's flat parameter buffer behind the prior's 333-element bias: 4-byte aligned.  The tall kernel's LDS-DMA needs
    16 bytes; such calls run on the generic kernel - same results."""
    from amuse_amd import train_ops as T
    st = T._st(torch.device(DEV))
    for key, (got, ref, _ven) in _linear_calls(st["lib"], st, 9600, 128, 128, 77, misalign=1).items():
        n = ref.shape[0]
        assert float((got[:n].double() - ref).abs().max()) / float(ref.abs().max()) < 3e-6, key


@pytest.mark.parametrize("B,S", [(2, 300), (3, 302), (32, 5), (1, 17), (2, 304), (1, 1)])
def test_attention_kernels_against_torch_math_attention(B, S):
    """csrc/k_train_attn.hip (fp32 MFMA): o and d(q | k | v) against softmax(q k^T / sqrt(32)) v under autograd, without dropout and with the kernel's own mask."""
    from amuse_amd import train_ops as T
    g = torch.Generator(device=DEV).manual_seed(S)
    qkv = torch.randn(B * S, 384, device=DEV, generator=g)
    dout = torch.randn(B * S, 128, device=DEV, generator=g)

    def ref(mask):
        x = qkv.clone().requires_grad_(True)
        q, k, v = (t.transpose(1, 2) for t in x.view(B, S, 3, 4, 32).unbind(2))          # (B, 4, S, 32)
        p = torch.softmax(q @ k.transpose(-1, -2) / 32 ** 0.5, dim=-1)
        if mask is not None:
            p = p * mask
        o = (p @ v).transpose(1, 2).reshape(B * S, 128)
        o.backward(dout)
        return o.detach(), x.grad

    for pdrop in (0.0, 0.1):
        o, lse, mask = T.attn_fwd(qkv, B, S, pdrop, 5, 9, want_mask=True)
        if pdrop == 0.0:
            assert torch.all(mask == 1.0)
        elif B * S * S > 2000:
            kept = (mask > 0).float().mean()
            assert abs(float(kept) - 0.9) < 0.02 and torch.all((mask == 0) | ((mask - 1 / 0.9).abs() < 1e-6))
            o_b, _ = T.attn_fwd(qkv, B, S, pdrop, 5, 10)
            assert not torch.equal(o_b, o)                                               # another offset: another mask
        o_ref, g_ref = ref(None if pdrop == 0.0 else mask)
        assert float((o - o_ref).abs().max()) < 2e-5, (pdrop, float((o - o_ref).abs().max()))
        dqkv = T.attn_bwd(qkv, o, lse, dout, B, S, pdrop, 5, 9)
        assert _rel(dqkv, g_ref) < 2e-4, (pdrop, _rel(dqkv, g_ref))
        for sl in (slice(0, 128), slice(128, 256), slice(256, 384)):                      # each of dq, dk, dv on its own scale
            scale = float(g_ref[:, sl].abs().max())                                       # (one key: the softmax is constant, dq = dk = 0 exactly in the reference)
            assert float((dqkv[:, sl] - g_ref[:, sl]).abs().max()) < 2e-4 * scale + 1e-6, (pdrop, sl)



def test_two_layer_chains_on_two_streams_do_not_share_scratch():
    """Two chains of 9,600-row layers - forward AND backward, the chunked weight gradients with their split-k partials and the layers' summing launches included - in
    flight on two streams of the device at once (stream 1 registered as scratch lane 1: train_ops.register_lane; the library's workspaces exist once per lane,
    amuse_train_set_lane) give bitwise what each chain gives alone.  (The trainer's own second chain, the Denoiser's, has 160-row layers and never reaches the chunked
    weight-gradient kernel: this is the test that lane 1 of THAT workspace works.)"""
    from amuse_amd import train_ops
    B, S = 32, 300
    g = torch.Generator(device=DEV).manual_seed(5)
    chains = []
    for k in range(2):
        m = _layers("enc" if k == 0 else "dec", 2).train()
        x = torch.randn(B, S, 128, device=DEV, generator=g)
        mem = torch.randn(B, 1, 128, device=DEV, generator=g)
        dout = torch.randn(B, S, 128, device=DEV, generator=g)
        chains.append((m, x, mem, dout, k))

    def run(chain, off0):
        m, x, mem, dout, k = chain
        train_ops._OFFSET[0] = off0                     # the same dropout offsets in both runs
        xr = x.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = m(xr) if k == 0 else m(xr, mem)
        out.backward(dout)
        return [out.detach().clone(), xr.grad.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]

    torch.manual_seed(11)
    alone = [run(c, 1000 * (i + 1)) for i, c in enumerate(chains)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    train_ops.register_lane(side, 1)
    main = torch.cuda.current_stream(DEV)
    both = [None, None]
    try:
        for rep in range(3):                            # a few rounds: the two chains' launches interleave differently every time
            torch.cuda._sleep(60_000_000)               # ~25 ms on the main stream, the side stream behind it: BOTH chains are fully enqueued when they start, so they do run
            side.wait_stream(main)                      # side by side (an eager host would otherwise finish issuing one before the other begins)
            with torch.cuda.stream(side):
                both[1] = run(chains[1], 2000)
            both[0] = run(chains[0], 1000)
            main.wait_stream(side)
            torch.cuda.synchronize()
            for a, b in zip(alone, both):
                assert len(a) == len(b)
                for ta, tb in zip(a, b):
                    assert torch.equal(ta, tb)
    finally:
        train_ops._LANES.clear()


def test_refused_layer_backward_touches_nothing_and_the_next_call_is_right(eager_switch, monkeypatch):
    """A decoder layer at B = 2, S = 8, self-attention inside the call.  amuse_train_layer_bwd without its dqkv buffer is refused BEFORE its first launch: dx, dWv
    and dmem, filled with a sentinel, are bit-for-bit what they were after a stream synchronise.  The next, valid call on the same buffers - and the call the
    autograd function itself makes - give the eager layer's gradients at this file's bars (test_fused_layer_equals_the_eager_layer_in_eval_mode)."""
    import ctypes as C

    from amuse_amd import _lib, train_ops
    B, S = 2, 8
    m = _layers("dec", 1).eval()
    g = torch.Generator(device=DEV).manual_seed(2)
    x, mem, dout = (torch.randn(B, n, 128, device=DEV, generator=g) for n in (S, 1, S))

    def run(on):
        eager_switch(on)
        xr, mr = x.clone().requires_grad_(True), mem.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        m(xr, mr).backward(dout)
        return xr.grad, mr.grad, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    dx0, dm0, g0 = run(False)
    st = train_ops._st(x.device)
    real = st["lib"]
    sizes = {"dx": B * S * 128, "dWv": 128 * 128, "dmem": B * 128}
    sentinel = torch.full((max(sizes.values()),), 0x5A5A5A5A, device=DEV, dtype=torch.int32)
    mine = {n: sentinel[:k].clone() for n, k in sizes.items()}
    assert all(t.numel() == sizes[n] for n, t in mine.items())
    seen = {}

    class Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        def amuse_train_layer_bwd(self, ref, stream):
            L = _lib.TrainLayer.from_buffer_copy(ref._obj)
            for n, t in mine.items():
                setattr(L, n, t.data_ptr())
            dqkv, L.dqkv = L.dqkv, None
            seen["rc"] = real.amuse_train_layer_bwd(C.byref(L), stream)
            seen["error"] = real.amuse_last_error().decode()
            torch.cuda.current_stream(DEV).synchronize()
            seen["untouched"] = all(torch.equal(t, sentinel[:t.numel()]) for t in mine.values())
            L.dqkv = dqkv
            _lib.check(real.amuse_train_layer_bwd(C.byref(L), stream))
            return real.amuse_train_layer_bwd(ref, stream)

    monkeypatch.setitem(st, "lib", Lib())
    dx1, dm1, g1 = run(True)
    assert seen["rc"] != 0 and "self-attention buffers missing" in seen["error"], seen
    assert seen["untouched"]
    dWv0 = g0["multihead_attn.in_proj_weight"][256:]
    for got, want in ((mine["dx"].view(torch.float32).view(B, S, 128), dx0), (mine["dmem"].view(torch.float32).view(B, 1, 128), dm0),
                      (mine["dWv"].view(torch.float32).view(128, 128), dWv0), (dx1, dx0), (dm1, dm0)):
        assert _rel(got, want) < 2e-4
    assert set(g0) == set(g1)
    for n in g0:
        assert _rel(g1[n], g0[n]) < 2e-4, n
