"""GPU: what exists only for the training step replayed as HIP graphs (GestureTrainer.enable_graph), pinned to numbers.

  * the device-side optimizer - FlatAdamW.step_dev on amuse_train_adamw_dev (k_train_adamw_scalars + k_train_adamw_dev, csrc/k_train.hip) - against the float64
    restatement of tests/train_ref.py (itself pinned to torch.optim.AdamW by tests/test_train_ref_cpu.py): every range length at which the launch changes shape
    (one thread, a ragged workgroup, one full grid of 16,384 x 256 threads, one full grid plus a ragged second pass of the grid-stride loop), the `advance`
    protocol over two ranges, the two bias-correction scalars, the host <-> device hand-over of the step count, and a captured step_dev();
  * the device-side dropout epoch (amuse_train_epoch_set / _advance) in the kernels that train the model - ln_fwd / ln_bwd, bias_gelu_drop_fwd / _bwd, the attention
    kernels, and the decoder layer's k_train_vk / k_train_dc through train_ops.decoder_layer;
  * the captured step itself, dropout live: forward + losses + backward into the bucket as one graph, step_dev() + the epoch advance as a second one, replayed three
    times against the same three calls made eagerly on a twin trainer - BITWISE (same kernels, same operands, same masks, ordered reductions);
  * a capture that fails while its second graph is recorded: the trainer is left as it was, bitwise a twin that never tried, and can still be captured.

The bar of the optimizer tests is this project's own 2e-6 of the largest entry (tests/test_gpu_train_ops.py test_flat_adamw_equals_torch_adamw_and_keeps_its_state_layout),
at lr 3e-3 and weight decay 0.01: one skipped or doubled update is ~1e-3 of the largest parameter away.  Every test leaves the epoch at 0 and train_ops' host-side offset
counter and lane table as it found them."""
import contextlib

import numpy as np
import pytest
import torch

import train_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, WD, BETAS, EPS = 3e-3, 0.01, (0.9, 0.999), 1e-8
BAR = 2e-6
FULL_GRID = 16384 * 256                    # launch_train_adamw / launch_train_adamw_dev: the grid is capped at 16,384 workgroups of 256 threads
P, SEED, OFF = 0.1, 7, 3                   # the layer kernels' dropout probability, seed and call offset


# ---------------------------------------------------------------------------------------------------- helpers
def _lib_stream():
    from amuse_amd import train_ops as T
    return T._st(torch.device(DEV))["lib"], torch.cuda.current_stream(DEV).cuda_stream


def _epoch_set(k):
    from amuse_amd import _lib, train_ops as T
    lib, stream = _lib_stream()
    with T._on(torch.device(DEV)):
        _lib.check(lib.amuse_train_epoch_set(int(k), stream))


@contextlib.contextmanager
def _clean_state():
    """The epoch back to 0 on the way out, whatever happened; train_ops' host-side offset counter and lane table as they were."""
    from amuse_amd import train_ops as T
    off, lanes = T._OFFSET[0], dict(T._LANES)
    try:
        yield
    finally:
        T._OFFSET[0] = off
        T._LANES.clear()
        T._LANES.update(lanes)
        _epoch_set(0)
        torch.cuda.synchronize()


_PROBE = {}


def _read_epoch(limit=8):
    """The dropout epoch of the device, read through a small layer call: bias_gelu_drop_fwd on 8 x 512 large positive values keeps exactly the mask; the mask at
    the ambient epoch is compared with the masks of epochs 0 .. limit - 1, which by the documented encoding are the epoch-0 masks at offset OFF + (e << 32) -
    computed once (the first call pins the epoch to 0 for that and must come while it is 0)."""
    from amuse_amd import train_ops as T
    if not _PROBE:
        _PROBE["h"], _PROBE["b"] = torch.full((8, 512), 30.0, device=DEV), torch.zeros(512, device=DEV)
        _epoch_set(0)
        _PROBE["table"] = [T.bias_gelu_drop_fwd(_PROBE["h"], _PROBE["b"], P, SEED, OFF + (e << 32)) > 0 for e in range(limit)]
        assert all(not torch.equal(_PROBE["table"][0], t) for t in _PROBE["table"][1:])
    got = T.bias_gelu_drop_fwd(_PROBE["h"], _PROBE["b"], P, SEED, OFF) > 0
    hits = [e for e, t in enumerate(_PROBE["table"]) if torch.equal(t, got)]
    assert len(hits) == 1, hits
    return hits[0]


def _rel64(got, ref):
    """max |got - ref| / max |ref| with got a device tensor and ref a float64 array"""
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


class _Ref:
    """The float64 twin of a FlatAdamW: the whole flat buffers, stepped over the optimizer's ranges only."""

    def __init__(self, opt):
        self.ranges = [tuple(r) for r in opt._ranges]
        self.p = opt._p.detach().cpu().numpy().astype(np.float64)
        self.m, self.v, self.t = np.zeros_like(self.p), np.zeros_like(self.p), 0

    def step(self, flat_g):
        g = flat_g.detach().cpu().numpy().astype(np.float64)
        self.t += 1
        for off, n in self.ranges:
            s = slice(off, off + n)
            self.p[s], self.m[s], self.v[s] = train_ref.adamw_ref(self.p[s], g[s], self.m[s], self.v[s], self.t, LR, BETAS, EPS, WD)

    def errors(self, opt, ranges=None):
        out = {}
        for off, n in ranges or self.ranges:
            s = slice(off, off + n)
            for name, got, ref in (("p", opt._p, self.p), ("m", opt._m, self.m), ("v", opt._v, self.v)):
                out[name] = max(out.get(name, 0.0), _rel64(got[s], ref[s]))
        return out


def _guarded(n, seed):
    """One optimizer range of n elements at offset 1 of n + 2-element flat buffers: a NaN guard element on either side in all four buffers."""
    from amuse_amd.train_ops import FlatAdamW
    g = torch.Generator(device=DEV).manual_seed(seed)
    flat_p, flat_g = torch.randn(n + 2, device=DEV, generator=g), torch.zeros(n + 2, device=DEV)
    p = torch.nn.Parameter(flat_p[1:n + 1])
    p.grad = flat_g[1:n + 1]
    opt = FlatAdamW([p], flat_p, flat_g, [(p, 1, n)], lr=LR)
    assert opt._ranges == [[1, n]] and opt.param_groups[0]["weight_decay"] == WD and tuple(opt.param_groups[0]["betas"]) == BETAS and opt.param_groups[0]["eps"] == EPS
    for t in (flat_p, flat_g, opt._m, opt._v):
        t[0] = t[n + 1] = float("nan")
    return g, flat_p, flat_g, opt


def _small(seed, skip_middle=False):
    """The layouts of tests/test_gpu_train_ops.py: _flat_setup's four parameters, or - skip_middle - the five of the step() test with the third one (the trainer's
    never-reached mem_pos.pe) outside the optimizer: two ranges."""
    from amuse_amd.train_ops import FlatAdamW
    g = torch.Generator(device=DEV).manual_seed(seed)
    shapes = [(128, 128), (128,), (500, 1, 128), (384, 128), (7,)] if skip_middle else [(128, 128), (128,), (384, 128), (7,)]
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
    skip = params[2] if skip_middle else None
    opt = FlatAdamW([p for p in params if p is not skip], flat_p, flat_g, layout, lr=LR)
    return g, n, flat_p, flat_g, opt, (layout[2] if skip_middle else None)


def _check(ref, opt, what, ranges=None):
    err = ref.errors(opt, ranges)
    print(f"[adamw] {what}: largest errors relative to the largest entry: p {err['p']:.3e}, m {err['m']:.3e}, v {err['v']:.3e} (bar {BAR:.0e})")
    for name, e in err.items():
        assert e < BAR, (what, name, e)


# ---------------------------------------------------------------------------------------------------- 2. the device-side optimizer
@pytest.mark.parametrize("path,n", [("dev", 1), ("dev", 3), ("dev", 255), ("dev", 256), ("dev", 257), ("dev", FULL_GRID), ("dev", FULL_GRID + 257),
                                    ("host", FULL_GRID), ("host", FULL_GRID + 257)])
def test_adamw_range_lengths_against_float64(path, n):
    """Five steps with fresh gradients over one range of n elements - step_dev() (k_train_adamw_scalars + k_train_adamw_dev), and for the two lengths that fill the
    capped grid also step() (k_train_adamw: the same grid-stride loop) - against tests/train_ref.py: p, m and v within 2e-6 of their largest entry, the NaN guard
    element on either side of the range still NaN in all four buffers."""
    with _clean_state():
        g, flat_p, flat_g, opt = _guarded(n, n % 1000 + 1)
        ref = _Ref(opt)
        for it in range(5):
            flat_g[1:n + 1] = torch.randn(n, device=DEV, generator=g)
            opt.step_dev() if path == "dev" else opt.step()
            ref.step(flat_g)
        _check(ref, opt, f"{path} n = {n}")
        for t in (flat_p, flat_g, opt._m, opt._v):
            assert bool(torch.isnan(t[0])) and bool(torch.isnan(t[n + 1])) and bool(torch.isfinite(t[1:n + 1]).all())
        assert int(opt._t_dev) == (5 if path == "dev" else 0) and opt._t == (0 if path == "dev" else 5)


def test_adamw_dev_advances_the_step_once_per_step_over_two_ranges():
    """A skipped parameter in the middle: two ranges, two launches per step_dev().  The first advances the device-side count and writes the scalars, the second
    reads them: after k calls the count is k, both ranges are at the reference's step k, and the skipped parameter, its moments included, is untouched."""
    with _clean_state():
        g, n, flat_p, flat_g, opt, (skip, soff, sn) = _small(0, skip_middle=True)
        assert len(opt._ranges) == 2
        ref = _Ref(opt)
        before = flat_p[soff:soff + sn].clone()
        k = 4
        for it in range(k):
            flat_g.copy_(torch.randn(n, device=DEV, generator=g))
            opt.step_dev()
            ref.step(flat_g)
            assert int(opt._t_dev) == it + 1
        assert int(opt._t_dev) == k
        assert torch.equal(flat_p[soff:soff + sn], before) and torch.equal(skip.detach().view(-1), before)
        assert float(opt._m[soff:soff + sn].abs().max()) == 0.0 and float(opt._v[soff:soff + sn].abs().max()) == 0.0
        for r in range(2):                                      # each range on its own scale
            _check(ref, opt, f"two ranges, range {r} after {k} steps", [ref.ranges[r]])
        assert float(opt.state_dict()["state"][0]["step"]) == float(k)


@pytest.mark.parametrize("t0", [0, 999, 99_999])
def test_adamw_dev_scalars_within_one_float32_ulp(t0):
    """push_step() at host count t0, one step_dev(): the device holds t0 + 1 and scal = {lr / (1 - b1^t), 1 / sqrt(1 - b2^t)} at t = t0 + 1, each within ONE float32
    ulp - a relative 2^-23, which no float two steps away meets - of the double value rounded to float32: the device's double pow may differ from the host's in its
    last bits, which moves the float32 rounding by at most one step."""
    with _clean_state():
        g, flat_p, flat_g, opt = _guarded(3, 5)
        opt._t = t0
        opt.push_step()
        flat_g[1:4] = torch.randn(3, device=DEV, generator=g)
        opt.step_dev()
        assert int(opt._t_dev) == t0 + 1
        got = opt._scal.cpu().numpy().astype(np.float64)
        want = [float(np.float32(s)) for s in train_ref.adamw_scalars(t0 + 1, LR, BETAS)]
        ulps = [abs(a - b) / float(np.spacing(np.float32(b))) for a, b in zip(got, want)]
        print(f"[adamw] scalars at t = {t0 + 1}: device {got[0]!r}, {got[1]!r}; float32 of the double value {want[0]!r}, {want[1]!r}; distance {ulps[0]:g}, {ulps[1]:g} ulp")
        for a, b in zip(got, want):
            assert abs(a - b) <= 2.0 ** -23 * abs(b), (t0, a, b)


def test_adamw_step_count_hand_over_between_host_and_device():
    """step() x 3, push_step(), step_dev() x 2, sync_step(), step(): six steps of the reference; the host's count follows the device's and state_dict() reports 6."""
    with _clean_state():
        g, n, flat_p, flat_g, opt, _ = _small(3)
        ref = _Ref(opt)

        def one(fn):
            flat_g.copy_(torch.randn(n, device=DEV, generator=g))
            fn()
            ref.step(flat_g)
        for _ in range(3):
            one(opt.step)
        opt.push_step()
        assert int(opt._t_dev) == 3
        for _ in range(2):
            one(opt.step_dev)
        assert opt._t == 3 and int(opt._t_dev) == 5
        opt.sync_step()
        assert opt._t == 5
        one(opt.step)
        assert opt._t == 6 and ref.t == 6
        _check(ref, opt, "3 step + 2 step_dev + 1 step")
        assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {6.0}


def test_adamw_dev_inside_a_graph():
    """One captured step_dev(), replayed three times with new gradients copied into the static bucket: every replay is the NEXT step (the count and the bias
    corrections live on the device).  Warm-up: one eager call, which the reference takes too; the capture itself runs nothing."""
    with _clean_state():
        g, n, flat_p, flat_g, opt, _ = _small(4)
        ref = _Ref(opt)
        flat_g.copy_(torch.randn(n, device=DEV, generator=g))
        opt.step_dev()
        ref.step(flat_g)
        torch.cuda.synchronize()
        held = [t.clone() for t in (flat_p, opt._m, opt._v, opt._t_dev)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step_dev()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(held, (flat_p, opt._m, opt._v, opt._t_dev)))
        for r in range(3):
            flat_g.copy_(torch.randn(n, device=DEV, generator=g))
            graph.replay()
            ref.step(flat_g)
            assert int(opt._t_dev) == 2 + r
        _check(ref, opt, "1 eager + 3 replayed step_dev")
        del graph


# ---------------------------------------------------------------------------------------------------- 3. the dropout epoch in the layer kernels
def _philox_calls(rows):
    """{name: callable(off) -> tuple of every output} of the four Philox kernels on fixed random operands, and {name: callable(outputs) -> kept set}"""
    from amuse_amd import train_ops as T
    g = torch.Generator(device=DEV).manual_seed(rows)
    x, y, dout = (torch.randn(rows, 128, device=DEV, generator=g) for _ in range(3))
    bias, ga, be = (torch.randn(128, device=DEV, generator=g) for _ in range(3))
    zhat, rstd = torch.randn(rows, 128, device=DEV, generator=g), torch.rand(rows, device=DEV, generator=g) + 0.5
    ones, one, zero = torch.ones(rows, 128, device=DEV), torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    calls = {"ln_fwd": lambda off: T.ln_fwd(x, y, bias, ga, be, P, SEED, off),
             "ln_fwd two-level": lambda off: T.ln_fwd(None, ones, None, one, zero, P, SEED, off),      # x = 0, y = 1: out > 0 where kept
             "ln_bwd": lambda off: T.ln_bwd(dout, zhat, rstd, ga, P, SEED, off)}
    kept = {"ln_fwd two-level": lambda o: o[0] > 0, "ln_bwd": lambda o: o[1] != 0}
    return calls, kept


def _ffn_calls(rows=160, F=512):
    from amuse_amd import train_ops as T
    g = torch.Generator(device=DEV).manual_seed(F)
    h, da, b = torch.randn(rows, F, device=DEV, generator=g) * 2, torch.randn(rows, F, device=DEV, generator=g), torch.randn(F, device=DEV, generator=g)
    calls = {"bias_gelu_drop_fwd": lambda off: (T.bias_gelu_drop_fwd(h, b, P, SEED, off),),
             "bias_gelu_drop_bwd": lambda off: T.bias_gelu_drop_bwd(da, h, b, P, SEED, off)}
    kept = {"bias_gelu_drop_fwd": lambda o: o[0] != 0, "bias_gelu_drop_bwd": lambda o: o[0] != 0}
    return calls, kept


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("rows", [1, 7, 160])
def test_epoch_is_the_high_word_of_the_offset_in_the_philox_kernels(rows):
    """ln_fwd, ln_bwd, bias_gelu_drop_fwd, bias_gelu_drop_bwd (the latter two at 160 rows, F = 512): a call at epoch e with offset off is BITWISE - every output - the
    call at epoch 0 with offset off + (e << 32); epoch 0 is bitwise what the call gave before this test touched the epoch; at e != 0 the kept set is another."""
    with _clean_state():
        calls, kept = _philox_calls(rows)
        if rows == 160:
            c2, k2 = _ffn_calls()
            calls.update(c2), kept.update(k2)
        first = {n: f(OFF) for n, f in calls.items()}                       # before any epoch call of this test (every test leaves the epoch at 0)
        for e in (1, 3, 0xFFFF):
            _epoch_set(e)
            at_e = {n: f(OFF) for n, f in calls.items()}
            _epoch_set(0)
            for n, f in calls.items():
                assert _same(at_e[n], f(OFF + (e << 32))), (n, e)
                assert _same(first[n], f(OFF)), (n, e)
                assert not _same(at_e[n], first[n]), (n, e)
                if n in kept:
                    assert not torch.equal(kept[n](at_e[n]), kept[n](first[n])), (n, e)


def test_backward_kernels_regenerate_the_forward_masks_at_the_same_epoch():
    """The constructions of test_dropout_masks_are_regenerated_by_the_backward_kernels (tests/test_gpu_train_ops.py) at epoch 5, on 512 rows: the backward kernel's
    kept set is the forward kernel's.  Forward at epoch 5 and backward at epoch 6 do NOT agree (the comparison can tell epochs apart)."""
    from amuse_amd import train_ops as T
    with _clean_state():
        rows, p = 512, P
        one, zero, zero512 = torch.ones(128, device=DEV), torch.zeros(128, device=DEV), torch.zeros(512, device=DEV)
        h = torch.full((rows, 512), 30.0, device=DEV)                      # gelu(h) = h: out / h is the mask / (1 - p)
        y = torch.ones(rows, 128, device=DEV)                              # x = 0, y = 1: a two-level row, high where kept
        dout = torch.randn(rows, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        _epoch_set(5)
        a = T.bias_gelu_drop_fwd(h, zero512, p, 7, 3)
        m = a / 30.0
        kept = m > 0
        assert float((m[kept] - 1 / (1 - p)).abs().max()) < 1e-6
        dh, db = T.bias_gelu_drop_bwd(torch.ones_like(h), h, zero512, p, 7, 3)
        assert torch.equal(dh > 0, kept) and float((dh[kept] - 1 / (1 - p)).abs().max()) < 1e-5
        assert float((db - dh.sum(0)).abs().max() / dh.sum(0).abs().max()) < 1e-5
        out, zhat, rstd = T.ln_fwd(None, y, None, one, zero, p, 7, 5)
        keptl = out > 0
        ref = torch.nn.functional.layer_norm(keptl.float() / (1 - p), (128,))
        ok = keptl.float().sum(1) < 128                                    # (a row with nothing dropped is constant: LayerNorm of it is 0 / eps)
        assert float((out - ref)[ok].abs().max()) < 1e-4
        dx, dy, *_ = T.ln_bwd(dout, zhat, rstd, one, p, 7, 5)
        assert torch.equal(dy != 0, keptl & (dx != 0)) and float((dy - dx * keptl / (1 - p)).abs().max()) < 1e-6
        assert 0 < int(kept.sum()) < kept.numel() and 0 < int(keptl.sum()) < keptl.numel()
        _epoch_set(6)                                                      # the backward pass one epoch later: other masks
        dh6, _ = T.bias_gelu_drop_bwd(torch.ones_like(h), h, zero512, p, 7, 3)
        assert not torch.equal(dh6 > 0, kept)
        dx6, dy6, *_ = T.ln_bwd(dout, zhat, rstd, one, p, 7, 5)
        assert torch.equal(dx6, dx) and not torch.equal(dy6 != 0, keptl & (dx6 != 0))
        _epoch_set(0)                                                      # ... and neither are they epoch 0's
        assert not torch.equal(T.bias_gelu_drop_fwd(h, zero512, p, 7, 3) > 0, kept)
        assert not torch.equal(T.ln_fwd(None, y, None, one, zero, p, 7, 5)[0] > 0, keptl)


@pytest.mark.parametrize("B,S", [(2, 17), (1, 33), (2, 304)])
def test_attention_kernels_at_epoch_5(B, S):
    """k_attn_fwd / k_attn_bwd at epoch 5 (a ragged last tile, three key tiles, the full 19): o and d(q | k | v) against autograd on softmax(q k^T / sqrt(32)) . mask v
    with the mask the forward kernel reports, at the bars of test_attention_kernels_against_torch_math_attention - a backward kernel that drew its mask at another
    epoch misses them; the epoch-5 mask is not epoch 0's; epoch 0 after epoch 5 gives the bits of the first epoch-0 call."""
    from amuse_amd import train_ops as T
    with _clean_state():
        g = torch.Generator(device=DEV).manual_seed(S)
        qkv = torch.randn(B * S, 384, device=DEV, generator=g)
        dout = torch.randn(B * S, 128, device=DEV, generator=g)

        def ref(mask):
            x = qkv.clone().requires_grad_(True)
            q, k, v = (t.transpose(1, 2) for t in x.view(B, S, 3, 4, 32).unbind(2))          # (B, 4, S, 32)
            o = ((torch.softmax(q @ k.transpose(-1, -2) / 32 ** 0.5, dim=-1) * mask) @ v).transpose(1, 2).reshape(B * S, 128)
            o.backward(dout)
            return o.detach(), x.grad

        def run():
            o, lse, mask = T.attn_fwd(qkv, B, S, P, 5, 9, want_mask=True)
            return o, lse, mask, T.attn_bwd(qkv, o, lse, dout, B, S, P, 5, 9)

        first = run()                                                                        # epoch 0
        _epoch_set(5)
        o, lse, mask, dqkv = run()
        assert torch.all((mask == 0) | ((mask - 1 / (1 - P)).abs() < 1e-6)) and 0 < int((mask == 0).sum()) < mask.numel() // 2
        assert not torch.equal(mask, first[2])
        o_ref, g_ref = ref(mask)
        assert float((o - o_ref).abs().max()) < 2e-5, float((o - o_ref).abs().max())
        for sl in (slice(0, 128), slice(128, 256), slice(256, 384)):                         # each of dq, dk, dv on its own scale
            scale = float(g_ref[:, sl].abs().max())
            err = float((dqkv[:, sl] - g_ref[:, sl]).abs().max())
            assert err < 2e-4 * scale + 1e-6, (sl, err, scale)
        _, g_first = ref(first[2])                                                           # (the bars tell the two epochs' gradients apart)
        assert float((g_first - g_ref).abs().max()) > 100 * 2e-4 * float(g_ref.abs().max())
        _epoch_set(0)
        assert _same(run(), first)


def _decoder_layer(seed):
    from amuse_amd import nn_modules as nm
    torch.manual_seed(seed)
    m = nm.DecoderLayer(p=P).to(DEV)
    for q in m.parameters():                                                # non-trivial LayerNorm parameters and biases (tests/test_gpu_train_ops.py _layers)
        if q.dim() == 1:
            q.data.normal_(1.0 if q.data.mean() > 0.5 else 0.0, 0.2)
    return m


def test_decoder_layer_follows_the_epoch():
    """train_ops.decoder_layer at B = 2, S = 8 in train mode - the way to k_train_vk / k_train_dc (the one-key cross-attention's dropout and its backward), which have
    no raw wrapper: with the host-side offsets reset before each run, two runs at epoch 5 give bitwise the same output and gradients, the epoch-5 output is not epoch
    0's, and at epoch 5 the directional derivative of test_fused_layer_in_train_mode_is_consistent_and_unbiased holds at that test's bar - in x, and in the memory
    token, whose gradient passes through k_train_dc."""
    from amuse_amd import train_ops as T
    with _clean_state():
        m = _decoder_layer(3).train()
        g = torch.Generator(device=DEV).manual_seed(4)
        x, mem = torch.randn(2, 8, 128, device=DEV, generator=g), torch.randn(2, 1, 128, device=DEV, generator=g)
        w = torch.randn(2, 8, 128, device=DEV, generator=g)
        dirx, dirm = torch.randn(2, 8, 128, device=DEV, generator=g), torch.randn(2, 1, 128, device=DEV, generator=g)

        def fwd(xin, memin):
            T._OFFSET[0] = 1000
            return T.decoder_layer(m, xin, memin)

        def fwd_bwd():
            xr, mr = x.clone().requires_grad_(True), mem.clone().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            out = fwd(xr, mr)
            (out * w).sum().backward()
            return [out.detach(), xr.grad, mr.grad] + [q.grad.clone() for q in m.parameters() if q.grad is not None]

        at0 = fwd_bwd()
        _epoch_set(5)
        a, b = fwd_bwd(), fwd_bwd()
        assert len(a) > 10 and _same(a, b)
        assert not torch.equal(a[0], at0[0])
        assert torch.equal(fwd(x, mem).detach(), a[0])
        eps = 1e-2
        for name, dx, dm, an in (("x", dirx, torch.zeros_like(dirm), float((a[1] * dirx).sum().double())),
                                 ("mem", torch.zeros_like(dirx), dirm, float((a[2] * dirm).sum().double()))):
            fd = float(((fwd(x + eps * dx, mem + eps * dm) - fwd(x - eps * dx, mem - eps * dm)).detach() * w).sum().double()) / (2 * eps)
            print(f"[decoder layer, epoch 5] d/d{name}: finite difference {fd:.6f}, analytic {an:.6f}")
            assert abs(fd - an) < 2e-2 * max(1.0, abs(an)), (name, fd, an)
        _epoch_set(0)
        assert _same(fwd_bwd(), at0)


# ---------------------------------------------------------------------------------------------------- 4. the captured step against the eager step
def _draws(B, g):
    return dict(noise=torch.randn(B, 1, 128, generator=g).to(DEV), timesteps=torch.randint(0, 1000, (B,), generator=g).to(DEV),
                eps_enc=torch.randn(1, B, 128, generator=g).to(DEV), eps_inf=torch.randn(1, B, 128, generator=g).to(DEV))


_TENSOR_KEYS = ("ld_motion", "ld_audio_con", "ld_audio_emo", "ld_audio_sty")


def test_captured_step_equals_the_eager_step_bit_for_bit():
    """Two trainers from identical arguments (batch 4, the gradient sink, dropout 0.1 LIVE, the default HIP inner sampler, the Denoiser's and the sampler's streams on):
    G replays the step as two graphs - forward_losses + backward_into_bucket | step_dev + amuse_train_epoch_advance, captured by GestureTrainer._capture, the routine
    enable_graph runs, with the test's draws as its static ones so that every draw stays explicit - and E makes the same three calls eagerly at the epoch pinned to the
    replay's number.  After each of three replays on three different batches the loss, the gradient bucket, the parameters, both moments and the device-side step count
    are BITWISE equal.

    Explicit draws: noise, timesteps and both rsample draws are device tensors (copied into G's static ones per replay); prior.encode's own rsample() still runs, its
    value is overwritten.  Dropout masks: seed = torch's initial seed, offsets from train_ops' host-side counter - pinned to the same value before the capture and before
    each eager step - and the device-side epoch.  The sampler's initial latents: the shipped capture draws them from torch's device generator (graph_safe), so E's sampler
    is switched to the same source and the generator is seeded alike before each replay and each eager step (a replay starts from the generator's state of that moment, as
    an eager step does); the clip counter stays pinned for the warm-up steps.

    The epoch is G's own: after every replay it is read through a small layer call (and must have advanced by one), E pins it for its step, and it is put back to the
    value read.  Control: E's forward + backward on replay 1's operands at epoch 0 instead of 1 does NOT give G's loss or bucket."""
    from amuse_amd import train_gesture as tg, train_ops as T
    dev = torch.device(DEV)
    B, K, CLIP = 4, 5000, 64
    with _clean_state():
        assert _read_epoch() == 0
        torch.manual_seed(21)                                               # (torch.initial_seed() keys the layer kernels' masks: one value for both trainers)
        gen = torch.Generator().manual_seed(5)
        warm = (tg.synthetic_batch(B, 30, dev), _draws(B, gen))
        work = [(tg.synthetic_batch(B, 40 + r, dev), _draws(B, gen)) for r in range(3)]
        G, E = (tg.build_trainer(dev, seed=4, use_hip_sampler=True, inner="eval", dropout=P, grads_mode="sink") for _ in range(2))
        torch.set_grad_enabled(True)

        def pin(tr):
            T._OFFSET[0] = K
            tr.inner_sampler.clip_counter = CLIP

        def state(tr):
            return [tr.flat_param, tr.lpdm_opt._m, tr.lpdm_opt._v, tr.lpdm_opt._t_dev]

        # two identical eager warm-up steps on both (workspaces, streams and the sampler's re-pack path exist before the capture)
        for tr in (G, E):
            assert tr.grads_mode == "sink" and tr.inner_sampler is not None and not tr.inner_sampler.dropout
            for _ in range(2):
                pin(tr)
                tr.train_step(warm[0], **warm[1])
            tr.lpdm_opt.push_step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(state(G), state(E))) and int(G.lpdm_opt._t_dev) == 2        # the precondition
        assert G._den_stream is not None and G._side_stream is not None and E._den_stream is not None and E._side_stream is not None

        # the capture on G: the trainer's own routine, the warm-up batch and draws as its static tensors
        pin(G)
        torch.cuda.synchronize()
        held = [t.clone() for t in state(G)]
        count0 = G.lpdm_losses.count
        assert G._capture(warm[0], **warm[1]) and G._graph is not None
        g1, g2, static, sdraws, loss_g = (G._graph[k] for k in ("g1", "g2", "static", "draws", "loss"))
        assert set(sdraws) == set(warm[1]) and all(static[k].data_ptr() != warm[0][k].data_ptr() for k in _TENSOR_KEYS)
        assert G.lpdm_losses.count == count0 and G.inner_sampler.graph_safe
        E.inner_sampler.graph_safe = True
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(held, state(G)))        # a capture runs nothing
        assert _read_epoch() == 0

        def eager(batch, ex, epoch, step, seed):
            pin(E)
            _epoch_set(epoch)
            torch.cuda.manual_seed(seed)
            l = E.forward_losses(batch, **ex)
            E.backward_into_bucket(l)
            if step:
                E.lpdm_opt.step_dev()
            return l.detach()

        _epoch_set(0)
        losses = []
        for r, (batch, ex) in enumerate(work):
            for k in _TENSOR_KEYS:
                static[k].copy_(batch[k])
            for k, v in ex.items():
                sdraws[k].copy_(v)
            torch.cuda.manual_seed(900 + r)
            g1.replay()
            g2.replay()
            torch.cuda.synchronize()
            after = _read_epoch()
            assert after == r + 1                                            # the second graph advanced G's epoch by one
            if r == 1:                                                       # the control: the same operands at epoch 0 - other masks, another loss and bucket
                l0 = eager(batch, ex, 0, step=False, seed=900 + r)
                torch.cuda.synchronize()
                assert not torch.equal(l0, loss_g) and not torch.equal(E.flat_grad, G.flat_grad)
            le = eager(batch, ex, r, step=True, seed=900 + r)
            _epoch_set(after)
            junk = torch.randn(3_000_000, device=dev).mul_(2)                # an eager allocation between replays
            junk2 = [torch.empty(1 << k, device=dev) for k in range(8, 22)]
            del junk, junk2
            torch.cuda.synchronize()
            assert torch.equal(le, loss_g), (r, float(le), float(loss_g))
            assert torch.equal(E.flat_grad, G.flat_grad), (r, float((E.flat_grad - G.flat_grad).abs().max()))
            for name, a, b in zip(("flat_param", "_m", "_v", "_t_dev"), state(G), state(E)):
                assert torch.equal(a, b), (r, name)
            assert int(G.lpdm_opt._t_dev) == 3 + r
            assert float((G.flat_grad != 0).float().mean()) > 0.9            # the bucket really is filled
            assert bool(torch.isfinite(G.flat_param).all())
            losses.append(float(loss_g))
        print(f"[captured step] losses of the three replays {losses}: loss, bucket, parameters, moments and step count bitwise the eager trainer's")
        assert len(set(losses)) == 3 and all(np.isfinite(losses))
        assert _read_epoch() == 3
        G.lpdm_opt.sync_step()
        assert G.lpdm_opt._t == 5
        del g1, g2
        G._graph = None


def test_enable_graph_moves_step_count_epoch_and_loss_count_by_one_per_replay():
    """GestureTrainer.enable_graph itself (dropout 0): one replayed train_step moves the device-side step count, the dropout epoch and lpdm_losses.count by exactly one."""
    from amuse_amd import train_gesture as tg
    dev = torch.device(DEV)
    with _clean_state():
        assert _read_epoch() == 0
        torch.manual_seed(22)
        tr = tg.build_trainer(dev, seed=4, use_hip_sampler=True, dropout=0.0, grads_mode="sink")
        batches = [tg.synthetic_batch(4, 50 + i, dev) for i in range(3)]
        for i in range(2):
            tr.train_step(batches[i])
        assert tr.enable_graph(batches[2]) and tr._graph is not None and tr._graph["draws"] == {}
        torch.cuda.synchronize()
        assert int(tr.lpdm_opt._t_dev) == 2 and tr.lpdm_losses.count == 2 and _read_epoch() == 0      # a capture runs nothing
        for r in range(2):
            before = tr.flat_param.clone()
            loss = float(tr.train_step(batches[r]))
            assert np.isfinite(loss) and not torch.equal(before, tr.flat_param)
            assert int(tr.lpdm_opt._t_dev) == 3 + r and tr.lpdm_losses.count == 3 + r and _read_epoch() == 1 + r
        tr._graph = None


def test_a_capture_that_fails_leaves_the_trainer_as_it_was():
    """Atomic failure of GestureTrainer.capture_or_stay_eager.  Two trainers from identical arguments (batch 4, grads_mode "steal", dropout 0.1 live, the default HIP
    sampler), two identical warm-up steps.  On A the optimizer's step_dev is replaced by a function that raises a Python RuntimeError before it launches anything: the
    first graph is recorded whole (its forked streams joined), the failure comes while the second is being recorded.  Then
      * the policy method answers (False, note) with the exception's text in the note, nothing ran (parameters, moments, step count, epoch as before), and _graph,
        grads_mode, steal, the sampler's graph_safe and call count, the loss count and the optimizer's host and device step counts are what they were;
      * the next eager step with explicit draws is BITWISE - loss, bucket, parameters, moments - that of N, which never tried (the layer kernels' host-side mask offset
        and the sampler's clip counter are pinned before either step, as in the bit-for-bit test above: they are streams of draws, not trainer state);
      * a real enable_graph on A then succeeds and a replay is one more iteration."""
    from amuse_amd import train_gesture as tg, train_ops as T
    dev = torch.device(DEV)
    B, K, CLIP = 4, 7000, 32
    with _clean_state():
        assert _read_epoch() == 0
        torch.manual_seed(23)
        gen = torch.Generator().manual_seed(6)
        work = [(tg.synthetic_batch(B, 60 + i, dev), _draws(B, gen)) for i in range(3)]
        A, N = (tg.build_trainer(dev, seed=4, use_hip_sampler=True, inner="eval", dropout=P, grads_mode="steal") for _ in range(2))

        def step(tr, batch, ex):
            T._OFFSET[0] = K
            tr.inner_sampler.clip_counter = CLIP
            return tr.train_step(batch, **ex)

        def facts(tr):
            return (tr._graph, tr.grads_mode, tr.steal, tr.inner_sampler.graph_safe, tr.inner_sampler.calls, tr.lpdm_losses.count, tr.lpdm_opt._t, int(tr.lpdm_opt._t_dev))

        def tensors(tr):
            return [tr.flat_param, tr.flat_grad, tr.lpdm_opt._m, tr.lpdm_opt._v]

        for tr in (A, N):
            for _ in range(2):
                step(tr, *work[0])
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(tensors(A), tensors(N)))
        before, held = facts(A), [t.clone() for t in tensors(A)]
        assert before[:4] == (None, "steal", True, False) and before[5:7] == (2, 2) and A.inner_sampler.mode == "eval"

        def no_step():
            raise RuntimeError("injected: the optimizer step cannot be recorded")
        A.lpdm_opt.step_dev = no_step
        try:
            captured, note = A.capture_or_stay_eager(work[0][0])
        finally:
            del A.lpdm_opt.step_dev
        torch.cuda.synchronize()
        print(f"[failed capture] {note}")
        assert captured is False and "capture failed (RuntimeError: injected: the optimizer step cannot be recorded)" in note
        assert facts(A) == before and _read_epoch() == 0
        assert all(torch.equal(a, b) for a, b in zip(held, tensors(A)))

        la, ln = step(A, *work[1]), step(N, *work[1])
        torch.cuda.synchronize()
        assert torch.equal(la, ln), (float(la), float(ln))
        for name, a, b in zip(("flat_param", "flat_grad", "_m", "_v"), tensors(A), tensors(N)):
            assert torch.equal(a, b), name
        assert facts(A)[1:] == facts(N)[1:] and A.lpdm_opt._t == 3

        assert A.enable_graph(work[2][0]) and A._graph is not None and A.grads_mode == "sink" and not A.steal
        p0 = A.flat_param.clone()
        loss = float(A.train_step(work[2][0]))
        torch.cuda.synchronize()
        assert np.isfinite(loss) and not torch.equal(p0, A.flat_param)
        assert int(A.lpdm_opt._t_dev) == 4 and A.lpdm_losses.count == 4 and _read_epoch() == 1
        A._graph = None
