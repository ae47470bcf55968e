"""GPU: the training step's fused transformer layers WITH DROPOUT LIVE (amuse_amd/train_ops.py on csrc/amuse_train.hip, k_train.hip, k_train_attn.hip) against a float64
reference that replays the kernels' masks.

tests/train_layer_ref.py restates the mask contract in integer arithmetic and writes the encoder / decoder layer out in float64 with a keep mask at each of the six dropout
sites; tests/test_train_layer_ref_cpu.py holds it to the eager layers and shows that a mask from a wrong offset at any one site is ten bars away while a float32 evaluation
of the same reference stays under half of every bar.  Here:

  a. every mask-drawing kernel's mask, recovered through probes, is BITWISE the restatement's - rows 1, 7, 33, F = 128 and 512, attention (1, 1), (2, 17), (1, 304), epochs
     0 and 5, a small seed and one above 2^32;
  b. fused forward + backward of nn_modules.EncoderLayer / DecoderLayer(p = 0.1).train() with torch's seed and train_ops._OFFSET pinned: out, dx, dmem and EVERY parameter
     gradient, each on its own scale, at the bars of test_fused_layer_equals_the_eager_layer_in_eval_mode (2e-5 absolute on out, 2e-4 of max |reference| per gradient) - the
     only value test of k_train_vk / k_train_dc, and of the decoder's side-stream memory branch at 1,200 rows;
  c. the raw kernels against float64 where tests/test_gpu_train_ops.py stops: ln_bwd's dgamma / dbeta / dbias / dy at p = 0.1 (also with dx, dy aliased onto dout, dout2, as the
     layer calls it), 38,437 rows (past one sweep of every capped grid, ragged), the attention's lse, its two forward instantiations against each other, the one-part
     launch at S > 64, and a peaked case whose running maximum moves from key tile to key tile.

Every test leaves the dropout epoch at 0 and train_ops' offset counter and lane table as it found them."""
import numpy as np
import pytest
import torch

import train_layer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P = 0.1
BIG_SEED = 0x0BAD_5EED_1234_5678 & 0x7FFFFFFFFFFFFFFF     # (above 2^32: the high word of the Philox key and of the attention key's product)
SEEDS = (7, BIG_SEED)


def _epoch_set(k):
    from amuse_amd import _lib, train_ops as T
    dev = torch.device(DEV)
    with T._on(dev):
        _lib.check(T._st(dev)["lib"].amuse_train_epoch_set(int(k), torch.cuda.current_stream(DEV).cuda_stream))


@pytest.fixture(autouse=True)
def clean_state():
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


def _rel(got, ref):
    """max |got - ref| / max |ref| in float64"""
    ref = ref.double()
    return float((got.double().to(ref.device) - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- a. masks, bitwise
@pytest.mark.parametrize("epoch", [0, 5])
@pytest.mark.parametrize("rows", [1, 7, 33])
def test_row_kernels_draw_the_restated_masks(rows, epoch):
    """k_train_ln_fwd / _bwd (128 columns) and k_train_bgd_fwd / _bwd (F = 128 and 512) keep exactly the restatement's elements and scale them by fp32 1 / (1 - p)."""
    from amuse_amd import train_ops as T
    _epoch_set(epoch)
    one, zero = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    scale = R.fp32_scale(P)
    for seed in SEEDS:
        for off in (3, (1 << 32) + 9):
            # LayerNorm with x = 0, y = 1, no bias: a two-level row, above its mean exactly where kept (rows with everything or nothing kept would be constant)
            want = R.row_keep(seed, off, epoch, rows, 128, P)
            assert ((want.sum(1) > 0) & (want.sum(1) < 128)).all()
            want = torch.from_numpy(want)
            out, zhat, rstd = T.ln_fwd(None, torch.ones(rows, 128, device=DEV), None, one, zero, P, seed, off)
            assert torch.equal((out > 0).cpu(), want), ("ln_fwd", seed, off)
            dx, dy, *_ = T.ln_bwd(torch.randn(rows, 128, generator=_gen(1)).to(DEV), zhat, rstd, one, P, seed, off)
            assert bool((dx != 0).all()) and torch.equal((dy != 0).cpu(), want), ("ln_bwd", seed, off)
            assert torch.equal(dy, torch.where(want.to(DEV), dx * scale, torch.zeros_like(dx)))
            # FFN activation on h = 30: gelu(h) = h, so out / 30 is keep / (1 - p)
            for F in (128, 512):
                want = torch.from_numpy(R.row_keep(seed, off, epoch, rows, F, P))
                h, b = torch.full((rows, F), 30.0, device=DEV), torch.zeros(F, device=DEV)
                a = T.bias_gelu_drop_fwd(h, b, P, seed, off)
                assert torch.equal((a > 0).cpu(), want), ("bias_gelu_drop_fwd", F, seed, off)
                assert torch.equal(a, torch.where(want.to(DEV), h * scale, torch.zeros_like(h)))
                dh, _ = T.bias_gelu_drop_bwd(torch.ones_like(h), h, b, P, seed, off)
                assert torch.equal((dh > 0).cpu(), want), ("bias_gelu_drop_bwd", F, seed, off)


@pytest.mark.parametrize("epoch", [0, 5])
@pytest.mark.parametrize("B,S", [(1, 1), (2, 17), (1, 304)])
def test_attention_kernel_draws_the_restated_mask(B, S, epoch):
    from amuse_amd import train_ops as T
    _epoch_set(epoch)
    qkv = torch.randn(B * S, 384, generator=_gen(S)).to(DEV)
    scale = torch.tensor(R.fp32_scale(P), dtype=torch.float32)
    for seed in SEEDS:
        for off in (9, (1 << 32) + 9):
            want = torch.from_numpy(R.attn_keep(seed, off, epoch, B, S, P))
            _, _, mask = T.attn_fwd(qkv, B, S, P, seed, off, want_mask=True)
            assert torch.equal((mask > 0).cpu(), want), (seed, off)
            assert torch.equal(mask.cpu(), torch.where(want, scale, torch.zeros(())))


# ---------------------------------------------------------------------------------------------------- b. layers, dropout live
def _fused(kind, m, x, mem, dout, epoch, offset=R.LAYER_OFFSET):
    from amuse_amd import train_ops as T
    m = m.to(DEV).train()
    xr, mr = x.to(DEV).requires_grad_(True), mem.to(DEV).requires_grad_(True)
    assert T.usable(xr, None) and T.own_attention(x.shape[1], 4, 128)
    m.zero_grad(set_to_none=True)
    _epoch_set(epoch)
    torch.manual_seed(R.LAYER_SEED)
    T._OFFSET[0] = offset
    out = m(xr) if kind == "enc" else m(xr, mr)
    assert T._OFFSET[0] == offset + 6                                         # five Philox sites and the self-attention, in train_layer_ref.layer_offsets' order
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return {"out": out.detach(), "dx": xr.grad, "dmem": mr.grad if kind == "dec" else None, "grads": {n: p.grad for n, p in m.named_parameters()}}


@pytest.mark.parametrize("kind,B,S,epoch", R.LAYER_CASES)
def test_fused_layer_with_dropout_live_against_the_float64_reference(kind, B, S, epoch):
    """Prints the error per tensor in units of its bar's scale (out absolute, gradients relative to max |reference|).  Measured on an MI355X: out 8.4e-7 .. 1.3e-6 over the
    five cases; at dec (4, 300) dx 2.2e-7, dmem 4.5e-7, the largest parameter gradient error 5.8e-7 (self_attn.in_proj_weight), the smallest 1.5e-7 (self_attn.out_proj.bias)."""
    m, x, mem, dout = R.layer_case(kind, B, S)
    ref = R.layer_ref(kind, m.state_dict(), x, mem, dout, R.layer_masks(epoch))
    got = _fused(kind, m, x, mem, dout, epoch)
    assert all(g is not None for g in got["grads"].values()) and len(got["grads"]) == (18 if kind == "dec" else 12)
    d = R.distances(got, ref)
    for n, v in d.items():
        print(f"{kind} ({B}, {S}) epoch {epoch}  {n:34s} {v:.3e}  (bar {R.OUT_BAR if n == 'out' else R.GRAD_BAR:.0e})")
    assert d["out"] < R.OUT_BAR, d["out"]
    bad = {n: v for n, v in d.items() if n != "out" and not v < R.GRAD_BAR}
    assert not bad, bad
    if kind == "dec":                                                         # the q / k rows of the cross-attention's in-projection take no gradient
        assert float(got["grads"]["multihead_attn.in_proj_weight"][:256].abs().max()) == 0 and float(got["grads"]["multihead_attn.in_proj_bias"][:256].abs().max()) == 0


def test_fused_layer_masks_follow_the_epoch_and_the_offset():
    """The comparison above can tell: the fused decoder layer at epoch 5, or one layer call later, is NOT within the bars of the reference at epoch 0 and the pinned offset."""
    kind, B, S = "dec", 2, 17
    m, x, mem, dout = R.layer_case(kind, B, S)
    ref = R.layer_ref(kind, m.state_dict(), x, mem, dout, R.layer_masks(0))
    for epoch, offset in ((5, R.LAYER_OFFSET), (0, R.LAYER_OFFSET + 6)):
        d = R.distances(_fused(kind, m, x, mem, dout, epoch, offset), ref)
        assert d["out"] > 10 * R.OUT_BAR and max(v for n, v in d.items() if n != "out") > 10 * R.GRAD_BAR, (epoch, offset)


# ---------------------------------------------------------------------------------------------------- c. raw kernels against float64
@pytest.mark.parametrize("rows", [7, 160, 2100])
def test_ln_bwd_with_dropout_against_float64_also_in_place(rows):
    """ln_fwd / ln_bwd at p = 0.1 (2,100 rows: more than one workgroup, two sweeps, a ragged tail): out, dx, dy, dgamma, dbeta, dbias against float64 with the restated mask at
    the bars of test_raw_kernels_against_torch; the same call with dx written over dout and dy over dout2 - the layer's own use of it - gives the same bits."""
    from amuse_amd import _lib, train_ops as T
    seed, off = BIG_SEED, 11
    g = _gen(rows)
    x, y, dout = (torch.randn(rows, 128, generator=g).to(DEV) for _ in range(3))
    bias, ga, be = (torch.randn(128, generator=g).to(DEV) for _ in range(3))
    keep = torch.from_numpy(R.row_keep(seed, off, 0, rows, 128, P)).to(DEV)
    d1, d2 = dout * 0.25, dout * 0.75
    ref = R.ln_drop_ref(x, y, bias, ga, be, keep, R.fp32_scale(P), (d1, d2))
    out, zhat, rstd = T.ln_fwd(x, y, bias, ga, be, P, seed, off)
    err = float((out.double() - ref[0]).abs().max())
    print(f"rows {rows}: ln_fwd out {err:.3e}")
    assert err < 2e-5
    got = T.ln_bwd(d1, zhat, rstd, ga, P, seed, off, dout2=d2)
    for name, a, b in zip(("dx", "dy", "dgamma", "dbeta", "dbias"), got, ref[1:]):
        print(f"rows {rows}: ln_bwd {name} {_rel(a, b):.3e}")
        assert _rel(a, b) < 2e-5, (name, _rel(a, b))
    # in place: dx = dout, dy = dout2
    a1, a2 = d1.clone(), d2.clone()
    small = torch.empty(3, 128, device=DEV)
    st = T._st(torch.device(DEV))
    with T._on(torch.device(DEV)):
        _lib.check(st["lib"].amuse_train_ln_bwd(a1.data_ptr(), a2.data_ptr(), zhat.data_ptr(), rstd.data_ptr(), ga.data_ptr(), P, seed, off, rows, a1.data_ptr(), a2.data_ptr(),
                                                small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), st["ws"].data_ptr(), torch.cuda.current_stream(DEV).cuda_stream))
    for name, a, b in zip(("dx", "dy", "dgamma", "dbeta", "dbias"), (a1, a2, small[0], small[1], small[2]), got):
        assert torch.equal(a, b), name


BIG_ROWS = 38437          # beyond one sweep of every capped grid (ln_fwd 4,096 x 8 rows; bias_gelu_drop_fwd 8,192 x 256 float4; the column-sum kernels' workgroup cap), ragged


def test_layer_norm_kernels_at_38437_rows_against_float64():
    """ln_fwd / ln_bwd with dropout live against float64 (plain torch in double on the device) with the restated mask; bars of test_raw_kernels_against_torch."""
    from amuse_amd import train_ops as T
    rows, seed, off = BIG_ROWS, BIG_SEED, 21
    g = torch.Generator(device=DEV).manual_seed(rows)
    x, y, dout = (torch.randn(rows, 128, device=DEV, generator=g) for _ in range(3))
    bias, ga, be = (torch.randn(128, device=DEV, generator=g) for _ in range(3))
    keep = torch.from_numpy(R.row_keep(seed, off, 0, rows, 128, P)).to(DEV)
    ref = R.ln_drop_ref(x, y, bias, ga, be, keep, R.fp32_scale(P), (dout,))
    out, zhat, rstd = T.ln_fwd(x, y, bias, ga, be, P, seed, off)
    err = float((out.double() - ref[0]).abs().max())
    print(f"ln_fwd out {err:.3e}")
    assert err < 2e-5
    got = T.ln_bwd(dout, zhat, rstd, ga, P, seed, off)
    for name, a, b in zip(("dx", "dy", "dgamma", "dbeta", "dbias"), got, ref[1:]):
        print(f"ln_bwd {name} {_rel(a, b):.3e}")
        assert _rel(a, b) < 2e-5, (name, _rel(a, b))


def test_ffn_activation_kernels_at_38437_rows_against_float64():
    """bias_gelu_drop_fwd / _bwd at F = 512 with dropout live against float64 with the restated mask; bars of test_raw_kernels_against_torch."""
    from amuse_amd import train_ops as T
    rows, seed, off = BIG_ROWS, BIG_SEED, 22
    g = torch.Generator(device=DEV).manual_seed(rows + 1)
    h, b1 = torch.randn(rows, 512, device=DEV, generator=g) * 2, torch.randn(512, device=DEV, generator=g)
    da = torch.randn(rows, 512, device=DEV, generator=g)
    keep = torch.from_numpy(R.row_keep(seed, off, 0, rows, 512, P)).to(DEV)
    a_ref, dh_ref, db_ref = R.gelu_drop_ref(h, b1, keep, R.fp32_scale(P), da)
    a = T.bias_gelu_drop_fwd(h, b1, P, seed, off)
    dh, db1 = T.bias_gelu_drop_bwd(da, h, b1, P, seed, off)
    ea = float((a.double() - a_ref).abs().max())
    print(f"bias_gelu_drop_fwd {ea:.3e}   bias_gelu_drop_bwd dh {_rel(dh, dh_ref):.3e} db {_rel(db1, db_ref):.3e}")
    assert ea < 2e-6 and _rel(dh, dh_ref) < 2e-6 and _rel(db1, db_ref) < 2e-5


def test_column_sums_at_38437_rows_against_float64():
    """colsum at C = 384 (in_proj's bias gradient), deterministic"""
    from amuse_amd import train_ops as T
    q = torch.randn(BIG_ROWS, 384, device=DEV, generator=torch.Generator(device=DEV).manual_seed(BIG_ROWS + 2))
    s = T.colsum(q)
    print(f"colsum {_rel(s, q.double().sum(0)):.3e}")
    assert _rel(s, q.double().sum(0)) < 1e-5 and torch.equal(s, T.colsum(q))


def _attention_against_float64(qkv, dout, B, S, seed, off, tag):
    """o, lse and d(q | k | v) of the attention kernels without and with dropout (the restated mask) against float64: o and lse 2e-5, gradients 2e-4 of the largest entry,
    each of dq, dk, dv on its own scale (the bars of test_attention_kernels_against_torch_math_attention); the training instantiation of the forward kernel (no mask
    output) gives the bits of the tests' one."""
    from amuse_amd import train_ops as T
    qd, dd = qkv.to(DEV), dout.to(DEV)
    for p in (0.0, P):
        keep = torch.from_numpy(R.attn_keep(seed, off, 0, B, S, p))
        o_ref, lse_ref, g_ref = R.attn_ref(qkv, dout, B, S, keep if p else None, R.fp32_scale(p))
        o, lse = T.attn_fwd(qd, B, S, p, seed, off)
        o_m, lse_m, mask = T.attn_fwd(qd, B, S, p, seed, off, want_mask=True)
        assert torch.equal(o, o_m) and torch.equal(lse, lse_m), (tag, p)
        assert torch.equal((mask > 0).cpu(), keep), (tag, p)
        eo, el = float((o.cpu().double() - o_ref).abs().max()), float((lse.cpu().double() - lse_ref).abs().max())
        dqkv = T.attn_bwd(qd, o, lse, dd, B, S, p, seed, off).cpu()
        print(f"{tag} p {p}: o {eo:.3e}  lse {el:.3e}  d(qkv) {_rel(dqkv, g_ref):.3e}")
        assert eo < 2e-5 and el < 2e-5, (tag, p, eo, el)
        assert _rel(dqkv, g_ref) < 2e-4, (tag, p)
        for sl in (slice(0, 128), slice(128, 256), slice(256, 384)):
            scale = float(g_ref[:, sl].abs().max())                          # (one key: the softmax is constant, dq = dk = 0 exactly in the reference)
            assert float((dqkv[:, sl].double() - g_ref[:, sl]).abs().max()) < 2e-4 * scale + 1e-6, (tag, p, sl)


@pytest.mark.parametrize("B,S", [(1, 1), (1, 17), (2, 300), (128, 65)])
def test_attention_lse_and_both_forward_instantiations(B, S):
    """(128, 65): the one-part launch at S > 64 (B x 4 workgroups already fill the chip); (2, 300): two parts, 19 tiles; a ragged single tile; one key."""
    g = _gen(1000 * B + S)
    qkv, dout = torch.randn(B * S, 384, generator=g), torch.randn(B * S, 128, generator=g)
    _attention_against_float64(qkv, dout, B, S, BIG_SEED, 9, f"({B}, {S})")


def test_attention_on_peaked_scores_with_a_moving_running_maximum():
    """train_layer_ref.peaked_case at (2, 300): q times 4 and a score ramp over the key index, ascending on head 0 (the online softmax rescales its accumulators at a third of
    its tile steps), descending on head 1 (it hardly ever does).  tests/test_train_layer_ref_cpu.py shows torch's float32 attention under half of these bars here."""
    qkv, dout = R.peaked_case()
    _attention_against_float64(qkv, dout, R.PEAKED_B, R.PEAKED_S, 5, 9, "peaked")
