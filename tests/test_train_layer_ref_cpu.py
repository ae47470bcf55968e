"""CPU: tests/train_layer_ref.py - the float64 restatement of the training step's transformer layers with the kernels' dropout masks injected - held to the eager
layers of nn_modules.py, and the two properties that make the GPU comparison (tests/test_gpu_train_layer_dropout.py) mean something:

  * sensitivity: a mask drawn at the wrong offset at ANY ONE of the six sites moves the output by at least ten times its bar and at least one parameter gradient by at
    least ten times its bar - the bars can tell a wrong mask from rounding;
  * conditioning: the same restatement evaluated in float32 with the same masks stays under HALF of every bar at every layer shape the GPU tests use - a correct fp32
    implementation has room.  This is a property of the inputs (train_layer_ref.layer_case)."""
import numpy as np
import pytest
import torch

import train_layer_ref as R

SEED = 0x0BAD_5EED_1234_5678 & 0x7FFFFFFFFFFFFFFF


def _eager(kind, m, x, mem, dout):
    m = m.double().eval()
    xr, mr = x.double().clone().requires_grad_(True), mem.double().clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m(xr) if kind == "enc" else m(xr, mr)
    out.backward(dout.double())
    return {"out": out.detach(), "dx": xr.grad, "dmem": mr.grad if kind == "dec" else None, "grads": {n: p.grad for n, p in m.named_parameters()}}


@pytest.mark.parametrize("kind,B,S", [("enc", 2, 17), ("enc", 1, 1), ("dec", 2, 17), ("dec", 3, 40)])
def test_all_keep_reference_is_the_eager_layer_in_float64(kind, B, S):
    m, x, mem, dout = R.layer_case(kind, B, S)
    want = _eager(kind, m, x, mem, dout)
    got = R.layer_ref(kind, m.state_dict(), x, mem, dout, R.AllKeep())
    assert len(got["grads"]) == (18 if kind == "dec" else 12) and all(g is not None for g in got["grads"].values())
    for n, (a, b) in {n: (R.tensors(got)[n], R.tensors(want)[n]) for n in R.tensors(want)}.items():
        rel = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
        assert a.shape == b.shape and rel < 1e-10, (n, rel)
    if kind == "dec":                                                        # the q / k rows of the cross-attention's in-projection: zero, as autograd gives them
        assert float(got["grads"]["multihead_attn.in_proj_weight"][:256].abs().max()) == 0 and float(got["grads"]["multihead_attn.in_proj_bias"][:256].abs().max()) == 0
        assert float(got["grads"]["multihead_attn.in_proj_weight"][256:].abs().max()) > 0


def test_masks_have_the_rate_of_their_probability():
    for p in (0.1, 0.25):
        for name, m in (("row 128", R.row_keep(SEED, 3, 0, 2048, 128, p)), ("row 512", R.row_keep(SEED, 4, 0, 512, 512, p)),
                        ("head", R.head_keep(SEED, 5, 0, 64, 300, 4, p)), ("attention", R.attn_keep(SEED, 6, 0, 2, 200, p))):
            n = m.size
            assert abs(float(m.mean()) - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n), (name, p, float(m.mean()))          # five standard deviations of the binomial
    assert R.row_keep(SEED, 3, 0, 7, 128, 0.0).all() and R.attn_keep(SEED, 3, 0, 1, 9, 0.0).all()
    assert abs(R.fp32_scale(0.1) - 1 / 0.9) < 1e-7 and R.philox_thr(0.1) == 1677721 and R.attn_thr(0.1) == int(float(np.float32(0.1)) * 2 ** 32)


def test_masks_change_with_seed_offset_epoch_and_site():
    offs = R.layer_offsets(100)
    assert sorted(offs.values()) == [101, 102, 103, 104, 105, 106] and offs["self"] == 106 and offs["cross"] == 105
    draws = {"row": lambda seed, off, ep: R.row_keep(seed, off, ep, 7, 128, 0.1), "head": lambda seed, off, ep: R.head_keep(seed, off, ep, 2, 17, 4, 0.1),
             "attention": lambda seed, off, ep: R.attn_keep(seed, off, ep, 2, 17, 0.1)}
    for name, f in draws.items():
        base = f(SEED, 9, 0)
        assert np.array_equal(base, f(SEED, 9, 0))
        for what, other in (("seed lo", f(SEED ^ 1, 9, 0)), ("seed hi", f(SEED ^ (1 << 40), 9, 0)), ("offset", f(SEED, 10, 0)), ("epoch", f(SEED, 9, 1)),
                            ("epoch 5", f(SEED, 9, 5))):
            assert not np.array_equal(base, other), (name, what)
    # the sites of one layer call draw six different masks (row sites compared at their common shape)
    m = R.Masks(SEED, offs)
    rows = [m(s, 2, 17).numpy() for s in ("drop1", "drop2", "drop3")]
    assert not any(np.array_equal(rows[i], rows[j]) for i in range(3) for j in range(i))
    assert m("ffn", 2, 17).shape == (2, 17, 512) and m("cross", 2, 17).shape == (2, 17, 4) and m("self", 2, 17).shape == (2, 4, 17, 17)
    # a row mask is a prefix property: element e does not depend on how many rows the call has; F = 128 and F = 512 index the same stream
    assert np.array_equal(R.row_keep(SEED, 3, 0, 33, 128, 0.1)[:7], R.row_keep(SEED, 3, 0, 7, 128, 0.1))
    assert np.array_equal(R.row_keep(SEED, 3, 0, 8, 512, 0.1).reshape(-1), R.row_keep(SEED, 3, 0, 32, 128, 0.1).reshape(-1))
    # attention: a (clip, head)'s mask does not depend on B or S
    assert np.array_equal(R.attn_keep(SEED, 3, 0, 2, 17, 0.1)[1, 2, :5, :5], R.attn_keep(SEED, 3, 0, 3, 5, 0.1)[1, 2])


def test_epoch_is_the_high_word_of_the_offset_at_the_philox_sites():
    for e in (1, 5, 0xFFFF):
        assert np.array_equal(R.row_keep(SEED, 9, e, 7, 128, 0.1), R.row_keep(SEED, 9 + (e << 32), 0, 7, 128, 0.1))
        assert np.array_equal(R.head_keep(SEED, 9, e, 2, 17, 4, 0.1), R.head_keep(SEED, 9 + (e << 32), 0, 2, 17, 4, 0.1))
        assert R.attn_key(SEED, 9, e) != R.attn_key(SEED, 9 + (e << 32), 0)       # (the attention hash mixes the epoch into its key another way)
    assert R.attn_key(SEED, 9, 0) == R.attn_key(SEED, 9, 1 << 32)                  # the epoch word has 32 bits


_REF = {}


def _ref(kind, B, S, epoch):
    """the float64 reference with the layer's masks, once per case"""
    key = (kind, B, S, epoch)
    if key not in _REF:
        m, x, mem, dout = R.layer_case(kind, B, S)
        _REF[key] = (m, x, mem, dout, R.layer_ref(kind, m.state_dict(), x, mem, dout, R.layer_masks(epoch)))
    return _REF[key]


@pytest.mark.parametrize("kind", ["enc", "dec"])
def test_a_mask_of_another_offset_at_any_one_site_is_ten_bars_away(kind):
    """At (2, 17), the smallest layer case of the GPU tests with more than one row: the fewest elements per site, so the least a wrong mask can move."""
    m, x, mem, dout, ref = _ref(kind, 2, 17, 0)
    masks = R.layer_masks(0)
    for site in (R.SITES if kind == "dec" else R.ENC_SITES):
        wrong = R.layer_ref(kind, m.state_dict(), x, mem, dout, masks.with_offset(site, masks.offsets[site] + 6))     # (the next layer call's offset for that site)
        d = R.distances(wrong, ref)
        worst = max((v, n) for n, v in d.items() if n not in ("out", "dx", "dmem"))
        print(f"{kind} {site}: out moves {d['out']:.3e} (bar {R.OUT_BAR:.0e}); parameter gradient {worst[1]} moves {worst[0]:.3e} of its max (bar {R.GRAD_BAR:.0e})")
        assert d["out"] >= 10 * R.OUT_BAR, (site, d["out"])
        assert worst[0] >= 10 * R.GRAD_BAR, (site, worst)


@pytest.mark.parametrize("kind,B,S,epoch", R.LAYER_CASES)
def test_float32_evaluation_of_the_reference_stays_under_half_of_every_bar(kind, B, S, epoch):
    m, x, mem, dout, ref = _ref(kind, B, S, epoch)
    lo = R.layer_ref(kind, m.state_dict(), x, mem, dout, R.layer_masks(epoch), dtype=torch.float32)
    d = R.distances(lo, ref)
    worst = max((v, n) for n, v in d.items() if n != "out")
    print(f"{kind} ({B}, {S}) epoch {epoch}: fp32 vs float64 out {d['out']:.3e}, worst gradient {worst[1]} {worst[0]:.3e}")
    assert d["out"] < 0.5 * R.OUT_BAR, d["out"]
    for n, v in d.items():
        if n != "out":
            assert v < 0.5 * R.GRAD_BAR, (n, v)


def test_peaked_attention_case_moves_the_running_maximum_and_leaves_room_under_the_bars():
    """train_layer_ref.peaked_case: per head, the share of steps from one 16-key tile to the next at which a query's running maximum rises; and torch's own float32
    attention against float64 on these inputs stays under half of the GPU test's bars (o 2e-5, lse 2e-5, d(qkv) 2e-4 of its largest entry)."""
    B, S = R.PEAKED_B, R.PEAKED_S
    qkv, dout = R.peaked_case()
    q, k = (qkv.double().view(B, S, 3, 4, 32)[:, :, i].transpose(1, 2) for i in (0, 1))
    tile_max = (q @ k.transpose(-1, -2))[..., :288].reshape(B, 4, S, 18, 16).amax(-1)
    run = torch.cummax(tile_max, -1).values
    moves = (run[..., 1:] > run[..., :-1]).double().mean((0, 2, 3))
    print("share of tile steps at which the running maximum moves, per head:", [round(float(v), 3) for v in moves])
    assert float(moves[0]) > 0.25 and float(moves[0]) > 2 * float(moves[2:].max()) and float(moves[1]) < 0.75 * float(moves[2:].min())
    keep = torch.from_numpy(R.attn_keep(5, 9, 0, B, S, 0.1))
    for kp in (None, keep):
        o64, l64, g64 = R.attn_ref(qkv, dout, B, S, kp, R.fp32_scale(0.1))
        o32, l32, g32 = R.attn_ref(qkv, dout, B, S, kp, R.fp32_scale(0.1), dtype=torch.float32)
        eo, el, eg = float((o32 - o64).abs().max()), float((l32 - l64).abs().max()), float((g32 - g64).abs().max() / g64.abs().max())
        print(f"peaked case, dropout {kp is not None}: fp32 vs float64 o {eo:.3e}, lse {el:.3e} (largest lse {float(l64.abs().max()):.1f}), d(qkv) {eg:.3e}")
        assert eo < 1e-5 and el < 1e-5 and eg < 1e-4
