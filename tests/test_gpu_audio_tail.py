"""GPU: the tail of AST_EVP behind the three encoders (include/amuse_hip.h "Audio model metrics"; csrc/k_audio_tail.hip, csrc/amuse_audio_tail.hip):
classifier heads, fusion + decoder back to a 1024 x 128 fbank, and AudioEngine.metrics = AST_EVP.eval_func(metrics=True).

Where the bars come from (none is measured on the code under test):
  * the skinny GEMM (amuse_debug_tail_gemm and the last Linear of reconstruct).  An EMULATION repeats the kernel's rounding points - operands rounded to
    bf16, or split into fp16 hi / lo with the lo.lo products dropped - and accumulates in float64.  Against it every output must be within
    K * 2^-24 * sum_k |x_k w_k| (the rounded operands' products): the bound of a K-term fp32 summation in any order.  Against plain float64 the worst output
    and the relative L2 must be within 4 x the emulation's own deviation from float64 (the rule of tests/test_gpu_audio_attn_rescale.py);
  * the fp32 trunk against stock torch modules in float64: max(1e-5, 4 x (torch's own fp32 CPU forward against its float64 one)) x max|ref|, 1e-5 being the
    project's parity bar;
  * the labels against float64 from the GPU's own block-11 tap: 1e-5 x max|ref|.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PRECS = {"bf16": 1, "fp32x": 2}


# ------------------------------------------------------------------------------------------------ shared helpers
def _round_ops(x: torch.Tensor, prec: str):
    """the kernel's operand rounding of an fp32 tensor -> list of float64 pieces (bf16: [x_r]; fp32x: [hi, lo])"""
    x = x.float()
    if prec == "bf16":
        return [x.bfloat16().double()]
    hi = x.half()
    lo = (x - hi.float()).half()
    return [hi.double(), lo.double()]


def _emulate(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, prec: str):
    """-> (emulation in float64 accumulation, sum of the products' magnitudes) for out = A . W^T + bias"""
    a, w = _round_ops(A, prec), _round_ops(W, prec)
    if prec == "bf16":
        emu = a[0] @ w[0].T
        mag = a[0].abs() @ w[0].abs().T
    else:   # Wl.xh + Wh.xl + Wh.xh, lo.lo dropped
        emu = a[0] @ w[1].T + a[1] @ w[0].T + a[0] @ w[0].T
        mag = a[0].abs() @ w[1].abs().T + a[1].abs() @ w[0].abs().T + a[0].abs() @ w[0].abs().T
    return emu + bias.double(), mag


def _check_gemm(got: torch.Tensor, A, W, bias, prec, tag):
    """the two bars of the module docstring for out = A . W^T + bias; W may be given in column chunks through a callable"""
    K = A.shape[1]
    got = got.double()
    ref = A.double() @ W.double().T + bias.double()
    emu, mag = _emulate(A, W, bias, prec)
    d_emu = (got - emu).abs()
    bound = K * U * mag
    worst = float((d_emu / bound.clamp_min(1e-300)).max())
    dev = (emu - ref).abs()
    err = (got - ref).abs()
    l2_got, l2_emu = float(torch.linalg.vector_norm(got - ref) / torch.linalg.vector_norm(ref)), float(torch.linalg.vector_norm(emu - ref) / torch.linalg.vector_norm(ref))
    print(f"[audio tail] {tag} {prec}: |got - emulation| / (K u sum|xw|) max {worst:.3f} (bar 1); vs float64 max {float(err.max()):.3e} (bar 4 x {float(dev.max()):.3e}), "
          f"rel-L2 {l2_got:.3e} (bar 4 x {l2_emu:.3e})")
    return worst, float(err.max()), float(dev.max()), l2_got, l2_emu


def _assert_gemm(stats, tag):
    worst, emax, dmax, l2g, l2e = stats
    assert worst <= 1.0, (tag, worst)
    assert emax <= 4 * dmax and l2g <= 4 * l2e, (tag, emax, dmax, l2g, l2e)


def _pack(lib, W: torch.Tensor, prec: str) -> torch.Tensor:
    N, K = W.shape
    w = np.ascontiguousarray(W.numpy(), dtype=np.float32)
    out = np.empty(N * K * (2 if prec == "fp32x" else 1), dtype=np.uint16)
    assert lib.amuse_debug_tail_pack(w.ctypes.data_as(C.c_void_p), N, K, PRECS[prec], out.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(out.view(np.int16)).cuda()


def _tail_gemm(lib, A, Wp, bias, N, prec):
    B, K = A.shape
    out = torch.full((B, N), float("nan"), device="cuda", dtype=torch.float32)
    rc = lib.amuse_debug_tail_gemm(C.c_void_p(A.data_ptr()), C.c_void_p(Wp.data_ptr()), C.c_void_p(bias.data_ptr()), B, N, K, PRECS[prec],
                                   C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.amuse_last_error()
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 1. the skinny GEMM alone
GEMM_SHAPES = [(256, 64), (1024, 1024), (256 * 1031, 128)]   # one span / both chunk depths / a prime span count above any workgroup count (unequal shares)
GEMM_B = (1, 5, 16, 17, 33)                                  # one row, a partial tile, a full tile, two tiles, a second pass


@pytest.fixture(scope="module")
def lib():
    from amuse_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("prec", ["bf16", "fp32x"])
@pytest.mark.parametrize("N,K", GEMM_SHAPES)
def test_skinny_gemm_against_emulation_and_float64(lib, N, K, prec):
    g = torch.Generator().manual_seed(1000 + N % 997 + K)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = 0.1 * torch.randn(N, generator=g)
    A = torch.randn(max(GEMM_B), K, generator=g)
    Wp, Ad, bd = _pack(lib, W, prec), A.cuda(), bias.cuda()
    outs = {B: _tail_gemm(lib, Ad[:B].contiguous(), Wp, bd, N, prec).cpu() for B in GEMM_B}
    stats = {B: _check_gemm(outs[B], A[:B], W, bias, prec, f"gemm N {N} K {K} B {B}") for B in GEMM_B}
    for B in GEMM_B:
        assert bool(torch.isfinite(outs[B]).all()), B
        _assert_gemm(stats[B], (N, K, B, prec))
    # a row's bits do not depend on its batch: the first rows of every batch size agree, and a row run alone (B = 1) is its row of the largest batch
    big = outs[max(GEMM_B)]
    for B in GEMM_B:
        assert torch.equal(outs[B], big[:B]), B
    for b in (4, 15, 16, 32):
        alone = _tail_gemm(lib, Ad[b:b + 1].contiguous(), Wp, bd, N, prec).cpu()
        assert torch.equal(alone[0], big[b]), b


# ------------------------------------------------------------------------------------------------ the engine + the torch restatement of the tail
class _Fusion(nn.Module):      # AST_EVP.py FusionBlock
    def __init__(self, d, out, n=2):
        super().__init__()
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(d_model=d, nhead=4) for _ in range(n)])
        self.norm = nn.LayerNorm(d)
        self.fc = nn.Linear(d, out)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return self.fc(self.norm(x))


class _DecodeTrunk(nn.Module):   # AST_EVP.py DecoderBlock up to the last Linear's input (projection.2 is compared on its own, in column chunks)
    def __init__(self, d, n=4):
        super().__init__()
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(d_model=d, nhead=4) for _ in range(n)])
        self.norm = nn.LayerNorm(d)
        self.projection = nn.Sequential(nn.Linear(d, 2 * d), nn.ReLU())

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return self.projection(self.norm(x))


class _Trunk(nn.Module):
    def __init__(self):
        super().__init__()
        self.fusion = _Fusion(768, 512)
        self.decode = _DecodeTrunk(512)

    def forward(self, con, emo, sty, group):
        x = torch.cat((emo, sty, con), dim=-1)
        # the reference hands the layers a 2-D tensor: one unbatched sequence whose tokens are the rows
        return torch.cat([self.decode(self.fusion(x[i:i + group])) for i in range(0, x.shape[0], group)])


def _wave(n=16000, seed=3):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    return (0.3 * torch.sin(2 * np.pi * 220 * t) + 0.05 * torch.randn(n, generator=g))[None]


@pytest.fixture(scope="module")
def env():
    from amuse_amd import audio_weights as aw
    from amuse_amd.audio import AudioEngine
    sds = {n: aw.make_ast_weights(0, n) for n in aw.ENCODERS}
    tail = aw.make_ast_tail_weights(0)
    eng = AudioEngine(sds["con"], sds["emo"], sds["sty"], "cuda:0")
    g = torch.Generator().manual_seed(7)
    fb = 0.5 * torch.randn(2, 1024, 128, generator=g)
    wave = _wave()
    # the encoders' bits BEFORE any tail exists (test_encoders_unmoved_by_the_tail)
    before = {"encode": {n: eng.encode(n, fb).cpu() for n in aw.ENCODERS}, "features": [t.cpu() for t in eng.features(wave)]}
    eng.set_tail(tail)
    trunk = _Trunk().eval()
    missing = trunk.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in tail.items()
                                     if (k.startswith("fusion.") or k.startswith("decode.")) and not k.startswith("decode.projection.2")}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    yield {"eng": eng, "sds": sds, "tail": tail, "fb": fb, "wave": wave, "before": before, "trunk32": trunk, "trunk64": _copy64(trunk)}
    eng.close()


def _copy64(m):
    import copy
    return copy.deepcopy(m).double()


def _embeddings(B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 256, generator=g) for _ in range(3)]   # con, emo, sty


# ------------------------------------------------------------------------------------------------ 2. the trunk
TRUNK_CASES = [(6, 1), (6, 3), (6, 6), (16, 16), (17, 1)]   # (B, group); 17 rows cross a 16-row tile of the last Linear


@pytest.fixture(scope="module")
def trunk_runs(env):
    """every case once: the GPU's hidden vector, torch's float64 and fp32 CPU forwards"""
    runs = {}
    with torch.no_grad():
        for B, S in TRUNK_CASES:
            con, emo, sty = _embeddings(B, 100 + B)
            got = env["eng"]._tail_hidden(con, emo, sty, S).cpu()
            ref = env["trunk64"](con.double(), emo.double(), sty.double(), S)
            t32 = env["trunk32"](con, emo, sty, S)
            runs[(B, S)] = (got, ref, t32)
    return runs


@pytest.mark.parametrize("B,S", TRUNK_CASES)
def test_trunk_hidden_against_torch_float64(trunk_runs, B, S):
    got, ref, t32 = trunk_runs[(B, S)]
    assert got.shape == (B, 1024) and bool(torch.isfinite(got).all())
    scale = float(ref.abs().max())
    own = float((t32.double() - ref).abs().max()) / scale
    err = float((got.double() - ref).abs().max()) / scale
    bar = max(1e-5, 4 * own)
    print(f"[audio tail] trunk B {B} group {S}: max error / max|ref| {err:.3e} (bar {bar:.3e}; torch fp32 against float64 {own:.3e}), max|ref| {scale:.3f}")
    assert err <= bar, (B, S, err, bar)
    if S > 1 and B == 6:   # the rows of a group DO attend to each other: the same rows as single clips give something else
        assert not torch.equal(got, trunk_runs[(6, 1)][0])


def test_trunk_groups_do_not_influence_each_other(env):
    eng = env["eng"]
    con, emo, sty = _embeddings(6, 106)
    base = eng._tail_hidden(con, emo, sty, 3).cpu()
    con2, emo2, sty2 = con.clone(), emo.clone(), sty.clone()
    emo2[4] += 1.0   # a row of the second group
    moved = eng._tail_hidden(con2, emo2, sty2, 3).cpu()
    assert torch.equal(moved[:3], base[:3]) and not torch.equal(moved[3:], base[3:])
    # ... and a group's bits depend on nothing but the group: alone, behind other groups, in a call of 33 groups (two passes of 30 + 3 rows)
    alone = eng._tail_hidden(con[3:], emo[3:], sty[3:], 3).cpu()
    assert torch.equal(alone, base[3:])
    rep = [t[3:].repeat(11, 1) for t in (con, emo, sty)]
    many = eng._tail_hidden(*rep, 3).cpu()
    assert torch.equal(many, base[3:].repeat(11, 1))


# ------------------------------------------------------------------------------------------------ 3. the full reconstruction
@pytest.mark.parametrize("prec", ["bf16", "fp32x"])
@pytest.mark.parametrize("B,S", [(3, 1), (4, 2)])
def test_full_reconstruct_against_float64(env, B, S, prec):
    """All 131072 outputs of every row: the last Linear on the GPU's own hidden vector (the trunk is held to float64 above), in column chunks."""
    eng = env["eng"]
    con, emo, sty = _embeddings(B, 200 + B)
    eng.set_precision(prec)
    try:
        out = eng.reconstruct(con, emo, sty, group=S)
        hid = eng._tail_hidden(con, emo, sty, S).cpu()
    finally:
        eng.set_precision("bf16")
    assert out.shape == (B, 1024, 128) and bool(torch.isfinite(out).all())
    flat = out.cpu().reshape(B, 1024 * 128)   # [b][h][w] with f = 128 h + w
    W = torch.from_numpy(np.asarray(env["tail"]["decode.projection.2.weight"]))
    bias = torch.from_numpy(np.asarray(env["tail"]["decode.projection.2.bias"]))
    worst, num_g, num_e, den, emax, dmax = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    step = 16384
    for c in range(0, W.shape[0], step):
        Wc, bc, got = W[c:c + step], bias[c:c + step], flat[:, c:c + step].double()
        ref = hid.double() @ Wc.double().T + bc.double()
        emu, mag = _emulate(hid, Wc, bc, prec)
        worst = max(worst, float(((got - emu).abs() / (1024 * U * mag).clamp_min(1e-300)).max()))
        emax, dmax = max(emax, float((got - ref).abs().max())), max(dmax, float((emu - ref).abs().max()))
        num_g += float(((got - ref) ** 2).sum()); num_e += float(((emu - ref) ** 2).sum()); den += float((ref ** 2).sum())
    l2g, l2e = (num_g / den) ** 0.5, (num_e / den) ** 0.5
    print(f"[audio tail] reconstruct B {B} group {S} {prec}: |got - emulation| / (K u sum|xw|) max {worst:.3f} (bar 1); vs float64 max {emax:.3e} (bar 4 x {dmax:.3e}), "
          f"rel-L2 {l2g:.3e} (bar 4 x {l2e:.3e})")
    _assert_gemm((worst, emax, dmax, l2g, l2e), (B, S, prec))
    # the layout: row h of the fbank is outputs 128 h .. 128 h + 127
    assert torch.equal(out[1, 5].cpu(), flat[1, 5 * 128:6 * 128])


# ------------------------------------------------------------------------------------------------ 4. the labels
def _ln64(x, w, b, eps):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], torch.from_numpy(np.array(w)).double(), torch.from_numpy(np.array(b)).double(), eps)


def _lin64(x, w, b):
    return x @ torch.from_numpy(np.array(w)).double().T + torch.from_numpy(np.array(b)).double()


def _labels64(env, which, hid, frame_based, feature=None):
    """ASTModel.forward behind the blocks (audio_main_new.py:191-204) in float64 from the block-11 residual stream; `feature` overrides the feature the
    non-frame-based head starts from"""
    sd, tail = env["sds"][which], env["tail"]
    x = _ln64(hid.double(), sd["v.norm.weight"], sd["v.norm.bias"], 1e-6)
    x_dist = (x[:, 0] + x[:, 1]) / 2
    head = lambda v: _lin64(_ln64(v, sd["feature_head.0.weight"], sd["feature_head.0.bias"], 1e-5), sd["feature_head.1.weight"], sd["feature_head.1.bias"])
    t = lambda name: tail[f"{which}_enc.{name}"]
    if frame_based:
        feat = head(x[:, 2:].mean(dim=1))
        lab = _lin64(_ln64(x_dist, t("mlp_head_featbased.0.weight"), t("mlp_head_featbased.0.bias"), 1e-5), t("mlp_head_featbased.1.weight"), t("mlp_head_featbased.1.bias"))
    else:
        feat = head(x_dist) if feature is None else feature.double()
        lab = _lin64(_ln64(feat, t("mlp_head.0.weight"), t("mlp_head.0.bias"), 1e-5), t("mlp_head.1.weight"), t("mlp_head.1.bias"))
    return feat, lab


@pytest.mark.parametrize("prec", ["fp32x", "bf16"])
@pytest.mark.parametrize("which", ["emo", "sty"])
def test_labels_against_float64_from_the_block11_tap(env, which, prec):
    """fp32x: final norm, pooling, feature head and classifier head are all fp32 behind the tap - features and labels of both poolings within 1e-5 x max.
    bf16: the feature head rounds its operands to bf16 (the encoders' contract), so mlp_head - which starts from the feature - is held to float64 FROM THE
    GPU'S FEATURE; mlp_head_featbased starts from the fp32 final norm and is held to the whole chain as in fp32x."""
    eng, fb = env["eng"], env["fb"]
    L = {"emo": 8, "sty": 30}[which]
    eng.set_precision(prec)
    try:
        _, hid = eng.encode(which, fb, tap_block=11)
        res = {flag: tuple(t.cpu() for t in eng.encode_labels(which, fb, flag)) for flag in (True, False, None)}
        plain = eng.encode(which, fb).cpu()
    finally:
        eng.set_precision("bf16")
    hid = hid.cpu()
    assert torch.equal(res[None][0], plain) and torch.equal(res[True][0], plain)       # the engine is frame-based: feat_out is amuse_audio_encode's, bit for bit
    assert torch.equal(res[None][1], res[True][1])
    for flag in (True, False):
        feat, lab = res[flag]
        assert lab.shape == (2, L) and bool(torch.isfinite(lab).all())
        rf, rl = _labels64(env, which, hid, flag, feature=feat if (prec == "bf16" and not flag) else None)
        el = float((lab.double() - rl).abs().max() / rl.abs().max())
        ef = float((feat.double() - rf).abs().max() / rf.abs().max())
        print(f"[audio tail] labels {which} {prec} frame_based {flag}: logits max / max {el:.3e} (bar 1e-5), feature {ef:.3e}" + (" (bar 1e-5)" if prec == "fp32x" else ""))
        assert el <= 1e-5, (which, prec, flag, el)
        if prec == "fp32x":
            assert ef <= 1e-5, (which, flag, ef)
    assert not torch.equal(res[True][1], res[False][1])


def test_content_encoder_has_no_labels(env):
    eng, fb = env["eng"], env["fb"].cuda()
    feat, lab = eng.encode_labels("con", fb)
    assert lab is None and torch.equal(feat.cpu(), env["before"]["encode"]["con"])
    dummy = torch.zeros(2, 30, device="cuda")
    out = torch.zeros(2, 256, device="cuda")
    rc = eng.lib.amuse_audio_encode_labels(eng.ctx, 0, -1, C.c_void_p(fb.data_ptr()), 2, C.c_void_p(out.data_ptr()), C.c_void_p(dummy.data_ptr()), None)
    assert rc == -1 and b"content" in eng.lib.amuse_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(dummy.abs().max()) == 0.0    # nothing was launched


# ------------------------------------------------------------------------------------------------ 5. composition and isolation
def test_metrics_is_the_composition_of_its_parts(env):
    eng, fb = env["eng"], env["fb"][:1]
    m = eng.metrics(fb)
    assert set(m) == {"fbanks", "emo", "sty", "con", "new_emo", "new_sty", "new_con"}
    assert m["fbanks"].shape == (1024, 128)
    for k, L in (("emo", 8), ("sty", 30), ("con", None)):
        for pre in ("", "new_"):
            d = m[pre + k]
            assert set(d) == {"feature", "predicted_labels"} and d["feature"].shape == (256,)
            assert (d["predicted_labels"] is None) if L is None else (d["predicted_labels"].shape == (1, L))
        f1, l1 = eng.encode_labels(k, fb, True)                     # the first pass is frame-based
        assert torch.equal(m[k]["feature"], f1[0]) and (l1 is None or torch.equal(m[k]["predicted_labels"], l1))
        f2, l2 = eng.encode_labels(k, m["fbanks"][None])            # the second: the reconstruction as it is, the engine's flag
        assert torch.equal(m["new_" + k]["feature"], f2[0]) and (l2 is None or torch.equal(m["new_" + k]["predicted_labels"], l2))
    rec = eng.reconstruct(m["con"]["feature"], m["emo"]["feature"], m["sty"]["feature"], group=1)
    assert torch.equal(rec[0], m["fbanks"])


def test_encoders_unmoved_by_the_tail(env):
    """amuse_audio_encode / amuse_audio_features: the same bits before set_tail (taken by the fixture), after it, and after a reconstruct call."""
    from amuse_amd import audio_weights as aw
    eng = env["eng"]
    for again in range(2):
        for n in aw.ENCODERS:
            assert torch.equal(eng.encode(n, env["fb"]).cpu(), env["before"]["encode"][n]), (again, n)
        for a, b in zip(eng.features(env["wave"]), env["before"]["features"]):
            assert torch.equal(a.cpu(), b), again
        eng.reconstruct(*_embeddings(2, 5), group=2)


def test_bf16_reconstruct_survives_a_round_trip_through_fp32x(env):
    eng = env["eng"]
    e = _embeddings(5, 9)
    assert eng.precision == "bf16"
    r1 = eng.reconstruct(*e, group=5).cpu()
    eng.set_precision("fp32x")
    try:
        rx = eng.reconstruct(*e, group=5).cpu()
    finally:
        eng.set_precision("bf16")
    r2 = eng.reconstruct(*e, group=5).cpu()
    assert torch.equal(r1, r2) and not torch.equal(rx, r1)
    # the same function in both arithmetics: two operands rounded to 2^-9 relative over 1024 random-sign terms leave ~2^-8 of a typical output, far inside 5 % of the largest
    assert float((rx - r1).abs().max()) < 0.05 * float(rx.abs().max())
