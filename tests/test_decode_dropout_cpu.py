"""CPU: train-mode decode (amuse_set_decode_dropout) - the symbol, its argument checks, the contract in the header, the trainer's option without a GPU, and the
restatement of the mask contract that tests/test_gpu_decode_dropout.py holds the kernels to, itself held to the reference's own MotionPrior module
(tests/golden/decode_dropout.npz, written by tools/gen_decode_dropout_golden.py: the module in train() mode with these masks injected).

The contract, restated here on its own.  MotionPrior.decode runs nine TransformerDecoderLayer.forward_post blocks (layer l = 0..8 in execution order: input
blocks 0-3, middle block, output blocks 0-3) on S = 300 rows; each has six dropout sites:
    s = 0  self-attention probabilities (after the softmax)   element e = (h S + q) S + k      [4 S S elements]
    s = 1  dropout1 on the self-attention out_proj + bias     e = q 128 + f
    s = 2  cross-attention probabilities (one key: exactly 1) e = h S + q
    s = 3  dropout2 on the cross-attention out_proj + bias    e = q 128 + f
    s = 4  dropout(gelu(linear1))                             e = q 512 + f
    s = 5  dropout3 on linear2 + bias                         e = q 128 + f
Element e of site s of layer l of global clip c takes draw e % 4 of Philox4x32-10(key = seed (lo, hi); counter = (c, 0x80000000 | (8 l + s), e / 4, 2 + epoch));
keep <=> (draw >> 8) >= (uint32)(p 2^24); kept values times 1 / (1 - p) in fp32."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
S, H, DH, D, FF = 300, 4, 32, 128, 512
SITE_ELEMS = {0: H * S * S, 1: S * D, 2: H * S, 3: S * D, 4: S * FF, 5: S * D}
SITE_SHAPE = {0: (H, S, S), 1: (S, D), 2: (H, S), 3: (S, D), 4: (S, FF), 5: (S, D)}
BLOCKS = [f"decoder.input_blocks.{i}" for i in range(4)] + ["decoder.middle_block"] + [f"decoder.output_blocks.{i}" for i in range(4)]
# fp32 distance allowed between the restatement and the reference module: the bar tests/test_oracle_golden.py gives the eval restatement against the module's decode
REF_BAR = 2e-5


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def thr_scale(p):
    p32 = np.float32(p)
    return int(p32 * np.float32(16777216.0)), float(np.float32(1.0) / (np.float32(1.0) - p32))


def keep_mask(seed, clips, layer, site, epoch, p):
    """bool tensor (B, *SITE_SHAPE[site]) of the clips' keep masks at one (layer, site)."""
    from oracle import amuse_oracle as orc
    thr, _ = thr_scale(p)
    clips = np.asarray(clips, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    n4 = SITE_ELEMS[site] // 4                      # (every site's element count is a multiple of 4: one Philox call = elements 4 i .. 4 i + 3)
    ctr = np.zeros((len(clips), n4, 4), dtype=np.uint64)
    ctr[..., 0] = clips[:, None]
    ctr[..., 1] = np.uint64(0x80000000 | (8 * layer + site))
    ctr[..., 2] = np.arange(n4, dtype=np.uint64)[None]
    ctr[..., 3] = np.uint64((2 + epoch) & 0xFFFFFFFF)
    draws = orc.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(len(clips), -1)
    keep = (draws >> np.uint64(8)) >= np.uint64(thr)
    return torch.from_numpy(keep.reshape(len(clips), *SITE_SHAPE[site]))


class Masks:
    """mask(l, s) -> keep tensor, drawn when asked for (site 0 of a 70-clip batch is 25 M elements per layer); scale = 1 / (1 - p)."""

    def __init__(self, seed, clips, epoch, p):
        self.seed, self.clips, self.epoch, self.p = seed, clips, epoch, p
        self.scale = thr_scale(p)[1]

    def __call__(self, layer, site):
        return keep_mask(self.seed, self.clips, layer, site, self.epoch, self.p)


class AllKeep:
    scale = 1.0

    def __call__(self, layer, site):
        return None


def _drop(x, keep, scale):
    return x if keep is None else torch.where(keep, x * scale, torch.zeros_like(x))


def dec_block_drop(ops, x, z, W, p, key_mask, masks, l):
    """oracle dec_block (TransformerDecoderLayer.forward_post with a one-token memory) with the six dropout sites."""
    from oracle import amuse_oracle as orc
    B = x.shape[0]
    pa = p + ".self_attn"
    qkv = ops.lin(x, W[pa + ".in_proj_weight"], W[pa + ".in_proj_bias"])
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    q = q * math.sqrt(1.0 / DH)
    sh = lambda t: t.reshape(B, S, H, DH).permute(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    sc = ops.mm(q, k.transpose(-1, -2))
    if key_mask is not None:
        sc = sc.masked_fill(~key_mask[:, None, None, :], float("-inf"))
    att = _drop(torch.softmax(sc, dim=-1), masks(l, 0), masks.scale)                       # site 0: AFTER the softmax normalised
    o = ops.mm(att, v).permute(0, 2, 1, 3).reshape(B, S, D)
    y = _drop(ops.lin(o, W[pa + ".out_proj.weight"], W[pa + ".out_proj.bias"]), masks(l, 1), masks.scale)   # site 1
    x = orc.layer_norm(x + y, W[p + ".norm1.weight"], W[p + ".norm1.bias"])
    # cross-attention onto the one memory token: the softmax over one key is 1, site 2 makes it 0 or 1 / (1 - p) per (head, query)
    pc = p + ".multihead_attn"
    vz = ops.lin(z, W[pc + ".in_proj_weight"][2 * D:], W[pc + ".in_proj_bias"][2 * D:])     # (B, 128)
    prob = _drop(torch.ones(B, H, S, dtype=x.dtype), masks(l, 2), masks.scale)              # (B, H, S)
    heads = prob.permute(0, 2, 1)[..., None] * vz.reshape(B, 1, H, DH)                      # (B, S, H, 32): probability . v_h
    y = _drop(ops.lin(heads.reshape(B, S, D), W[pc + ".out_proj.weight"], W[pc + ".out_proj.bias"]), masks(l, 3), masks.scale)   # site 3
    x = orc.layer_norm(x + y, W[p + ".norm2.weight"], W[p + ".norm2.bias"])
    h = _drop(ops.act(ops.lin(x, W[p + ".linear1.weight"], W[p + ".linear1.bias"])), masks(l, 4), masks.scale)                   # site 4
    y = _drop(ops.lin(h, W[p + ".linear2.weight"], W[p + ".linear2.bias"]), masks(l, 5), masks.scale)                            # site 5
    return orc.layer_norm(x + y, W[p + ".norm3.weight"], W[p + ".norm3.bias"])


def decode_restated(Wp, z, lengths, masks, emulate=None):
    """oracle.vae_decode (MotionPrior.decode) on S = 300 rows with the dropout sites; emulate = None | "bf16" | "fp16" (the oracle's 16-bit models).
    masks: Masks(...) or AllKeep()."""
    from oracle import amuse_oracle as orc
    ops = orc.Ops(emulate is not None, poly_gelu=emulate is not None, fp16=emulate == "fp16")
    B = z.shape[0]
    lengths = [S] * B if lengths is None else list(lengths)
    valid = torch.arange(S)[None, :] < torch.tensor(lengths)[:, None]
    km = None if bool(valid.all()) else valid
    x = torch.zeros(B, S, D, dtype=z.dtype) + Wp["query_pos_decoder.pe"][:S, 0][None]
    layer = iter(range(9))
    x = orc.skip_stack(ops, x, Wp, "decoder", lambda h, name: dec_block_drop(ops, h, z, Wp, name, km, masks, next(layer)))
    feats = ops.lin(x, Wp["final_layer.weight"], Wp["final_layer.bias"])
    return feats * valid[..., None].to(feats.dtype)


def fixture_cases():
    """[(name, lengths, {clip: (frames, expected)})] of decode_dropout.npz + its inputs.  The fixture holds every frame of one clip per case and every
    `stride`-th frame of the other two."""
    g = np.load(GOLDEN / "decode_dropout.npz")
    st = int(g["stride"])
    thin = np.arange(0, S, st)
    rag = [int(v) for v in g["lengths_ragged"]]
    cases = [("full", None, {0: (np.arange(S), g["full_clip0"]), 1: (thin, g["full_thin12"][0]), 2: (thin, g["full_thin12"][1])}),
             ("ragged", rag, {1: (np.arange(rag[1]), g["ragged_clip1"]), 0: (thin, g["ragged_thin02"][0]), 2: (thin, g["ragged_thin02"][1])})]
    meta = dict(z=torch.from_numpy(g["z"]), clips=[int(c) for c in g["clips"]], p=float(g["p"]), seed=int(g["seed"]), epoch=int(g["epoch"]))
    return cases, meta


def fixture_distance(feats, expect):
    """max |difference| of a (3, 300, 333) result to one fixture case."""
    feats = np.asarray(feats)
    return max(float(np.abs(feats[c][fr] - want).max()) for c, (fr, want) in expect.items())


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_declared():
    from amuse_amd import _lib
    lib = _lib.load()
    assert "amuse_set_decode_dropout" in _lib.EXPORTS and hasattr(lib, "amuse_set_decode_dropout")
    hdr = (REPO / "include/amuse_hip.h").read_text()
    assert re.search(r"int amuse_set_decode_dropout\(amuse_ctx\* ctx, float p, uint64_t seed, uint64_t clip_index0\);", hdr)
    assert re.search(r"int amuse_set_sample_dropout\(amuse_ctx\* ctx, float p, uint64_t seed\);", hdr)        # (untouched)
    assert int(re.search(r"#define AMUSE_ABI_VERSION (\d+)", hdr).group(1)) == 5 and lib.amuse_abi_version() == 5


@pytest.mark.parametrize("p", [float("nan"), -0.1, 1.0, 1.5, float("inf")])
def test_bad_probability_is_einval(p):
    from amuse_amd import _lib
    lib = _lib.load()
    assert lib.amuse_set_decode_dropout(None, p, 1, 0) == -1          # AMUSE_EINVAL
    assert b"dropout probability" in lib.amuse_last_error()


def test_null_context_is_einval():
    from amuse_amd import _lib
    lib = _lib.load()
    for p in (0.0, 0.1, 0.999):
        assert lib.amuse_set_decode_dropout(None, p, 1, 7) == -1
        assert b"ctx is NULL" in lib.amuse_last_error()


def test_header_states_the_mask_contract():
    hdr = (REPO / "include/amuse_hip.h").read_text()
    i = hdr.index("int amuse_set_decode_dropout(")
    doc = hdr[hdr.rindex("/*", 0, i):i]
    for field in ("Philox4x32-10", "(clip, 0x80000000 | (8 l + s), e / 4, 2 + epoch)", "(h S + q) S + k", "e = h S + q", "q 512 + f", "(draw >> 8) >= thr",
                  "thr = (uint32)(p 2^24)", "1 / (1 - p)", "AMUSE_ESTATE", "AMUSE_PREC_F32X", "staged", "AMUSE_DECODE_STAGED", "clip_index0 + b", "S = 300"):
        assert field in doc, field
    assert doc.count("q 128 + f") == 3                                # sites 1, 3 and 5
    assert "AMUSE_TRAIN_INNER=eval|train|train-hip" in hdr and "train-hip-decode" in hdr
    for name in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "amuse_set_decode_dropout" in (REPO / name).read_text(), name
    assert "train-hip-decode" in (REPO / "INTEGRATION.md").read_text()


def test_train_hip_decode_inner_sampler_has_no_cpu_path():
    from amuse_amd.train_gesture import build_trainer
    with pytest.raises(RuntimeError, match="train-hip-decode"):
        build_trainer("cpu", inner="train-hip-decode")
    with pytest.raises(ValueError, match="bogus"):
        build_trainer("cpu", inner="bogus")


def test_masks_have_the_contracts_shape_and_rate():
    m = keep_mask(5, [3, 4], 2, 0, 0, 0.1)
    assert m.shape == (2, H, S, S) and abs(float(m.float().mean()) - 0.9) < 2e-3
    assert not torch.equal(m[0], m[1])
    assert torch.equal(keep_mask(5, [4], 2, 0, 0, 0.1)[0], m[1])                              # a clip's mask does not depend on its batch
    assert torch.equal(keep_mask(5, [4 + (1 << 32)], 2, 0, 0, 0.1)[0], m[1])                  # the clip index is truncated to 32 bits
    for other in (keep_mask(6, [3], 2, 0, 0, 0.1), keep_mask(5, [3], 3, 0, 0, 0.1), keep_mask(5, [3], 2, 0, 1, 0.1)):
        assert not torch.equal(other[0], m[0])
    assert keep_mask(5, [3], 0, 2, 0, 0.1).shape == (1, H, S) and keep_mask(5, [3], 0, 4, 0, 0.1).shape == (1, S, FF)
    assert bool(keep_mask(5, [3], 0, 1, 0, 0.0).all())


def test_all_keep_restatement_is_the_oracles_decode():
    """With every element kept and scale 1 the restatement is oracle.vae_decode up to the reassociation of fp32 sums (measured: 2.3e-6; the bar leaves room for another BLAS)."""
    from amuse_amd import weights as wts
    from oracle import amuse_oracle as orc
    Wp = orc.to_torch(wts.make_prior_weights(0))
    z = torch.from_numpy(np.load(GOLDEN / "vae_decode.npz")["z"])
    for lengths in (None, [300, 173, 1]):
        d = float((decode_restated(Wp, z, lengths, AllKeep()) - orc.vae_decode(Wp, z, lengths)).abs().max())
        print(f"all-keep restatement vs oracle.vae_decode, lengths {lengths}: {d:.3e}")
        assert d < 1e-5, d


def test_restatement_reproduces_the_reference_module():
    """fp32 on the CPU, full and ragged: the restatement with the contract's masks against the reference's own MotionPrior.decode in train() mode with the same
    masks injected (the fixture).  Measured: 1.9e-6 in both cases (bar 2e-5)."""
    from amuse_amd import weights as wts
    from oracle import amuse_oracle as orc
    Wp = orc.to_torch(wts.make_prior_weights(0))
    cases, m = fixture_cases()
    for name, lengths, expect in cases:
        out = decode_restated(Wp, m["z"], lengths, Masks(m["seed"], m["clips"], m["epoch"], m["p"]))
        d = fixture_distance(out.numpy(), expect)
        eval_d = fixture_distance(orc.vae_decode(Wp, m["z"], lengths).numpy(), expect)
        print(f"restatement vs reference module ({name}): {d:.3e}   (eval decode vs the same fixture: {eval_d:.3e})")
        assert d < REF_BAR, (name, d)
        assert eval_d > 0.1, (name, eval_d)                           # (the masks matter)
        if lengths is not None:
            for b, n in enumerate(lengths):
                assert bool((out[b, n:] == 0).all())
    # the wrong clip indices, seed or epoch do not reproduce it
    name, lengths, expect = cases[0]
    for kw in (dict(clips=[c + 1 for c in m["clips"]]), dict(seed=m["seed"] ^ 1), dict(epoch=m["epoch"] + 1)):
        a = dict(m, **kw)
        wrong = decode_restated(Wp, m["z"], lengths, Masks(a["seed"], a["clips"], a["epoch"], a["p"]))
        assert fixture_distance(wrong.numpy(), expect) > 0.1, kw
