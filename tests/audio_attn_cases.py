"""Helper (not a test): inputs that drive the audio attention kernels (csrc/k_audio.hip k_ast_attn<1|2>, csrc/k_audio_x.hip k_ast_attn_x) into the
lazy running-maximum rescale behind chunk 0, and the references the tests of that branch compare with.

The branch (amuse_dev.hpp kAttnTau = 6): keys arrive in 64-key chunks, scores leave the MFMA relative to the row's running maximum m_run (the C operand,
0 before chunk 0).  Chunk 0 takes its own maximum.  A later chunk shifts its scores, multiplies o[] and the row sum by alpha = exp2(-d) and advances m_run
only when SOME row of the wave's 16-query tile holds a score more than 6 log2 units above its running maximum (wave-uniform ballot); every row of a
triggering tile then moves by d = max(mx, 0).  With make_ast_weights(0, *) - N(0, 0.02) matrices - no chunk behind the first ever triggers.

Three things live here:
  * craft(name): the weight dictionaries of the three encoder slots - con: recipe A "diverse keys", emo: recipe B "ramp heads", sty: stock
    (the control) - crafted in blocks 1, 6 and 11 only, and fbanks(): the two clips every test encodes;
  * block_f64: one ViT block of oracle/audio_oracle.py ast_forward in float64 on a given block input (teacher forcing on the kernel's own tap);
  * chunk_attention: a model of the kernels' chunk rule - float64 to count triggers, with the bf16 kernel's rounding points (block_bf16_model) as the
    bf16 reference, and with fault= to show on the CPU that a broken rescale would be noticed.  Nothing in the library is touched.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

TAU = 6.0                        # amuse_dev.hpp kAttnTau
CHUNK, TILE = 64, 16             # keys per online-softmax step, queries per wave tile
TOKENS, DIM, HEADS, HD = 1214, 768, 12, 64
CRAFTED_BLOCKS = (1, 6, 11)
TAPS = ((0, 1), (5, 6), (10, 11))          # (tap that is the block's input, tap of the crafted block)
RECIPE = {"con": "A", "emo": "B", "sty": None}

# recipe A "diverse keys": v.pos_embed N(0, 1), q and k rows of a head scaled by LADDER[head] (scores by its square); no ramp head - on the N(0, 1)
# pos_embed a ramp head made the FEATURE of the whole network ill-conditioned (split-fp16 emulation 4.6e-6 .. 9.8e-6 of max|feature| over summation
# orders, the bar is 1e-5; without it 1.4e-6 .. 1.9e-6), so the x 10 heads supply the scores far under m_run here
LADDER = (1, 1, 3, 4, 6, 6, 8, 8, 10, 10, 10, 10)
A_CONTROL, A_MEANT, A_DEEP = (0, 1), (4, 5, 6, 7, 8, 9, 10, 11), (8, 9, 10, 11)
# recipe B "ramp heads": head 3 a pure ascending ramp (every row of a tile moves alike, chunk after chunk), head 7 the descending one (later scores
# hundreds of units under m_run: p underflows to 0), head 9 a gentle ascending ramp under keys made diverse (its stock q and k rows x 8) - rows of one
# tile then move by different amounts, the case in which a running maximum that fails to advance shows; every other head stock
B_CONTROL, B_MEANT, B_DESC = (0, 1, 2, 4, 5, 6, 8, 10, 11), (3, 9), 7
RAMP_COORD = 5                   # the coordinate of v.pos_embed that carries ramp(j) = RAMP_HEIGHT * j / TOKENS
RAMP_HEIGHT = 12.0
# (head, added to k feature 0's weight on RAMP_COORD, added to q feature 0's bias, factor on the head's stock q and k rows)
RAMPS = {"B": ((3, 3.0, 90.0, 1.0), (7, -3.0, 90.0, 1.0), (9, 1.0, 12.0, 8.0))}
# attn.proj.weight of the crafted blocks x this: the attention branch has to be a large enough part of the residual stream for a faulty rescale to miss
# the bf16 bars by 10 x (tests/test_audio_attn_cases_cpu.py, sensitivity)
PROJ_GAIN = {"A": 2.0, "B": 3.0}


def heads_of(name: str):
    """-> (control heads, heads meant to trigger, heads whose later scores lie far under m_run) of encoder slot `name`"""
    if RECIPE[name] == "A":
        return A_CONTROL, A_MEANT, A_DEEP
    if RECIPE[name] == "B":
        return B_CONTROL, B_MEANT, (B_DESC,)
    return tuple(range(HEADS)), (), ()


def _ramp_heads(W: Dict[str, np.ndarray], recipe: str) -> None:
    pos = W["v.pos_embed"].copy()
    pos[0, :, RAMP_COORD] += (RAMP_HEIGHT / TOKENS) * np.arange(TOKENS, dtype=np.float32)
    W["v.pos_embed"] = pos
    for l in CRAFTED_BLOCKS:
        w, b = W[f"v.blocks.{l}.attn.qkv.weight"].copy(), W[f"v.blocks.{l}.attn.qkv.bias"].copy()
        for head, kgain, qbias, noise in RAMPS[recipe]:
            for off in (0, DIM):
                w[off + HD * head:off + HD * (head + 1)] *= np.float32(noise)
                b[off + HD * head:off + HD * (head + 1)] *= np.float32(noise)
            w[DIM + HD * head, RAMP_COORD] += kgain
            b[HD * head] += qbias
        W[f"v.blocks.{l}.attn.qkv.weight"], W[f"v.blocks.{l}.attn.qkv.bias"] = w, b


def craft(name: str) -> "OrderedDict[str, np.ndarray]":
    """The weights of encoder slot `name` for AudioEngine(con, emo, sty): make_ast_weights(0, name) with arrays REPLACED in a copy of the dict."""
    from amuse_amd import audio_weights as aw
    W = aw.make_ast_weights(0, name)
    recipe = RECIPE[name]
    if recipe is None:
        return W
    if recipe == "A":
        g = np.random.default_rng(20240)
        W["v.pos_embed"] = g.standard_normal(W["v.pos_embed"].shape).astype(np.float32)
        scale = np.repeat(np.asarray(LADDER, dtype=np.float32), HD)
        scale = np.concatenate([scale, scale])                       # q rows, k rows
        for l in CRAFTED_BLOCKS:
            w, b = W[f"v.blocks.{l}.attn.qkv.weight"].copy(), W[f"v.blocks.{l}.attn.qkv.bias"].copy()
            w[:2 * DIM] *= scale[:, None]
            b[:2 * DIM] *= scale
            W[f"v.blocks.{l}.attn.qkv.weight"], W[f"v.blocks.{l}.attn.qkv.bias"] = w, b
    else:
        _ramp_heads(W, recipe)
    if PROJ_GAIN[recipe] != 1.0:
        for l in CRAFTED_BLOCKS:
            W[f"v.blocks.{l}.attn.proj.weight"] = W[f"v.blocks.{l}.attn.proj.weight"] * np.float32(PROJ_GAIN[recipe])
    for v in W.values():
        v.flags.writeable = False
    return W


def fbanks() -> torch.Tensor:
    """(2, 1024, 128) fp32: clip 0 N(0, 1), clip 1 the speech-like signal of tests/test_gpu_audio.py through the oracle's fbank."""
    from oracle import audio_oracle as ao
    g = torch.Generator().manual_seed(4711)
    noise = torch.randn(1024, 128, generator=g)
    n = 60000
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    wave = 0.1 * torch.sin(2 * np.pi * 220.0 * t) + 0.05 * torch.sin(2 * np.pi * 1900.0 * t) + 0.05 * torch.randn(n, generator=g)
    return torch.stack([noise, ao.prepare_fbank(wave)])


def embed(W: Dict[str, torch.Tensor], fbank: torch.Tensor) -> torch.Tensor:
    """The input of block 0 (ast_forward up to + pos_embed), in the dtype of W / fbank."""
    x = fbank[:, None].transpose(2, 3)
    cols = torch.nn.functional.unfold(x, kernel_size=16, stride=10)
    x = cols.transpose(1, 2) @ W["v.patch_embed.proj.weight"].reshape(DIM, 256).T + W["v.patch_embed.proj.bias"]
    B = x.shape[0]
    x = torch.cat([W["v.cls_token"].expand(B, -1, -1), W["v.dist_token"].expand(B, -1, -1), x], dim=1)
    return x + W["v.pos_embed"]


# ------------------------------------------------------------------------------------------------ the chunk rule
def chunk_attention(q, k, v, rp=None, fault: Optional[str] = None, stats: Optional[dict] = None):
    """q, k, v (..., S, 64); q already in log2 units (x log2(e) / 8).  The kernels' online softmax: 64-key chunks, m_run = 0 as the first C operand,
    chunk 0 takes its own maximum, later chunks move a 16-row tile's maxima - every row by d = max(mx, 0) - only when some row's chunk maximum is more
    than TAU above its running one.  rp rounds the un-normalised p (the PV operand; the row sum adds up the rounded p).  Returns o / l, NOT rounded.
    fault (CPU sensitivity test only): "o" - the accumulators are not multiplied by alpha; "l" - the row sum is not; "m" - the scores are shifted and
    the accumulators rescaled but m_run is not advanced.
    stats, if given, receives trig (..., tiles, chunks) bool, moves (..., S) = number of chunks >= 1 in which the row's maximum moved, dmax (..., S) =
    its largest single move, below / above (..., S) = the deepest / highest chunk maximum under / over m_run in a chunk >= 1 (log2 units)."""
    assert fault in (None, "o", "l", "m")
    rp = rp or (lambda t: t)
    lead, S = q.shape[:-2], q.shape[-2]
    Sp = -(-S // TILE) * TILE
    m = q.new_zeros(*lead, S)
    l = q.new_zeros(*lead, S)
    o = torch.zeros_like(q)
    trigs = []
    moves, dmax, below = q.new_zeros(*lead, S), q.new_zeros(*lead, S), q.new_zeros(*lead, S)
    above = q.new_full((*lead, S), -math.inf)
    for c, k0 in enumerate(range(0, S, CHUNK)):
        k1 = min(k0 + CHUNK, S)
        st = q @ k[..., k0:k1, :].transpose(-1, -2) - m[..., None]
        mx = st.max(dim=-1).values
        if c == 0:
            d = mx
        else:
            # pad query rows (the last tile's rows 1214, 1215) take no part in the decision
            trig = torch.nn.functional.pad(mx, (0, Sp - S), value=-math.inf).reshape(*lead, Sp // TILE, TILE).gt(TAU).any(-1)
            trigs.append(trig)
            trow = trig[..., None].expand(*lead, Sp // TILE, TILE).reshape(*lead, Sp)[..., :S]
            d = torch.where(trow, mx.clamp(min=0.0), torch.zeros_like(mx))
            moves += (d > 0).to(q.dtype)
            dmax = torch.maximum(dmax, d)
            below = torch.maximum(below, -mx)
            above = torch.maximum(above, mx)
        st = st - d[..., None]
        if c > 0:
            alpha = torch.exp2(-d)
            if fault != "l":
                l = l * alpha
            if fault != "o":
                o = o * alpha[..., None]
        if not (fault == "m" and c > 0):
            m = m + d
        p = rp(torch.exp2(st))
        l = l + p.sum(-1)
        o = o + p @ v[..., k0:k1, :]
    if stats is not None:
        stats.update(trig=torch.stack(trigs, -1), moves=moves, dmax=dmax, below=below, above=above)
    return o / l[..., None]


# ------------------------------------------------------------------------------------------------ one block
def _ln(t, W, p):
    return torch.nn.functional.layer_norm(t, (DIM,), W[p + ".weight"], W[p + ".bias"], 1e-6)


def _heads(t):
    return t.reshape(t.shape[0], -1, HEADS, HD).transpose(1, 2)      # (B, H, S, 64)


def qkv_f64(W, l: int, x):
    """q (log2 units), k, v (B, H, S, 64) of block l on block input x, float64."""
    p = f"v.blocks.{l}"
    qkv = _ln(x, W, p + ".norm1") @ W[p + ".attn.qkv.weight"].T + W[p + ".attn.qkv.bias"]
    return _heads(qkv[..., :DIM]) * (math.log2(math.e) / 8.0), _heads(qkv[..., DIM:2 * DIM]), _heads(qkv[..., 2 * DIM:])


def _rest(W, l: int, x, o, r=lambda t: t):
    """x + proj(o), then the MLP half; r rounds the GEMM operands."""
    p = f"v.blocks.{l}"
    x = x + r(o) @ r(W[p + ".attn.proj.weight"]).T + W[p + ".attn.proj.bias"]
    h = torch.nn.functional.gelu(r(_ln(x, W, p + ".norm2")) @ r(W[p + ".mlp.fc1.weight"]).T + W[p + ".mlp.fc1.bias"])
    return x + r(h) @ r(W[p + ".mlp.fc2.weight"]).T + W[p + ".mlp.fc2.bias"]


def block_f64(W64, l: int, x, fault: Optional[str] = None, chunked: bool = False):
    """Block l of ast_forward (LayerNorm eps 1e-6, normalised softmax, exact GELU) on block input x (B, 1214, 768), float64.  W64: float64 tensors.
    chunked / fault: the attention through chunk_attention instead (float64: the same function up to summation order unless a fault is set)."""
    x = x.double()
    q, k, v = qkv_f64(W64, l, x)
    if chunked or fault:
        o = chunk_attention(q, k, v, fault=fault)
    else:
        o = torch.exp2(q @ k.transpose(-1, -2) - (q @ k.transpose(-1, -2)).max(-1, keepdim=True).values)
        o = (o / o.sum(-1, keepdim=True)) @ v
    return _rest(W64, l, x, o.transpose(1, 2).reshape(x.shape[0], -1, DIM))


def _r(t):
    return t.to(torch.bfloat16).to(t.dtype)


KQ = float(np.float32(0.125) * np.float32(1.44269504088896340736))    # the qkv epilogue's factor on q (k_audio_gemm.hip)


def block_bf16_model(W, l: int, x, dtype=torch.float32):
    """Block l with the bf16 kernels' rounding points, on block input x: LayerNorm output, weights, q x log2(e) / 8, k, v, the un-normalised p of every
    chunk (summed as rounded), o, the MLP's hidden - all rounded to bf16; accumulation, softmax statistics, LayerNorm, GELU and the residual stream in
    `dtype` (float32 as the kernels; float64 to measure what the accumulation order alone can move)."""
    W = {k_: v_.to(dtype) for k_, v_ in W.items() if k_.startswith(f"v.blocks.{l}.")}
    x = x.to(dtype)
    p = f"v.blocks.{l}"
    qkv = _r(_ln(x, W, p + ".norm1")) @ _r(W[p + ".attn.qkv.weight"]).T + W[p + ".attn.qkv.bias"]
    q, k, v = _heads(_r(qkv[..., :DIM] * KQ)), _heads(_r(qkv[..., DIM:2 * DIM])), _heads(_r(qkv[..., 2 * DIM:]))
    o = _r(chunk_attention(q, k, v, rp=_r))
    return _rest(W, l, x, o.transpose(1, 2).reshape(x.shape[0], -1, DIM), _r)


# ------------------------------------------------------------------------------------------------ metrics
def rel_l2(got, ref) -> float:
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm())


def worst_token_rel_l2(got, ref) -> float:
    """the worst single token's relative L2 over its 768-vector: a few wrong rows cannot hide among 1,214"""
    got, ref = got.double(), ref.double()
    return float(((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max())


def bf16_metrics(got, ref):
    """(max |error|, mean |error|) over max |ref|: the two figures tests/test_gpu_audio.py holds to 2e-2 and 5e-4"""
    got, ref = got.double(), ref.double()
    s = float(ref.abs().max())
    return float((got - ref).abs().max()) / s, float((got - ref).abs().mean()) / s


def trigger_share(trig, heads) -> float:
    """share of (head, tile, chunk >= 1) triples that trigger; trig (B, H, tiles, chunks)"""
    return float(trig[:, list(heads)].double().mean()) if len(heads) else 0.0


# ------------------------------------------------------------------------------------------------ bars
# Split-fp16 emulation of the whole network against the float64 oracle on the crafted weights and the two clips (relative L2 of the residual stream,
# worst single token's relative L2), per (slot, crafted block): measured by tests/test_audio_attn_cases_cpu.py, which holds this record to what it
# measures.  Not a kernel's output.
EMULATED = {
    ("con", 1): (2.10e-6, 8.06e-6), ("con", 6): (5.13e-6, 3.73e-5), ("con", 11): (9.98e-6, 1.15e-4),
    ("emo", 1): (2.19e-6, 1.26e-5), ("emo", 6): (3.22e-6, 1.06e-5), ("emo", 11): (3.56e-6, 8.92e-6),
    ("sty", 1): (1.87e-6, 3.72e-6), ("sty", 6): (2.33e-6, 3.62e-6), ("sty", 11): (2.55e-6, 3.71e-6),
}
BF16_BARS = (2e-2, 5e-4)         # tests/test_gpu_audio.py: every element / the mean error, over max|x| - unwidened (the CPU test shows they can stand)
FEATURE_BAR = 1e-5               # tests/test_gpu_audio_parity.py: max |feature error| over max |feature|


def fp32x_bars(name: str, block: int):
    """(relative L2, worst token's relative L2) the parity mode has to hold after crafted block `block`: max(1e-5, 4 x emulated) - 1e-5 is the
    contract's bar, 4 x the margin the project gave the stock case (2.5e-6 emulated, bar 1e-5)"""
    return tuple(max(1e-5, 4.0 * e) for e in EMULATED[name, block])


def write_golden(path) -> None:
    """tests/golden/audio_attn_cases.npz: the float64 oracle's features (2, 256) of the three slots on fbanks() - `python tests/audio_attn_cases.py`"""
    from oracle import audio_oracle as ao
    out = {}
    with torch.no_grad():
        for name in RECIPE:
            W64 = {k_: v_.double() for k_, v_ in ao.to_torch(craft(name)).items()}
            out[name] = ao.ast_forward(W64, fbanks().double(), True).numpy()
    np.savez(path, **out)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    write_golden(Path(__file__).resolve().parent / "golden" / "audio_attn_cases.npz")
