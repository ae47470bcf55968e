"""Parameter inventory + deterministic weights for the audio front-end (models/audio: 3 x AST -> con / emo / sty).

The reference builds each encoder as ``ASTModel(label_dim, fstride=10, tstride=10, input_fdim=128, input_tdim=1024,
model_size='base384')`` (AST_EVP.py:53-61) around timm 0.4.5's ``vit_deit_base_distilled_patch16_384``
(audio_main_new.py:66-70): 12 pre-norm blocks of width 768 / 12 heads / MLP 3072 over 2 + 12 x 101 tokens.
timm is not installed, so the key list below is restated from timm 0.4.5's ``DistilledVisionTransformer`` attribute
names (parity unpinned - see oracle/audio_oracle.py); only the tensors the forward pass reads are listed.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np

from .weights import _rng_for

AST_DIM = 768
AST_HEADS = 12
AST_LAYERS = 12
AST_MLP = 3072
AST_FDIM, AST_TDIM = 128, 1024            # mel bins, frames (configs/base_new.json wav_dtw_mfcc)
AST_PATCH, AST_STRIDE = 16, 10
AST_F = (AST_FDIM - AST_PATCH) // AST_STRIDE + 1   # 12
AST_T = (AST_TDIM - AST_PATCH) // AST_STRIDE + 1   # 101
AST_TOKENS = 2 + AST_F * AST_T                     # 1214
AST_FEAT = 256
ENCODERS = ("con", "emo", "sty")


def ast_param_spec() -> "OrderedDict[str, Tuple[int, ...]]":
    """Forward-pass tensors of one ASTModel, timm 0.4.5 names under ``v.`` plus ``feature_head`` (audio_main_new.py:77)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["v.cls_token"] = (1, 1, AST_DIM)
    s["v.dist_token"] = (1, 1, AST_DIM)
    s["v.pos_embed"] = (1, AST_TOKENS, AST_DIM)
    s["v.patch_embed.proj.weight"] = (AST_DIM, 1, AST_PATCH, AST_PATCH)
    s["v.patch_embed.proj.bias"] = (AST_DIM,)
    for i in range(AST_LAYERS):
        p = f"v.blocks.{i}"
        s[f"{p}.norm1.weight"] = (AST_DIM,)
        s[f"{p}.norm1.bias"] = (AST_DIM,)
        s[f"{p}.attn.qkv.weight"] = (3 * AST_DIM, AST_DIM)
        s[f"{p}.attn.qkv.bias"] = (3 * AST_DIM,)
        s[f"{p}.attn.proj.weight"] = (AST_DIM, AST_DIM)
        s[f"{p}.attn.proj.bias"] = (AST_DIM,)
        s[f"{p}.norm2.weight"] = (AST_DIM,)
        s[f"{p}.norm2.bias"] = (AST_DIM,)
        s[f"{p}.mlp.fc1.weight"] = (AST_MLP, AST_DIM)
        s[f"{p}.mlp.fc1.bias"] = (AST_MLP,)
        s[f"{p}.mlp.fc2.weight"] = (AST_DIM, AST_MLP)
        s[f"{p}.mlp.fc2.bias"] = (AST_DIM,)
    s["v.norm.weight"] = (AST_DIM,)
    s["v.norm.bias"] = (AST_DIM,)
    s["feature_head.0.weight"] = (AST_DIM,)
    s["feature_head.0.bias"] = (AST_DIM,)
    s["feature_head.1.weight"] = (AST_FEAT, AST_DIM)
    s["feature_head.1.bias"] = (AST_FEAT,)
    return s


def ast_param_count() -> int:
    return int(sum(int(np.prod(v)) for v in ast_param_spec().values()))


_MADE: Dict[tuple, Dict[str, np.ndarray]] = {}


def make_ast_weights(seed: int, encoder: str) -> Dict[str, np.ndarray]:
    """Deterministic float32 weights for encoder ``con`` | ``emo`` | ``sty``: N(0, 0.02) matrices (timm's trunc_normal
    scale), LayerNorm parameters perturbed away from (1, 0), small non-zero biases.  The arrays of a (seed, encoder) pair are generated once per process
    (345 MB, 3.3 s) and handed out read-only in a fresh dict."""
    assert encoder in ENCODERS
    if (seed, encoder) in _MADE:
        return OrderedDict(_MADE[(seed, encoder)])
    out: Dict[str, np.ndarray] = OrderedDict()
    for name, shape in ast_param_spec().items():
        g = _rng_for(seed, f"ast.{encoder}.{name}")
        parts = name.split(".")
        leaf = parts[-1]
        is_norm = parts[-2].startswith("norm") or name.startswith("feature_head.0")
        if is_norm:
            a = (1.0 if leaf == "weight" else 0.0) + g.uniform(-0.1, 0.1, shape)
        elif leaf == "bias":
            a = g.uniform(-0.05, 0.05, shape)
        else:
            a = 0.02 * g.standard_normal(shape, dtype=np.float32)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
        out[name].flags.writeable = False
    if len(_MADE) < 6:
        _MADE[(seed, encoder)] = out
    return OrderedDict(out)


# ---- the tail of AST_EVP behind the three encoders (models/audio/AST_EVP.py:12-42,63-82; audio_main_new.py:76-81): classifier heads, FusionBlock, DecoderBlock
TAIL_LABELS = {"emo": 8, "sty": 30}                      # label_dim of emo_enc / sty_enc (con_enc has none)
TAIL_FUSION_DIM, TAIL_FUSION_LAYERS = 3 * AST_FEAT, 2     # cat(emo, sty, con)
TAIL_LATENT_DIM, TAIL_DECODE_LAYERS = 512, 4
TAIL_FF = 2048                                            # nn.TransformerEncoderLayer's default dim_feedforward
TAIL_HIDDEN = 2 * TAIL_LATENT_DIM                         # decode.projection.0
TAIL_OUT = AST_TDIM * AST_FDIM                            # decode.projection.2: the 1024 x 128 fbank


def _encoder_layer_spec(s, p: str, d: int) -> None:
    """nn.TransformerEncoderLayer(d, nhead=4) in torch's state-dict order."""
    s[f"{p}.self_attn.in_proj_weight"] = (3 * d, d)
    s[f"{p}.self_attn.in_proj_bias"] = (3 * d,)
    s[f"{p}.self_attn.out_proj.weight"] = (d, d)
    s[f"{p}.self_attn.out_proj.bias"] = (d,)
    s[f"{p}.linear1.weight"] = (TAIL_FF, d)
    s[f"{p}.linear1.bias"] = (TAIL_FF,)
    s[f"{p}.linear2.weight"] = (d, TAIL_FF)
    s[f"{p}.linear2.bias"] = (d,)
    for n in ("norm1", "norm2"):
        s[f"{p}.{n}.weight"] = (d,)
        s[f"{p}.{n}.bias"] = (d,)


def ast_tail_param_spec() -> "OrderedDict[str, Tuple[int, ...]]":
    """AST_EVP's state-dict entries behind the encoders' feature heads, in the order of the flat array amuse_audio_set_tail takes
    (include/amuse_hip.h AMUSE_AST_TAIL_PARAMS): the classifier heads of emo_enc / sty_enc, fusion, decode."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    for enc in ("emo", "sty"):
        L = TAIL_LABELS[enc]
        for head, d in (("mlp_head", AST_FEAT), ("mlp_head_featbased", AST_DIM)):
            s[f"{enc}_enc.{head}.0.weight"] = (d,)
            s[f"{enc}_enc.{head}.0.bias"] = (d,)
            s[f"{enc}_enc.{head}.1.weight"] = (L, d)
            s[f"{enc}_enc.{head}.1.bias"] = (L,)
    for i in range(TAIL_FUSION_LAYERS):
        _encoder_layer_spec(s, f"fusion.layers.{i}", TAIL_FUSION_DIM)
    s["fusion.norm.weight"] = (TAIL_FUSION_DIM,)
    s["fusion.norm.bias"] = (TAIL_FUSION_DIM,)
    s["fusion.fc.weight"] = (TAIL_LATENT_DIM, TAIL_FUSION_DIM)
    s["fusion.fc.bias"] = (TAIL_LATENT_DIM,)
    for i in range(TAIL_DECODE_LAYERS):
        _encoder_layer_spec(s, f"decode.layers.{i}", TAIL_LATENT_DIM)
    s["decode.norm.weight"] = (TAIL_LATENT_DIM,)
    s["decode.norm.bias"] = (TAIL_LATENT_DIM,)
    s["decode.projection.0.weight"] = (TAIL_HIDDEN, TAIL_LATENT_DIM)
    s["decode.projection.0.bias"] = (TAIL_HIDDEN,)
    s["decode.projection.2.weight"] = (TAIL_OUT, TAIL_HIDDEN)
    s["decode.projection.2.bias"] = (TAIL_OUT,)
    return s


def ast_tail_param_count() -> int:
    return int(sum(int(np.prod(v)) for v in ast_tail_param_spec().values()))


def make_ast_tail_weights(seed: int) -> Dict[str, np.ndarray]:
    """Deterministic float32 weights for ast_tail_param_spec, in the style of make_ast_weights: N(0, 1 / fan_in) matrices, LayerNorm parameters perturbed
    away from (1, 0), small non-zero biases.  The 131072 x 1024 matrix of decode.projection.2 is one seeded 1024 x 1024 block tiled 128 times with a per-row
    scale of magnitude 0.5 .. 1.5 and random sign, all 131072 scales distinct (no two rows are equal), so that drawing it costs one pass over its 537 MB."""
    out: Dict[str, np.ndarray] = OrderedDict()
    for name, shape in ast_tail_param_spec().items():
        g = _rng_for(seed, f"ast.tail.{name}")
        parts = name.split(".")
        leaf = parts[-1]
        is_norm = parts[-2].startswith("norm") or (parts[1].startswith("mlp_head") and parts[2] == "0")
        if is_norm:
            a = (1.0 if leaf == "weight" else 0.0) + g.uniform(-0.1, 0.1, shape)
        elif leaf in ("bias", "in_proj_bias"):
            a = g.uniform(-0.05, 0.05, shape)
        elif name == "decode.projection.2.weight":
            block = (g.standard_normal((TAIL_HIDDEN, TAIL_HIDDEN), dtype=np.float32) / np.float32(np.sqrt(TAIL_HIDDEN)))
            mag = np.float32(0.5) + (g.permutation(TAIL_OUT).astype(np.float32) + np.float32(0.5)) / np.float32(TAIL_OUT)
            scale = (mag * g.choice(np.array([-1.0, 1.0], dtype=np.float32), TAIL_OUT)).astype(np.float32)
            a = (block[None, :, :] * scale.reshape(TAIL_OUT // TAIL_HIDDEN, TAIL_HIDDEN, 1)).reshape(shape)
        else:
            a = g.standard_normal(shape, dtype=np.float32) / np.float32(np.sqrt(shape[-1]))
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
        out[name].flags.writeable = False
    return out
