"""CPU: where the bar of the audio front-end's parity mode (amuse_audio_set_precision AMUSE_PREC_F32X, tests/test_gpu_audio_parity.py) comes from.
oracle/audio_oracle.py rounds every GEMM operand through `_rb`; here `_rb` is replaced (pytest's monkeypatch - the oracle file is untouched) by each
operand scheme in turn - split fp16 (hi = rn16(x), lo = rn16(x - hi), the operand is hi + lo), plain fp16, bf16 (what the throughput kernels do) - and
one encoder on one clip is compared with the same oracle in float64: the residual stream after block 11 (relative L2) and the feature (max error over
max value).  Split fp16 lands at ~2.5e-6, two to three orders below the one-piece formats: the GPU bar is 1e-5, the margin the sampler's fp32x mode got
(emulated 3.0e-6, bar 1e-5).

This is an emulation of arithmetic, not a test of the library: it passes before the feature exists, and says what the feature has to reach."""
import numpy as np
import torch


def _wave(n, seed):   # the speech-like signal of tests/test_gpu_audio.py (_waves(n, 1, seed)[0])
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    base = 0.2 * torch.sin(2 * np.pi * 220.0 * t) + 0.1 * torch.sin(2 * np.pi * 1900.0 * t)
    return base * 0.5 + 0.05 * torch.randn(n, generator=g)


def _split16(x):
    hi = x.to(torch.float16).to(torch.float32)
    return hi + (x - hi).to(torch.float16).to(torch.float32)


SCHEMES = {
    "fp32": lambda x: x,
    "split_fp16": _split16,
    "fp16": lambda x: x.to(torch.float16).to(torch.float32),
    "bf16": lambda x: x.to(torch.bfloat16).to(torch.float32),
}


def test_split_fp16_operands_reach_fp32_class_and_one_piece_formats_do_not(monkeypatch):
    from amuse_amd import audio_weights as aw
    from oracle import audio_oracle as ao
    W = ao.to_torch(aw.make_ast_weights(0, "emo"))
    fb = ao.prepare_fbank(_wave(60000, 5))[None]
    with torch.no_grad():
        taps64 = {}
        ref = ao.ast_forward({k: v.double() for k, v in W.items()}, fb.double(), True, emulate_bf16=False, taps=taps64)
        h64 = taps64["block11"]
        err = {}
        for name, fn in SCHEMES.items():
            monkeypatch.setattr(ao, "_rb", lambda x, on, fn=fn: fn(x) if on else x)
            taps = {}
            feat = ao.ast_forward(W, fb, True, emulate_bf16=True, taps=taps)
            err[name] = (float((taps["block11"].double() - h64).norm() / h64.norm()), float((feat.double() - ref).abs().max() / ref.abs().max()))
            print(f"{name:11s} residual stream after block 11 rel-L2 {err[name][0]:.2e}   feature max / max {err[name][1]:.2e}")
    assert max(err["split_fp16"]) <= 1e-5, err
    assert min(err["fp16"]) > 1e-4, err
    assert min(err["bf16"]) > 1e-3, err
