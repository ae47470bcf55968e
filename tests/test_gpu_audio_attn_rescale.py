"""GPU: the lazy running-maximum rescale of the audio attention kernels (csrc/k_audio.hip k_ast_attn<1|2>, csrc/k_audio_x.hip k_ast_attn_x; amuse_dev.hpp
kAttnTau) on inputs that reach it.  On make_ast_weights(0, *) no chunk behind the first ever moves a running maximum, so every other audio test passes
with that branch deleted; tests/audio_attn_cases.py crafts blocks 1, 6 and 11 of two encoder slots so that half of the (head, query tile, chunk) triples
of the heads meant to rescale (con: recipe A, emo: recipe B; sty stays stock, the control on which the same tests must pass), and
tests/test_audio_attn_cases_cpu.py shows on the CPU that they do, where the bars come from and that a rescale that forgets o[], the row sum or m_run
would miss them by 10 x and more.

One engine, two clips per call, everything through AudioEngine.encode:
  * fp32x: the taps (0 -> 1), (5 -> 6), (10 -> 11), teacher-forced on the kernel's own tap, against the float64 block (audio_attn_cases.block_f64):
    relative L2 and the worst token's relative L2 within max(1e-5, 4 x the split-fp16 emulation) (audio_attn_cases.fp32x_bars), the feature within
    1e-5 x max of the float64 oracle's (tests/golden/audio_attn_cases.npz, written by that oracle);
  * bf16: the same taps against the model of the bf16 kernel's rounding points (audio_attn_cases.block_bf16_model), under the bars of
    tests/test_gpu_audio.py: every element within 2e-2 x max|x|, the mean error within 5e-4 x max|x|;
  * bitwise, both modes: a call repeated, a clip alone (bf16: the NQ = 1 instantiation) against its row of the two-clip call, the clips swapped, and
    bf16 after a round trip through fp32x.
"""
import numpy as np
import pytest
import torch

import audio_attn_cases as ac
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SLOTS = ("con", "emo", "sty")


@pytest.fixture(scope="module")
def env():
    from amuse_amd.audio import AudioEngine
    from oracle import audio_oracle as ao
    Wnp = {n: ac.craft(n) for n in SLOTS}
    eng = AudioEngine(Wnp["con"], Wnp["emo"], Wnp["sty"], "cuda:0")
    gold = np.load(GOLDEN / "audio_attn_cases.npz")
    yield {"eng": eng, "W": {n: ao.to_torch(Wnp[n]) for n in SLOTS}, "fb": ac.fbanks(), "feat64": {n: torch.from_numpy(gold[n]) for n in SLOTS}}
    eng.close()


@pytest.fixture
def mode(env, request):
    """the module's engine in the requested mode for one test, back in bf16 afterwards"""
    env["eng"].set_precision(request.param)
    yield request.param
    env["eng"].set_precision("bf16")


def _block_weights(W, l, dtype):
    return {k: v.to(dtype) for k, v in W.items() if k.startswith(f"v.blocks.{l}.")}


@pytest.mark.parametrize("which", SLOTS)
def test_fp32x_blocks_with_rescale_against_float64(env, which):
    eng, W, fb = env["eng"], env["W"][which], env["fb"]
    eng.set_precision("fp32x")
    try:
        got = {}
        for lin, lout in ac.TAPS:
            _, h_in = eng.encode(which, fb, tap_block=lin)
            _, h_out = eng.encode(which, fb, tap_block=lout)
            got[lout] = (h_in.cpu(), h_out.cpu())
    finally:
        eng.set_precision("bf16")
    res = {}
    with torch.no_grad():
        for l, (h_in, h_out) in got.items():
            ref = ac.block_f64(_block_weights(W, l, torch.float64), l, h_in)
            res[l] = (ac.rel_l2(h_out, ref), ac.worst_token_rel_l2(h_out, ref))
            bars = ac.fp32x_bars(which, l)
            print(f"[attn rescale] fp32x {which} block {l}: rel-L2 {res[l][0]:.2e} (bar {bars[0]:.2e}), worst token {res[l][1]:.2e} (bar {bars[1]:.2e})")
    for l, r in res.items():
        bars = ac.fp32x_bars(which, l)
        assert r[0] <= bars[0] and r[1] <= bars[1], (which, l, r, bars)


@pytest.mark.parametrize("which", SLOTS)
def test_fp32x_feature_against_float64(env, which):
    """The whole crafted network in fp32x: the feature within 1e-5 x max|feature| of the float64 oracle's (the bar of tests/test_gpu_audio_parity.py).
    The split-fp16 emulation of the three slots sits at 2.3e-6 / 3.5e-6 / 3.2e-6 (tests/test_audio_attn_cases_cpu.py holds it under 0.4 of the bar)."""
    eng, fb = env["eng"], env["fb"]
    eng.set_precision("fp32x")
    try:
        feat = eng.encode(which, fb).cpu()
    finally:
        eng.set_precision("bf16")
    ref = env["feat64"][which]
    ferr = (feat.double() - ref).abs().max(dim=1).values / ref.abs().max()
    print(f"[attn rescale] fp32x {which}: feature max / max per clip {float(ferr[0]):.2e} {float(ferr[1]):.2e} (bar {ac.FEATURE_BAR:.0e})")
    assert float(ferr.max()) <= ac.FEATURE_BAR, (which, ferr.tolist())


@pytest.mark.parametrize("which", SLOTS)
def test_bf16_blocks_with_rescale_against_the_rounding_point_model(env, which):
    eng, W, fb = env["eng"], env["W"][which], env["fb"]
    assert eng.precision == "bf16"
    res = {}
    with torch.no_grad():
        for lin, lout in ac.TAPS:
            _, h_in = eng.encode(which, fb, tap_block=lin)
            _, h_out = eng.encode(which, fb, tap_block=lout)
            ref = ac.block_bf16_model(W, lout, h_in.cpu())
            assert bool(torch.isfinite(h_out).all())
            res[lout] = ac.bf16_metrics(h_out.cpu(), ref)
            print(f"[attn rescale] bf16 {which} block {lout}: max error {res[lout][0]:.2e} (bar {ac.BF16_BARS[0]:.0e}), mean error {res[lout][1]:.2e} "
                  f"(bar {ac.BF16_BARS[1]:.0e}) of max|x| = {float(ref.abs().max()):.1f}")
    for l, r in res.items():
        assert r[0] < ac.BF16_BARS[0] and r[1] < ac.BF16_BARS[1], (which, l, r)


@pytest.mark.parametrize("mode", ["bf16", "fp32x"], indirect=True)
def test_bitwise_properties_in_the_peaked_regime(env, mode):
    eng, fb = env["eng"], env["fb"]
    assert eng.precision == mode
    both = {n: eng.encode(n, fb, tap_block=11) for n in SLOTS}
    for n in SLOTS:
        feat, hid = both[n]
        assert bool(torch.isfinite(hid).all()) and bool(torch.isfinite(feat).all()), n
        # a clip alone (bf16: one query tile per wave, NQ = 1) is its row of the two-clip call
        for k in (0, 1):
            f1, h1 = eng.encode(n, fb[k:k + 1], tap_block=11)
            assert torch.equal(h1[0], hid[k]) and torch.equal(f1[0], feat[k]), (n, k)
        # the clips swapped: the rows swapped
        fs, hs = eng.encode(n, fb.flip(0), tap_block=11)
        assert torch.equal(hs.flip(0), hid) and torch.equal(fs.flip(0), feat), n
        # the same call again, behind all of the above
        f2, h2 = eng.encode(n, fb, tap_block=11)
        assert torch.equal(h2, hid) and torch.equal(f2, feat), n
    if mode == "bf16":
        # ... and behind a round trip through the parity mode
        eng.set_precision("fp32x")
        x = {n: eng.encode(n, fb, tap_block=11) for n in SLOTS}
        eng.set_precision("bf16")
        for n in SLOTS:
            f3, h3 = eng.encode(n, fb, tap_block=11)
            assert torch.equal(h3, both[n][1]) and torch.equal(f3, both[n][0]), n
            assert not torch.equal(x[n][1], h3), n                     # the modes differ
