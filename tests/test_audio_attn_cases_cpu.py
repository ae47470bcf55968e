"""CPU: what makes tests/test_gpu_audio_attn_rescale.py mean something.  The audio attention kernels rescale their accumulators only when a chunk behind
the first moves a running maximum by more than kAttnTau = 6 log2 units, and on make_ast_weights(0, *) that never happens.  Here, in float64 and without
the library:
  (1) the stock slot triggers 0 times in blocks 0, 1, 6 and 11 - the gap the old suite leaves;
  (2) the crafted slots of tests/audio_attn_cases.py (con: recipe A, emo: recipe B) reach the branch in every crafted block (1, 6, 11): >= 20 % of the
      (head, 16-query tile, chunk >= 1) triples of the heads meant to trigger do, the control heads of the same launch never do, some row's maximum moves
      >= 4 times, some single move exceeds 24 log2 units (the old mass falls below fp32 resolution), some head's later scores lie > 100 units under m_run;
  (3) the bars of the GPU test are MEASURED here, not taken from a kernel: the oracle with `_rb` monkeypatched to split-fp16 operands, fp32, against
      the float64 oracle on the crafted weights - relative L2 of the residual stream after each crafted block and the worst single token's relative L2;
      the GPU bar is max(1e-5, 4 x emulated) (1e-5: the contract's bar; 4 x: the margin of the stock case, 2.5e-6 emulated under a bar of 1e-5).
      The figures are recorded in audio_attn_cases.EMULATED (the GPU test reads them there); this test re-measures them and holds the record to them;
  (4) the bf16 rounding-point model run in fp32 stays far inside the bars of tests/test_gpu_audio.py (2e-2 / 5e-4 of max|x|) of the same model
      accumulating in float64, so those bars stand unwidened;
  (5) each of three faults of the rescale - o[] not multiplied by alpha, the row sum not multiplied, m_run not advanced - pushed through the rest of the
      float64 block misses BOTH fp32x bars by >= 10 x and one of the two bf16 bars by >= 10 x, in every crafted block of both recipes.  For that the
      crafting scales attn.proj.weight of the crafted blocks (x 2 in A, x 3 in B): at x 1 the attention branch was too small a part of the stream.

Measured (2 clips; share over the heads meant to trigger; emulated = split-fp16 whole network against float64; sensitivity on clip 0 = by how many
times the LEAST visible of the three faults misses each bar - every figure below has to be >= 10):
  slot block  share  most moves  largest  deepest under   emulated                GPU bars                fault misses the bar by
                     of a row    move     m_run           rel-L2    worst token   rel-L2    worst token   rel-L2   worst token  bf16 (mean)
  con    1    0.61       9       130.2      152.5         2.10e-06  8.06e-06      1.00e-05  3.22e-05      2.7e+04  1.1e+04      80
  con    6    0.61       8       114.7      152.4         5.13e-06  3.73e-05      2.05e-05  1.49e-04      1.0e+04  1.9e+03      66
  con   11    0.59       8       105.5      147.6         9.98e-06  1.15e-04      3.99e-05  4.60e-04      4.4e+03  5.3e+02      57
  emo    1    0.66      18        85.2      792.6         2.19e-06  1.26e-05      1.00e-05  5.04e-05      2.5e+04  9.0e+03      28
  emo    6    0.51      18        54.7      480.2         3.22e-06  1.06e-05      1.29e-05  4.24e-05      6.5e+03  3.7e+03      13
  emo   11    0.48      18        41.6      351.6         3.56e-06  8.92e-06      1.42e-05  3.57e-05      3.5e+03  2.5e+03      11
  sty  1/6/11 0          0         0        (highest score over m_run 1.6)  1.9-2.6e-06  3.6-3.7e-06  1.0e-05  1.5e-05   (the control: nothing to break)
Emulated feature error (max / max): con 2.3e-06, emo 3.5e-06, sty 3.2e-06 (asserted <= 0.4 x the 1e-5 bar: the stock class).  bf16 model, fp32 against float64
accumulation: max <= 3.0e-03, mean <= 6.0e-05
of max|x| on every slot and block (bars 2e-2, 5e-4).
"""
import numpy as np
import pytest
import torch

import audio_attn_cases as ac
from conftest import GOLDEN


def _split16(x):   # tests/test_audio_split_emulation_cpu.py
    hi = x.to(torch.float16).to(torch.float32)
    return hi + (x - hi).to(torch.float16).to(torch.float32)


_CACHE = {}


def _slot(name):
    """float64 oracle of encoder slot `name` on the two clips: weights, taps of every block, the feature"""
    if name not in _CACHE:
        from oracle import audio_oracle as ao
        _CACHE.clear()                                   # one slot's 64-bit weights at a time
        W = ao.to_torch(ac.craft(name))
        W64 = {k: v.double() for k, v in W.items()}
        fb = ac.fbanks()
        taps = {}
        with torch.no_grad():
            feat = ao.ast_forward(W64, fb.double(), True, taps=taps)
            taps["block-1"] = ac.embed(W64, fb.double())
        _CACHE[name] = {"W": W, "W64": W64, "fb": fb, "taps": taps, "feat": feat}
    return _CACHE[name]


def _stats(s, l):
    q, k, v = ac.qkv_f64(s["W64"], l, s["taps"][f"block{l - 1}"])
    st = {}
    ac.chunk_attention(q, k, v, stats=st)
    return st


def test_stock_weights_never_reach_the_rescale():
    s = _slot("sty")
    with torch.no_grad():
        for l in (0, 1, 6, 11):
            st = _stats(s, l)
            n = int(st["trig"].sum())
            print(f"[attn cases] stock (sty) block {l}: {n} of {st['trig'].numel()} (clip, head, tile, chunk >= 1) trigger; highest score over m_run "
                  f"{float(st['above'].max()):.2f} (the rule asks for > {ac.TAU:.0f})")
            assert n == 0 and float(st["moves"].max()) == 0.0, l


@pytest.mark.parametrize("name", ["con", "emo"])
def test_crafted_inputs_reach_the_rescale(name):
    s = _slot(name)
    ctrl, meant, desc = ac.heads_of(name)
    with torch.no_grad():
        for l in ac.CRAFTED_BLOCKS:
            st = _stats(s, l)
            share = ac.trigger_share(st["trig"], meant)
            per_head = [round(ac.trigger_share(st["trig"], [h]), 3) for h in range(ac.HEADS)]
            moves, dmax = int(st["moves"].max()), float(st["dmax"].max())
            deep = float(st["below"][:, list(desc)].max())
            print(f"[attn cases] {name} block {l}: trigger share {share:.3f} over heads {meant} (per head {per_head}), most moves of one row {moves}, "
                  f"largest single move {dmax:.1f}, heads {desc}: scores up to {deep:.1f} under m_run")
            assert share >= 0.20, (l, share)
            assert int(st["trig"][:, list(ctrl)].sum()) == 0 and float(st["moves"][:, list(ctrl)].max()) == 0.0, l
            assert moves >= 4 and dmax > 24.0 and deep > 100.0, (l, moves, dmax, deep)
        # the crafting stays out of the other blocks: block 0 of a crafted slot moves nothing
        assert name == "con" or int(_stats(s, 0)["trig"].sum()) == 0


@pytest.mark.parametrize("name", ["con", "emo", "sty"])
def test_bars_are_measured_and_faults_would_be_noticed(name, monkeypatch):
    from oracle import audio_oracle as ao
    s = _slot(name)
    W, W64, fb, taps = s["W"], s["W64"], s["fb"], s["taps"]
    # the committed feature reference of the GPU test is this float64 oracle's
    gold = np.load(GOLDEN / "audio_attn_cases.npz")[name]
    assert np.abs(gold - s["feat"].numpy()).max() <= 1e-9 * np.abs(gold).max()
    with torch.no_grad():
        monkeypatch.setattr(ao, "_rb", lambda x, on: _split16(x) if on else x)
        tapse = {}
        fe = ao.ast_forward(W, fb, True, emulate_bf16=True, taps=tapse)
        monkeypatch.undo()
        ferr = float((fe.double() - s["feat"]).abs().max() / s["feat"].abs().max())
        print(f"[attn cases] {name}: split-fp16 emulation, feature max / max {ferr:.2e}")
        # the feature bar is the contract's 1e-5 whatever the input, so the input has to be as well-conditioned as the stock slot (3.2e-6 on these clips):
        # recipe A with ramp heads emulated at 4.6e-6 .. 9.8e-6 depending on nothing but the summation order, and lost them for that reason
        assert ferr <= 0.4 * ac.FEATURE_BAR, (name, ferr)
        for l in ac.CRAFTED_BLOCKS:
            ref = taps[f"block{l}"]
            em = (ac.rel_l2(tapse[f"block{l}"], ref), ac.worst_token_rel_l2(tapse[f"block{l}"], ref))
            bars = ac.fp32x_bars(name, l)
            print(f"[attn cases] {name} block {l}: emulated rel-L2 {em[0]:.3e} worst token {em[1]:.3e} (recorded {ac.EMULATED[name, l][0]:.3e} "
                  f"{ac.EMULATED[name, l][1]:.3e}) -> GPU bars {bars[0]:.3e} {bars[1]:.3e}")
            # the record IS the measurement (fp32 summation order may differ between machines: 25 %), so the bars are max(1e-5, 4 x emulated)
            for got, rec in zip(em, ac.EMULATED[name, l]):
                assert 0.8 * rec <= got <= 1.25 * rec, (l, em, ac.EMULATED[name, l])
            # bf16: the rounding-point model in fp32 against itself accumulating in float64 - inside a quarter of the bars, which therefore stand
            x = taps[f"block{l - 1}"].float()
            model = ac.block_bf16_model(W, l, x, torch.float32)
            spread = ac.bf16_metrics(model, ac.block_bf16_model(W, l, x, torch.float64))
            print(f"[attn cases] {name} block {l}: bf16 model, fp32 vs float64 accumulation: max {spread[0]:.2e} mean {spread[1]:.2e} of max|x| "
                  f"(bars {ac.BF16_BARS[0]:.0e} {ac.BF16_BARS[1]:.0e})")
            assert spread[0] <= ac.BF16_BARS[0] / 4 and spread[1] <= ac.BF16_BARS[1] / 4, (l, spread)
            if ac.RECIPE[name] is None:
                continue
            # sensitivity, clip 0: a faulty rescale in the float64 chunk model, through the rest of the float64 block
            x0 = taps[f"block{l - 1}"][:1]
            good = ac.block_f64(W64, l, x0)
            assert ac.worst_token_rel_l2(ac.block_f64(W64, l, x0, chunked=True), good) < 1e-12       # the chunk rule itself is exact
            for fault in ("o", "l", "m"):
                bad = ac.block_f64(W64, l, x0, fault=fault)
                r = (ac.rel_l2(bad, good) / bars[0], ac.worst_token_rel_l2(bad, good) / bars[1])
                b = tuple(g / bar for g, bar in zip(ac.bf16_metrics(bad, good), ac.BF16_BARS))
                print(f"[attn cases] {name} block {l} fault {fault!r}: misses the fp32x bars {r[0]:.1e} x (rel-L2) {r[1]:.1e} x (worst token), the bf16 bars "
                      f"{b[0]:.1f} x (max) {b[1]:.1f} x (mean)")
                assert min(r) >= 10.0 and max(b) >= 10.0, (l, fault, r, b)
