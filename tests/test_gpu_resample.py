"""GPU: the resampler (csrc/k_resample.hip through amuse_resampler_create / amuse_resample) against tests/resample_ref.py's float64 restatement, and the path
built on it (PretrainedLPDM_v1.infer_long(sample_rate=...), the trainer's switch).

The bar of every comparison is resample_ref.bar's: 4 x the float32 restatement's own distance from the float64 one on the same input, floor 2^-20, relative to
max|y| (the rule of tests/body_grad_ref.py).  Measured when this was written: the float32 restatement sits 1.1e-8 .. 2.8e-7 from float64 (about 2e-7 from 700
samples up), so the bars are the floor, 9.5e-7, or just above it (up to 1.1e-6); the kernel (one fma per tap, so one rounding where the restatement has two) sits in
the same range, 1.1e-8 .. 2.8e-7.  The test prints every figure.
Impulse, shift and equal rates are exact: bitwise, no tolerance.

A workgroup is 256 output samples.  8000 -> 16000 Hz doubles the count, so its n_out is always even: its "one more than whole workgroups" case leaves TWO
samples in the last workgroup, the fewest that rate can leave."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import resample_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOCK = 256         # csrc/amuse_resample_host.hpp kResampleBlock
RATES = (48000, 44100, 22050, 8000)


def _gpu(pcm: np.ndarray, r_in: int, r_out: int = 16000) -> np.ndarray:
    from amuse_amd import resample
    y = resample.resample(pcm, r_in, device=DEV, rate_out=r_out)
    assert y.dtype == torch.float32 and y.dim() == 2 and y.shape[0] == 1 and y.is_cuda
    return y[0].cpu().numpy()


def _noise(rng, n, dtype, channels=1):
    shape = (n,) if channels == 1 else (n, channels)
    if dtype == np.int16:
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    if dtype == np.int32:
        return rng.integers(-2 ** 31, 2 ** 31, shape).astype(np.int32)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape).astype(np.uint8)
    return rng.standard_normal(shape).astype(np.float32)


def _tail_length(r_in):
    """the smallest n_in >= 600 whose n_out leaves the fewest samples the rate can leave in a last workgroup (1; 2 where n_out is always even)"""
    want = 2 if rr.plan(r_in, 16000)["L"] % 2 == 0 and rr.plan(r_in, 16000)["M"] == 1 else 1
    n = 600
    while rr.plan(r_in, 16000, n)["n_out"] % BLOCK != want:
        n += 1
    return n


def _compare(pcm, r_in, label, m=None):
    x = rr.decode(pcm)
    got = _gpu(pcm, r_in)
    ref = rr.resample(x, r_in, 16000, m)
    assert got.shape == (rr.plan(r_in, 16000, len(x))["n_out"],) and np.isfinite(got).all()
    bar, f32 = rr.bar(x, r_in, 16000, m)
    err = float(np.abs(got.astype(np.float64)[slice(None) if m is None else m] - ref).max()) / max(float(np.abs(ref).max()), 1e-30)
    print(f"{label}: kernel {err:.2e} from float64 (float32 restatement {f32:.2e}, bar {bar:.2e})")
    assert err <= bar, (label, err, bar)
    return got


@pytest.mark.parametrize("r_in", RATES)
def test_kernel_against_float64_restatement(r_in):
    rng = np.random.default_rng(r_in)
    Hw = rr.plan(r_in, 16000)["Hw"]
    tail = _tail_length(r_in)
    n_tail = rr.plan(r_in, 16000, tail)["n_out"]
    assert n_tail > BLOCK and n_tail % BLOCK in (1, 2)
    for k, n in enumerate((1, Hw - 1, 700, tail)):
        dtype = (np.int16, np.float32)[k % 2]
        _compare(_noise(rng, n, dtype), r_in, f"{r_in} Hz, n_in {n}, {np.dtype(dtype).name} mono")
        other = (np.float32, np.int16)[k % 2]
        if n in (700, tail):
            _compare(_noise(rng, n, other), r_in, f"{r_in} Hz, n_in {n}, {np.dtype(other).name} mono")


def test_formats_and_channel_zero_only():
    rng = np.random.default_rng(11)
    _compare(_noise(rng, 700, np.uint8), 44100, "44100 Hz, uint8 mono")
    _compare(_noise(rng, 700, np.int32), 48000, "48000 Hz, int32 mono")
    _compare(_noise(rng, 700, np.uint8, 3), 22050, "22050 Hz, uint8 3 channels")
    # int16 stereo, channel 1 full-scale noise: the mono result, bit for bit
    st = _noise(rng, 700, np.int16, 2)
    st[:, 1] = rng.choice(np.array([-32768, 32767], np.int16), 700)
    got = _compare(st, 44100, "44100 Hz, int16 stereo (channel 1 full scale)")
    assert np.array_equal(got, _gpu(np.ascontiguousarray(st[:, 0]), 44100))
    # float32 stereo, channel 1 NaN: finite, and the mono result bit for bit - channel 1 is never read
    for r_in in (48000, 8000):
        f = _noise(rng, 700, np.float32, 2)
        f[:, 1] = np.nan
        got = _gpu(f, r_in)
        assert np.isfinite(got).all() and np.array_equal(got, _gpu(np.ascontiguousarray(f[:, 0]), r_in)), r_in
    f8 = _noise(rng, 300, np.float32, 8)
    f8[:, 1:] = np.nan
    assert np.array_equal(_gpu(f8, 22050), _gpu(np.ascontiguousarray(f8[:, 0]), 22050))


@pytest.mark.parametrize("r_in", RATES)
def test_impulse_gives_the_bank_bitwise(r_in):
    from amuse_amd import resample
    p = rr.plan(r_in, 16000, 900)
    M, L, Hw, K = p["M"], p["L"], p["Hw"], p["K"]
    h = resample.bank(r_in, 16000)
    m = np.arange(p["n_out"])
    for j in (0, 5, 450, 899):
        x = np.zeros(900, np.float32)
        x[j] = 1.0
        k = j - (m * M // L - Hw)
        want = np.where((k >= 0) & (k < K), h[m % L, np.clip(k, 0, K - 1)], np.float32(0))
        got = _gpu(x, r_in)
        assert np.count_nonzero(want) > 0 and np.array_equal(got.view(np.int32), want.view(np.int32)), (r_in, j)


@pytest.mark.parametrize("r_in", RATES)
def test_shift_by_M_is_shift_by_L_bitwise(r_in):
    p = rr.plan(r_in, 16000)
    M, L, Hw = p["M"], p["L"], p["Hw"]
    n = max(1500, 8 * M)
    x = _noise(np.random.default_rng(3), n, np.int16)
    xd = np.concatenate([np.zeros(M, np.int16), x])[:n]
    y, yd = _gpu(x, r_in), _gpu(xd, r_in)
    edge = (Hw + M) * L // M + L + 2
    assert len(y) - L - 2 * edge > 50
    assert np.array_equal(yd[edge + L:len(y) - edge].view(np.int32), y[edge:len(y) - edge - L].view(np.int32))


def test_equal_rates_are_the_format_conversion_bitwise():
    rng = np.random.default_rng(4)
    for dtype in (np.uint8, np.int16, np.int32, np.float32):
        for ch in (1, 2):
            pcm = _noise(rng, 1000, dtype, ch)
            if dtype == np.float32:
                pcm.reshape(1000, -1)[:3, 0] = (-0.0, np.inf, 1e-42)          # signed zero, infinity, a subnormal: the bits pass
            got = _gpu(pcm, 16000, 16000)
            assert got.shape == (1000,) and np.array_equal(got.view(np.int32), rr.decode(pcm).view(np.int32)), (dtype, ch)


def test_long_waveforms_use_64_bit_indices():
    """3 x 2^20 samples at 48 kHz (12 MB of float32), and 14,000,000 int16 samples at 44.1 kHz, where m M passes 2^31 from output 4,869,579 on (n_out =
    5,079,366): 4,096 outputs at the start, the middle and the end of each."""
    rng = np.random.default_rng(5)
    for r_in, n, dtype in ((48000, 3 << 20, np.float32), (44100, 14_000_000, np.int16)):
        pcm = _noise(rng, n, dtype)
        n_out = rr.plan(r_in, 16000, n)["n_out"]
        m = np.concatenate([np.arange(4096), n_out // 2 + np.arange(4096), n_out - 4096 + np.arange(4096)])
        if r_in == 44100:
            assert int(m[-1]) * 441 > 2 ** 31 and n_out == 5079366
        _compare(pcm, r_in, f"{r_in} Hz, n_in {n}", m)


def test_repeat_calls_and_graph_replay():
    from amuse_amd import resample
    rng = np.random.default_rng(6)
    r = resample.Resampler.get(DEV, 44100)
    assert resample.Resampler.get(DEV, 44100) is r and resample.Resampler.get(DEV, 48000) is not r          # cached per rate pair
    pcm = torch.from_numpy(_noise(rng, 2000, np.int16, 2)).to(DEV)
    n_out = rr.plan(44100, 16000, 2000)["n_out"]
    out = torch.full((n_out + 7,), 123.0, device=DEV)
    e1, e2 = r(pcm).clone(), r(pcm, out=out).clone()
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and bool((out[n_out:] == 123.0).all())                                        # nothing past n_out is written
    g = torch.cuda.CUDAGraph()
    gout = torch.zeros(n_out, device=DEV)
    with torch.cuda.graph(g):                # the entry point allocates nothing, copies nothing and never synchronises
        r(pcm, out=gout)
    pcm.copy_(torch.from_numpy(_noise(rng, 2000, np.int16, 2)))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout[None], r(pcm)) and not torch.equal(gout[None], e1)


# ------------------------------------------------------------------ the path built on the kernel
@pytest.fixture(scope="module")
def model():
    from amuse_amd import audio_weights as aw
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))     # random-init front-end, as tests/test_gpu_longform.py builds its model
    m.precision = "fp32x"
    yield m
    m.audio_engine.close()
    m.engine.close()


def _speech(n, rate, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / rate
    w = 0.2 * torch.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 0.3 * t)) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64) + 0.01
    return (w.numpy() * 20000).astype(np.int16)


def test_infer_long_at_44100(model, tmp_path):
    from scipy.io import wavfile
    from amuse_amd import resample
    from amuse_amd.trainer import load_wav_rate
    n = 12 * 44100
    wavfile.write(tmp_path / "a.wav", 44100, _speech(n, 44100, 1))
    wave, rate = load_wav_rate(tmp_path / "a.wav")
    assert rate == 44100 and wave.shape == (1, n)
    assert model.num_inference_timesteps == 50
    model._clip_counter = 3
    on = model.infer_long([wave], sample_rate=44100)
    assert on[0]["poses"].shape == (360, 55, 3) and on[0]["trans"].shape == (360, 3) and bool(torch.isfinite(on[0]["poses"]).all())     # 12 s at 30 fps
    # the resampler's own output, passed as a 16 kHz waveform: the same poses, bit for bit
    w16 = resample.resample(wave, 44100, device=DEV).cpu()
    assert w16.shape == (1, 192000)
    model._clip_counter = 3
    for kw in ({}, {"sample_rate": 16000}):
        model._clip_counter = 3
        same = model.infer_long([w16], **kw)
        assert torch.equal(same[0]["poses"], on[0]["poses"]) and torch.equal(same[0]["trans"], on[0]["trans"])
    # without the rate the file is read as 16 kHz, as today: the frame count of its raw sample count
    model._clip_counter = 3
    off = model.infer_long([wave])
    assert off[0]["poses"].shape == (3 * n // 1600, 55, 3) == (992, 55, 3)


def test_trainer_switch(model, tmp_path):
    """in process, on one model, --long-form on: with the switch on the 12 s 44.1 kHz WAV becomes an NPZ of 360 frames (992 with it off) and the 16 kHz WAVs give
    the bytes they give with it off"""
    from conftest import make_reference_tree
    from scipy.io import wavfile
    from amuse_amd import main as cli
    from amuse_amd.trainer import trainer
    root = make_reference_tree(tmp_path / "tree", n_infer_wavs=2)
    wavfile.write(root / "viz_dump/test/speech/scott_9_441.wav", 44100, _speech(12 * 44100, 44100, 2))      # sorts after the two 16 kHz files
    config, _ = cli.load_config(root, "infer_gesture", None)
    config["TRAIN_PARAM"]["test"]["long_form"] = True

    def run(switch, stamp):
        config["TRAIN_PARAM"]["test"]["resample"] = switch
        model._clip_counter = 0
        random.seed(5)
        tr = trainer(config, torch.device(DEV), model=model, stamp=stamp)
        return tr.eval_prior_latdiff_forward_backward_v1(False, 0, True, False, modelversion="full", ammetric=True)
    off, on = run(False, "off"), run(True, "on")
    assert [p.name for p in off] == [p.name for p in on] and len(off) == 3
    assert off[0].read_bytes() == on[0].read_bytes() and off[1].read_bytes() == on[1].read_bytes()
    with np.load(off[2]) as z0, np.load(on[2]) as z1:
        assert z0["poses"].shape == (992, 55, 3) and z1["poses"].shape == (360, 55, 3) and z1["trans"].shape == (360, 3)
        assert np.isfinite(z1["poses"]).all()
