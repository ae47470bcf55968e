"""CPU: the resampler without a GPU - the library's plan and bank (amuse_resample_plan / amuse_debug_resample_bank) against tests/resample_ref.py's restatement,
the restatement against known answers (scipy.signal.upfirdn on the prototype filter, impulses, shifts, tones: it is the GPU tests' reference), every refusal of
the entry points (made before any HIP call), and the switches: the command line's, and the long-form job list's sample counts.

The filter's constants are a recollection of torchaudio's defaults and are pinned against nothing outside this file (tests/resample_ref.py).

The bank: both sides compute it in double with the C library's sin / cos (the restatement through `math`), and on the machines this was written on the fp32
banks agree BIT FOR BIT; the assertion allows the 1 ulp (of fp32) that a C library whose sin / cos differ in the last place may cause, and prints which it is."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import resample_ref as rr
from amuse_amd import _lib, resample

ROWS = {48000: (3, 1, 19, 40, 40), 44100: (441, 160, 17, 36, 5760), 22050: (441, 320, 9, 20, 6400), 8000: (1, 2, 7, 16, 32), 96000: (6, 1, 37, 76, 76),
        11025: (441, 640, 7, 16, 10240)}                      # r_in -> 16000: M, L, Hw, K, bank floats
DC_RANGE = (1.00004, 1.00088)


def test_plan_table():
    for r_in, (M, L, Hw, K, floats) in ROWS.items():
        p = resample.plan(r_in, 16000, 1000)
        assert (p["down"], p["up"], p["taps"]) == (M, L, K) and K == 2 * Hw + 2 and L * K == floats, (r_in, p)
        q = rr.plan(r_in, 16000, 1000)
        assert (q["M"], q["L"], q["Hw"], q["K"], q["n_out"]) == (M, L, Hw, K, p["n_out"]), (r_in, q)
    assert resample.plan(16000, 16000, 321) == {"up": 1, "down": 1, "taps": 1, "n_out": 321}          # equal rates: the identity
    assert resample.bank(16000, 16000).tolist() == [[1.0]]


def test_output_count_sweep():
    lib = _lib.load()
    n_out = C.c_longlong()
    for r_in, (M, L, _, _, _) in ROWS.items():
        for n in range(1, 2001):
            assert lib.amuse_resample_plan(r_in, 16000, n, None, None, None, C.byref(n_out)) == 0
            assert n_out.value == -(-(n * L) // M) == rr.plan(r_in, 16000, n)["n_out"], (r_in, n)


def test_bank_matches_restatement():
    worst = 0
    for r_in, (M, L, Hw, K, _) in ROWS.items():
        got = resample.bank(r_in, 16000)
        ref64 = rr.bank(r_in, 16000)
        ref = ref64.astype(np.float32)
        assert got.shape == ref.shape == (L, K) and got.dtype == np.float32
        ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        worst = max(worst, int(ulps.max()))
        assert ulps.max() <= 1, (r_in, int(ulps.max()))
        for h in (ref64, got.astype(np.float64)):
            dc = h.sum(axis=1)
            assert DC_RANGE[0] - 2e-6 <= dc.min() and dc.max() <= DC_RANGE[1] + 2e-6, (r_in, dc.min(), dc.max())
        dc = ref64.sum(axis=1)
        assert DC_RANGE[0] <= round(float(dc.min()), 5) and round(float(dc.max()), 5) <= DC_RANGE[1], (r_in, dc.min(), dc.max())
    print("bank vs restatement: " + ("bit for bit" if worst == 0 else f"within {worst} ulp of fp32 (the host's sin / cos differ in the last place)"))


@pytest.mark.parametrize("r_in", [48000, 44100, 8000])
def test_restatement_equals_upfirdn_on_the_prototype(r_in):
    from scipy.signal import upfirdn
    p = rr.plan(r_in, 16000, 700)
    x = np.random.default_rng(r_in).standard_normal(700)
    proto, R = rr.prototype(r_in, 16000)
    pad = (-R) % p["M"]                                                   # the prototype's centre onto a multiple of M: output m is then sample c + m
    c = (R + pad) // p["M"]
    z = upfirdn(np.concatenate([np.zeros(pad), proto]), x, up=p["L"], down=p["M"])
    y = rr.resample(x, r_in, 16000, exact_bank=True)
    assert len(y) == p["n_out"] and len(z) >= c + len(y)
    assert np.abs(z[c:c + len(y)] - y).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize("r_in", [48000, 44100, 22050, 8000])
def test_restatement_impulse_gives_the_bank(r_in):
    p = rr.plan(r_in, 16000, 500)
    M, L, Hw, K = p["M"], p["L"], p["Hw"], p["K"]
    h32 = rr.bank(r_in, 16000).astype(np.float32)
    for j in (0, 3, 250, 499):
        x = np.zeros(500)
        x[j] = 1.0
        y = rr.resample(x, r_in, 16000)
        y32 = rr.resample_f32(x, r_in, 16000)
        hit = 0
        for m in range(p["n_out"]):
            k = j - (m * M // L - Hw)
            want = h32[m % L, k] if 0 <= k < K else np.float32(0)
            hit += 0 <= k < K
            assert y[m] == np.float64(want) and y32[m] == want, (r_in, j, m)
        assert hit > 0


@pytest.mark.parametrize("r_in", [48000, 44100, 22050, 8000])
def test_restatement_shift(r_in):
    p = rr.plan(r_in, 16000)
    M, L, Hw = p["M"], p["L"], p["Hw"]
    n = max(1500, 8 * M)
    x = np.random.default_rng(7).standard_normal(n)
    xd = np.concatenate([np.zeros(M), x])[:n]                            # delayed by M samples
    y, yd = rr.resample(x, r_in, 16000), rr.resample(xd, r_in, 16000)
    edge = (Hw + M) * L // M + L + 2                                      # outputs whose taps reach neither end, before and after the delay
    assert len(y) - L - 2 * edge > 50
    assert np.array_equal(yd[edge + L:len(y) - edge], y[edge:len(y) - edge - L])


def _tone(r_in, f, n=2000, phase=0.3):
    x = np.sin(2 * np.pi * f * np.arange(n) / r_in + phase)
    y = rr.resample(x, r_in, 16000)
    m = np.arange(len(y))
    ideal = np.sin(2 * np.pi * f * m / 16000 + phase)
    return y[40:-40], ideal[40:-40]


@pytest.mark.parametrize("r_in", [48000, 44100])
def test_restatement_tones_downsampling(r_in):
    for f in (1000, 3000):                                                # in band: the ideally sampled tone
        y, ideal = _tone(r_in, f)
        d = float(np.abs(y - ideal).max())
        print(f"{r_in} Hz, {f} Hz tone: distance from the ideally sampled tone {d:.2e} (bar 1e-3)")
        assert d <= 1e-3, (r_in, f, d)
    for f, bar in ((12000, 4e-3), (10000, 1.2e-2)):                       # beyond the new Nyquist: must fold to (next to) nothing
        y, _ = _tone(r_in, f)
        a = float(np.abs(y).max())
        print(f"{r_in} Hz, {f} Hz tone: output amplitude {a:.2e} (bar {bar:g})")
        assert a <= bar, (r_in, f, a)


def test_restatement_tone_upsampling():
    y, ideal = _tone(8000, 1000)
    d = float(np.abs(y - ideal).max())
    print(f"8000 Hz, 1000 Hz tone: distance from the ideally sampled tone {d:.2e} (bar 4e-4)")
    assert d <= 4e-4, d


def test_decode_is_load_wav(tmp_path):
    from scipy.io import wavfile
    from amuse_amd.trainer import load_wav, load_wav_rate, wav_header, wav_samples
    rng = np.random.default_rng(5)
    cases = {"s16": (rng.standard_normal((300, 2)) * 9000).astype(np.int16), "u8": rng.integers(0, 256, 300).astype(np.uint8),
             "s32": (rng.standard_normal(300) * 5e8).astype(np.int32), "f32": rng.standard_normal((300, 3)).astype(np.float32)}
    for k, (name, pcm) in enumerate(cases.items()):
        rate = (44100, 8000, 48000, 16000)[k]
        wavfile.write(tmp_path / f"{name}.wav", rate, pcm)
        wave, got_rate = load_wav_rate(tmp_path / f"{name}.wav")
        assert got_rate == rate and wav_header(tmp_path / f"{name}.wav") == (300, rate) and wav_samples(tmp_path / f"{name}.wav") == 300
        assert torch.equal(wave, load_wav(tmp_path / f"{name}.wav")) and np.array_equal(wave[0].numpy(), rr.decode(pcm)), name


def test_refusals_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.amuse_last_error().decode()
    plan = lambda ri, ro, n: lib.amuse_resample_plan(ri, ro, n, None, None, None, None)
    for bad in (3999, 384001, 0, -1):
        assert plan(bad, 16000, 10) == -1 and "outside" in err()
        assert plan(16000, bad, 10) == -1 and "outside" in err()
        assert lib.amuse_resampler_create(0, bad, 16000) is None and lib.amuse_debug_resample_bank(bad, 16000, None) == -1
    assert plan(4000, 384000, 10) == 0 and plan(384000, 4000, 10) == 0
    assert plan(44101, 16000, 10) == -1 and "cap" in err()               # 16000 phases of 36 taps: 2.2 MiB of coefficients
    assert lib.amuse_resampler_create(0, 44101, 16000) is None and "cap" in err()
    assert plan(48000, 16000, 0) == -1 and "n_in" in err() and plan(48000, 16000, -3) == -1
    with pytest.raises(_lib.AmuseHipError):
        resample.plan(44101, 16000, 10)
    # the call's own checks come before any HIP call: a resampler's host struct is enough (never dereferenced past its rates; the addresses are never read)
    class R(C.Structure):
        _fields_ = [("device", C.c_int), ("rate_in", C.c_int), ("rate_out", C.c_int), ("M", C.c_int), ("L", C.c_int), ("Hw", C.c_int), ("K", C.c_int), ("bank", C.c_void_p)]
    r = R(0, 48000, 16000, 3, 1, 19, 40, None)
    one = 0x1000
    call = lambda fmt=_lib.PCM_S16, ch=1, n=700, cap=234, pcm=one, out=one, h=C.byref(r): lib.amuse_resample(h, pcm, fmt, ch, n, out, cap, None)
    assert call(n=0) == -1 and "n_in" in err()
    assert call(ch=0) == -1 and "channels" in err() and call(ch=9) == -1 and "channels" in err()
    assert call(fmt=4) == -1 and "format" in err() and call(fmt=-1) == -1
    assert call(cap=233) == -1 and "out_capacity" in err()                # ceil(700 / 3) = 234
    assert call(pcm=None) == -1 and call(out=None) == -1 and call(h=None) == -1
    r.rate_in = 44101
    assert call() == -1 and "cap" in err()
    r.rate_in = 1000
    assert call() == -1 and "outside" in err()
    with pytest.raises(_lib.AmuseHipError, match="no CPU fallback"):
        resample.resample(torch.zeros(1, 100), 48000, device="cpu")


class _StubModel:
    """process_seq_list alone (tests/test_longform_cpu.py): an embedding that names its chunk's length"""
    device = "cpu"

    def __init__(self):
        self.seen = []

    def process_seq_list(self, chunks, framerate=16000, baseline=False):
        self.seen += [tuple(c.shape) for c in chunks]
        return [tuple(torch.full((1, 256), float(c.shape[1] + i)) for i in range(3)) for c in chunks]


def _strip(jobs):
    return [{k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in j.items()} for j in jobs]


def test_switches_and_long_form_job_list(tmp_path):
    from conftest import make_reference_tree
    from scipy.io import wavfile
    from amuse_amd import longform, main as cli
    from amuse_amd.trainer import trainer
    root = make_reference_tree(tmp_path / "tree")
    # the command line: accepted by the two inference entry points' parser, refused for training
    with pytest.raises(SystemExit, match="--resample belongs to"):
        cli.main(["--fn", "train_gesture", "--root", str(root), "--resample"])
    with pytest.raises(SystemExit, match="--long-form belongs to"):            # (parsed: the refusal is --long-form's, not the parser's)
        cli.main(["--fn", "edit_gesture", "--root", str(root), "--resample", "--long-form"])
    d = root / "viz_dump/test/speech"
    for p in d.glob("*.wav"):
        p.unlink()
    rng = np.random.default_rng(6)
    n441 = 25 * 44100
    wavfile.write(d / "scott_0_0_0.wav", 44100, (rng.standard_normal(n441) * 3000).astype(np.int16))
    wavfile.write(d / "scott_0_1_1.wav", 16000, (rng.standard_normal(400000) * 3000).astype(np.int16))
    audios = sorted(d.glob("*.wav"))
    config, _ = cli.load_config(root, "infer_gesture", None)
    config["TRAIN_PARAM"]["test"].update(long_form=True, hop_frames=270)
    W16, Wraw = longform.plan(400000, 270)["windows"], longform.plan(n441, 270)["windows"]
    assert (W16, Wraw) == (3, 8)
    off = trainer(config, "cpu", model=_StubModel(), rank=0, world=1)
    assert off._long_form_samples(audios) == [n441, 400000]
    jobs_off, _ = off._long_form_jobs(audios)                               # the switch off: the file's own sample count, as before
    assert [j["bsz"] for j in jobs_off] == [Wraw, W16] and jobs_off[0]["long_form"]["frames"] == 3 * n441 // 1600
    config = copy.deepcopy(config)                                          # (`off` keeps the configuration without the key)
    config["TRAIN_PARAM"]["test"]["resample"] = True
    on = trainer(config, "cpu", model=_StubModel(), rank=0, world=1)
    assert on._long_form_samples(audios) == [400000, 400000]                 # 25 s at 16 kHz, from the header and amuse_resample_plan alone
    # the job list on two ranks: the rank that does NOT own the 44.1 kHz file builds its job from the header alone - the window count of the 16 kHz length, not of
    # the file's own sample count; the rank that owns it goes on to the resampler, which has no CPU path to fall back to
    remote = owner = 0
    for rank in range(2):
        try:
            jobs, mine = trainer(config, "cpu", model=_StubModel(), rank=rank, world=2)._long_form_jobs(audios[:1])
        except _lib.AmuseHipError as e:
            assert "no CPU fallback" in str(e)
            owner += 1
            continue
        remote += 1
        assert not mine[0] and jobs[0]["remote"] and jobs[0]["bsz"] == W16 != Wraw and jobs[0]["long_form"] == {"frames": 750, "hop": 270}
    assert (remote, owner) == (1, 1)
    # a 16 kHz file: the same job list with and without the switch, and the resampler is never reached (there is no GPU here to reach it on)
    a16 = [audios[1]]
    j_on, _ = on._long_form_jobs(a16)
    j_off, _ = off._long_form_jobs(a16)
    assert _strip(j_on) == _strip(j_off) and j_on[0]["bsz"] == W16
    assert torch.equal(on._load_wave(audios[1]), off._load_wave(audios[1]))
    # the switch off: a 44.1 kHz file is loaded as it is
    from amuse_amd.trainer import load_wav
    assert torch.equal(off._load_wave(audios[0]), load_wav(audios[0]))
