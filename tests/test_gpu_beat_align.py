"""GPU: the beat alignment - amuse_beat_onsets / amuse_beat_pick / amuse_beat_align (csrc/k_beat.hip) against the float64 restatement (tests/beat_ref.py) on the
seeded cases of tests/beat_cases.py, end to end through BeatEngine and BeatAlign, and the command line.

Bars.
  envelope   |got - want| <= ENV_BAR = 8 x 4.63e-6 = 3.7e-5 absolute.  4.625e-6 is the largest difference, on exactly these waves, between the float64
             restatement and a float32 numpy restatement of the same steps (tests/test_beat_cases_cpu.py measures and holds it; neither is the code under test);
             the factor of 8 covers the kernel's different FFT twiddles and summation order (observed on the MI355X: at most 5.07e-6).  Frames beyond a
             clip's own and silence are exact zeros.
  pick       equalities.  The stage is double arithmetic on fp32 inputs both sides are given bit for bit, in the same order of operations.
  beats      equalities: tests/test_beat_cases_cpu.py proves every deciding comparison of these motions clear of its tie by >= 1e-9 relative.
  rows       |got - want| <= 1e-9 absolute: the project's bar for double sums of a few hundred terms <= 1 (tests/test_gpu_motion_metrics.py).
The click train's onsets on the GPU's own fp32 envelope equal the restatement's: their margins (>= 1.8e-2 M, proven on the CPU) are three orders above ENV_BAR."""
import functools
import json

import numpy as np
import pytest
import torch

import beat_cases as bc
import beat_ref as br
import body_cases as bodyc
from beat_cases import ENV_BAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-9


@pytest.fixture(scope="module")
def eng():
    from amuse_amd import beat_align as ba
    e = ba.BeatEngine(DEV)
    yield e
    e.close()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _env64(kind, n, nv):
    """the float64 envelope of one wave cut at nv samples: computed once, shared, read-only"""
    w = bc.click_train(n)[0] if kind == "click" else bc.two_tone(n, 11 if kind == "tone" else 12)
    e = br.envelope(w[:nv])
    e.setflags(write=False)
    return e


def _wave(kind, n):
    return bc.click_train(n)[0] if kind == "click" else bc.two_tone(n, 11 if kind == "tone" else 12)


@pytest.mark.parametrize("n", bc.ENVELOPE_SAMPLES)
@pytest.mark.parametrize("B", [1, 3])
def test_envelope_vs_restatement(eng, B, n):
    T = br.frames_of(n)
    kinds = ("click", "tone", "tone2")
    runs = [(("click",), None), (("tone",), None)] if B == 1 else [(kinds, None), (kinds, (n, min(399, n - 1), 400 + 160 * (T // 2) + 37 if T > 1 else 400))]
    for ks, nvs in runs:
        waves = np.stack([_wave(k, n) for k in ks])
        env, mask = eng.onsets(torch.from_numpy(waves), None if nvs is None else torch.tensor(nvs, dtype=torch.int32))
        env, mask = _np(env), _np(mask)
        assert env.shape == (len(ks), T) and mask.shape == (len(ks), T) and env.dtype == np.float32
        for b, k in enumerate(ks):
            nv = n if nvs is None else min(nvs[b], n)
            want = _env64(k, n, nv)
            Tb = len(want)
            err = float(np.abs(env[b, :Tb] - want).max()) if Tb else 0.0
            print(f"B {B} n {n} {k} n_valid {nv}: T_b {Tb}, max |e - e64| = {err:.3e} (bar {ENV_BAR:.3e}), max e {float(want.max()) if Tb else 0:.3f}")
            assert err <= ENV_BAR
            assert np.array_equal(env[b, Tb:], np.zeros(T - Tb, np.float32)) and not mask[b, Tb:].any()       # beyond the clip's own frames: exactly 0
            if Tb:
                assert env[b, 0] == 0.0
        # amuse_beat_onsets' mask is exactly amuse_beat_pick on its own envelope output
        frames = [len(_env64(k, n, n if nvs is None else min(nvs[b], n))) for b, k in enumerate(ks)]
        again = _np(eng.pick(torch.from_numpy(env), torch.tensor(frames, dtype=torch.int32)))
        assert np.array_equal(mask, again)
        for b in range(len(ks)):                                                                                 # and the restatement's pick of those fp32 numbers
            assert np.array_equal(mask[b], br.pick(env[b], frames[b]))


def test_click_train_onsets_silence_and_short_waves(eng):
    for n in (32000, 170000):
        wave, starts = bc.click_train(n)
        _, mask = eng.onsets(torch.from_numpy(wave.copy()))
        assert list(np.flatnonzero(_np(mask)[0])) == [bc.burst_frame(s) for s in starts]
    env, mask = eng.onsets(torch.from_numpy(np.stack([bc.silence(), bc.click_train(32000)[0]])))
    env, mask = _np(env), _np(mask)
    assert np.array_equal(env[0], np.zeros(198, np.float32)) and not mask[0].any() and mask[1].sum() == 5      # silence: an envelope of exactly 0
    w399, w400 = bc.short_waves()
    env, mask = eng.onsets(torch.from_numpy(w399.copy()))
    assert tuple(env.shape) == (1, 0) and tuple(mask.shape) == (1, 0)                                            # T = 0: nothing to write
    env, mask = eng.onsets(torch.from_numpy(w400.copy()))
    assert _np(env).tolist() == [[0.0]] and _np(mask).tolist() == [[0]]
    # ragged: a clip with n_valid < 400 beside a whole one
    env, mask = eng.onsets(torch.from_numpy(np.stack([bc.click_train(32000)[0]] * 2)), torch.tensor([250, 32000], dtype=torch.int32))
    assert not _np(env)[0].any() and not _np(mask)[0].any() and _np(mask)[1].sum() == 5


def test_pick_vs_restatement(eng):
    for name, (e, T, _) in bc.crafted_envelopes().items():
        got = _np(eng.pick(torch.from_numpy(e.copy())[None], torch.tensor([T], dtype=torch.int32)))[0]
        assert np.array_equal(got, br.pick(e, T)), name
    e, T, _ = bc.crafted_envelopes()["plateau: the first frame wins"]
    assert list(np.flatnonzero(_np(eng.pick(torch.from_numpy(e.copy())[None], [T]))[0])) == [10, 25]
    env, frames = bc.ragged_envelopes()
    got = _np(eng.pick(torch.from_numpy(env.copy()), torch.from_numpy(frames.copy())))
    for b in range(4):
        assert np.array_equal(got[b], br.pick(env[b], int(frames[b]))), b
    assert not got[1].any() and got[0].any()
    # other parameters: windows beyond the clip, a zero offset
    for p in (br.params(onset_window=1, onset_avg_window=1), br.params(onset_window=100, onset_avg_window=2000, onset_delta=0.0), br.params(onset_delta=0.5)):
        got = _np(eng.pick(torch.from_numpy(env.copy()), torch.from_numpy(frames.copy()), p))
        for b in range(4):
            assert np.array_equal(got[b], br.pick(env[b], int(frames[b]), p)), (p, b)
    # the float64-proven envelopes of the click train, as fp32
    for n in (32000, 170000):
        wave, starts = bc.click_train(n)
        e32 = _env64("click", n, n).astype(np.float32)
        got = _np(eng.pick(torch.from_numpy(e32)[None], [len(e32)]))[0]
        assert np.array_equal(got, br.pick(e32)) and list(np.flatnonzero(got)) == [bc.burst_frame(s) for s in starts]


def _align(eng, mask, af, X, L=None, p=None):
    rows, beats = eng.align_rows(torch.from_numpy(np.array(mask)), torch.tensor(list(af), dtype=torch.int32), torch.from_numpy(np.array(X)).to(DEV),
                                 None if L is None else torch.from_numpy(np.array(L, dtype=np.int32)), p, return_beats=True)
    return _np(rows), _np(beats)


def _close(got, want, what):
    err = float(np.abs(got - want).max())
    print(f"{what}: max |got - want| = {err:.3e} (bar {BAR:.0e})")
    assert np.isfinite(got).all() and err <= BAR, (what, err)


@pytest.mark.parametrize("N,F", bc.ALIGN_SHAPES)
def test_align_vs_restatement(eng, N, F):
    m1, T = bc.audio_for(F)
    mask = np.stack([m1] * N)
    af = [T, T // 2, T][:N]
    full = np.full(N, F)
    X = bc.random_motion(N, F)
    rows, beats = _align(eng, mask, af, X)
    want, wb = br.align_rows(mask, af, X, full)
    assert np.array_equal(beats, wb)
    _close(rows, want, "random")
    assert np.array_equal(rows[:, :56], want[:, :56])                                                           # the counts are exact
    # onsets after the motion's end are dropped: the mask holds more than are counted
    kept = int((br.tau_audio(np.flatnonzero(m1)) <= (F - 1) / 30.0).sum())
    assert rows[0, 0] == kept < int(m1.sum())
    # mixed lengths {2, 3, F}, NaN at and beyond L: nothing of it reaches a row
    Xm, Lm = bc.mixed_lengths(N, F)
    rows, beats = _align(eng, mask, af, Xm, Lm)
    want, wb = br.align_rows(mask, af, Xm, Lm)
    assert np.isfinite(rows).all() and np.array_equal(beats, wb)
    _close(rows, want, "mixed lengths")
    # a static clip: no beat anywhere, a2m and m2a exactly 0; silence: no onset, a2m and m2a exactly 0
    rows, beats = _align(eng, mask, af, bc.static_motion(N, F))
    assert not beats.any() and np.array_equal(rows[:, 1:], np.zeros((N, 165))) and rows[0, 0] == kept
    rows, beats = _align(eng, np.zeros_like(mask), af, X)
    assert np.array_equal(rows[:, 0], np.zeros(N)) and np.array_equal(rows[:, 56:], np.zeros((N, 110))) and np.array_equal(beats, br.align_rows(mask, af, X, full)[1])
    # other parameters
    p = br.params(motion_order=1, sigma_s=0.05, fps=25.0)
    rows, beats = _align(eng, mask, af, X, None, p)
    want, wb = br.align_rows(mask, af, X, full, p)
    assert np.array_equal(beats, wb)
    _close(rows, want, "order 1, sigma 0.05, 25 fps")


@pytest.mark.parametrize("F", [8, 300])
def test_same_bits_alone_and_in_a_batch_and_nan_rows(eng, F):
    m1, T = bc.audio_for(F)
    X = bc.random_motion(3, F)
    alone, b_alone = _align(eng, m1[None], [T], X[1:2])
    for order in ([1, 0, 2], [0, 2, 1]):                                                                         # the clip first, then last, in a batch of 3
        rows, beats = _align(eng, np.stack([m1] * 3), [T] * 3, X[order])
        at = order.index(1)
        assert np.array_equal(rows[at], alone[0]) and np.array_equal(beats[at], b_alone[0])
    # a length outside 2..F: a row of NaN, a beat mask of 0, the neighbours untouched - even when that clip's joints are NaN throughout
    Xn = np.array(X)
    Xn[1] = np.nan
    for bad in (1, 0, -5, F + 1):
        rows, beats = _align(eng, np.stack([m1] * 3), [T] * 3, Xn, [F, bad, F])
        assert np.isnan(rows[1]).all() and not beats[1].any()
        ref, rb = _align(eng, np.stack([m1] * 2), [T] * 2, X[[0, 2]])
        assert np.array_equal(rows[[0, 2]], ref) and np.array_equal(beats[[0, 2]], rb)


def test_known_answer_and_end_to_end(eng):
    """the click train and the dipping motion through BeatEngine.onsets -> align_rows -> BeatAlign.compute, against the restatement's value and the closed form"""
    from amuse_amd import beat_align as ba
    wave, _ = bc.click_train(32000)
    X = bc.dipping_motion(1, 60)
    env, mask = eng.onsets(torch.from_numpy(wave.copy()))
    rows, beats = eng.align_rows(mask, [198], torch.from_numpy(np.array(X)).to(DEV), None, None, return_beats=True)
    rows, beats = _np(rows), _np(beats)
    for j in bc.CHOSEN:
        assert list(np.flatnonzero(beats[0, :, j])) == list(bc.DIP_FRAMES)
    want_row, _ = br.align_row(br.pick(_env64("click", 32000, 32000)), 198, X[0], 60)
    _close(rows[0], want_row, "end to end")
    acc = ba.BeatAlign()
    acc.update(rows, *ba.clip_seconds(32000, 60))
    c = acc.compute()
    want_ba, want_m2a = br.compute(want_row)
    delta = br.tau_audio([18, 48, 79, 123, 168]) - (np.array(bc.DIP_FRAMES) + 0.5) / 30.0
    closed = float(np.exp(-delta ** 2 / 0.02).sum()) / 5
    print(f"BA {c['BA']:.12f} (restatement {want_ba:.12f}, closed form {closed:.12f}); motion->audio {c['BA_motion_to_audio']:.12f}")
    assert abs(c["BA"] - want_ba) <= BAR and abs(c["BA_motion_to_audio"] - want_m2a) <= BAR and abs(c["BA"] - closed) <= BAR
    assert c["n_onsets"] == 5 and abs(c["onsets_per_s"] - 5 / (59 / 30.0)) < 1e-12
    # L = 40: the onset at 1.69 s lies after the motion's end and is dropped everywhere
    r40 = _np(eng.align_rows(mask, [198], torch.from_numpy(np.array(X)).to(DEV), [40]))
    _close(r40[0], br.align_row(_np(mask)[0], 198, X[0], 40)[0], "L = 40")
    assert r40[0, 0] == 4


def _write_models(d):
    from amuse_amd import body
    d.mkdir()
    for i, f in enumerate(body.SMPLX_FILES.values()):
        body.BodyModel.from_dict(bodyc.make_model(203, seed=70 + i)).to_npz(d / f)
    return d


def test_cli_on_a_written_pair_and_a_44k_wav(eng, tmp_path):
    from scipy.io import wavfile
    from amuse_amd import beat_align as ba, body, npz_writer
    models_dir = _write_models(tmp_path / "smplx")
    aa, _, _ = bodyc.make_motion(1, 60, seed=9)
    g = np.random.default_rng(4)
    aa = (np.cumsum(g.standard_normal((60, 55, 3)) * 0.03, axis=0)).astype(np.float32)                          # a smooth-ish motion: beats exist
    fields = npz_writer.smplx_npz_fields(np.concatenate([aa.reshape(60, 165), np.zeros((60, 3), np.float32)], 1), "neutral", np.zeros(300))
    npz = tmp_path / "scott_seq_0_ABCDEF_motion_smplx.npz"
    np.savez(npz, **fields)
    pcm = np.round(bc.click_train(32000)[0] * 32767.0).astype(np.int16)
    wav = tmp_path / "clicks.wav"
    wavfile.write(wav, 16000, pcm)
    out = tmp_path / "ba.json"
    rep = ba.main([str(npz), str(wav), "--smplx-models", str(models_dir), "--out", str(out), "--device", DEV])
    js = json.loads(out.read_text())
    assert js["overall"]["BA"] == rep["overall"]["BA"] and js["per_file"][str(npz)]["n_onsets"] == 5 and "librosa" in js["note"]
    # the library path on the same inputs
    models = body.load_models(models_dir)
    be = body.BodyEngine(DEV, models["neutral"])
    try:
        be.set_subjects(np.zeros((1, 300), np.float32))
        J = be.joints(torch.from_numpy(fields["poses"][None]).to(DEV).contiguous(), torch.zeros(1, 60, 3, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), "aa")
    finally:
        be.close()
    _, mask = eng.onsets(torch.from_numpy(pcm.astype(np.float32) / 32768.0))
    acc = ba.BeatAlign()
    acc.update(eng.align_rows(mask, [198], J), *ba.clip_seconds(32000, 60))
    c = acc.compute()
    assert c["BA"] is not None and js["overall"]["BA"] == c["BA"] and js["overall"]["BA_motion_to_audio"] == c["BA_motion_to_audio"]
    # --joints and --sigma reach the computation
    rep2 = ba.main([str(npz), str(wav), "--smplx-models", str(models_dir), "--out", str(out), "--device", DEV, "--joints", "20", "21", "--sigma", "0.05"])
    assert rep2["overall"]["joints"] == [20, 21] and rep2["params"]["sigma_s"] == 0.05 and rep2["overall"]["BA"] < acc.compute([20, 21])["BA"]
    # a 44.1 kHz WAV goes through the resampler: 2 s of clicks at 44.1 kHz -> finite values and the five onsets
    t44 = np.interp(np.arange(88200) / 44100.0, np.arange(32000) / 16000.0, bc.click_train(32000)[0].astype(np.float64))
    wav44 = tmp_path / "clicks44.wav"
    wavfile.write(wav44, 44100, np.round(t44 * 32767.0).astype(np.int16))
    rep3 = ba.main([str(npz), str(wav44), "--smplx-models", str(models_dir), "--out", str(out), "--device", DEV])
    v = rep3["per_file"][str(npz)]
    assert v["samples"] == 32000 and v["n_onsets"] >= 1 and np.isfinite(v["BA"]) and np.isfinite(v["BA_motion_to_audio"])
    # refusals before anything is loaded
    with pytest.raises(SystemExit):
        ba.main([str(npz), "--smplx-models", str(models_dir)])
    with pytest.raises(SystemExit):
        ba.main([str(npz), str(wav), "--smplx-models", str(tmp_path / "nowhere")])


def test_trainer_hook_writes_the_report_and_leaves_the_npz_alone(tmp_path):
    """the trainer's --beat-align step on pairs as the audio list records them: the JSON appears under <model_path>/viz, the NPZ keeps its bytes"""
    import types
    from scipy.io import wavfile
    from amuse_amd import body, npz_writer
    from amuse_amd.trainer import trainer
    models = body.load_models(_write_models(tmp_path / "smplx"))
    g = np.random.default_rng(6)
    aa = (np.cumsum(g.standard_normal((60, 55, 3)) * 0.03, axis=0)).astype(np.float32)
    npz = tmp_path / "scott_seq_0_ABCDEF_motion_smplx.npz"
    np.savez(npz, **npz_writer.smplx_npz_fields(np.concatenate([aa.reshape(60, 165), np.zeros((60, 3), np.float32)], 1), "male", np.zeros(300)))
    before = npz.read_bytes()
    wav = tmp_path / "clicks.wav"
    wavfile.write(wav, 16000, np.round(bc.click_train(32000)[0] * 32767.0).astype(np.int16))
    config = {"TRAIN_PARAM": {"latent_diffusion": {"smplx_data": True, "skip_trans": False}, "test": {"beat_align": True}}}
    tr = trainer(config, torch.device(DEV), model=types.SimpleNamespace(precision="fp32x"), model_path=tmp_path / "saved", stamp="s", body_models=models, rank=0, world=1)
    assert tr._beat_align_on()
    tr.beat_pairs = [(npz, wav)]
    path = tr._beat_align_write(7)
    assert path == tr.beat_align_path and path.name == "beat_align_s_E7.json" and path.parent.name == "viz"
    rep = json.loads(path.read_text())
    assert rep["precision"] == "fp32x" and rep["params"]["sigma_s"] == 0.1 and rep["overall"]["n_onsets"] == 5 and rep["overall"]["clips"] == 1
    assert np.isfinite(rep["overall"]["BA"]) and list(rep["files"]) == [str(npz)] and rep["files"][str(npz)]["wav"] == str(wav)
    assert npz.read_bytes() == before
    config["TRAIN_PARAM"]["test"]["beat_align"] = False
    assert not trainer(config, torch.device(DEV), model=None, model_path=tmp_path / "saved", stamp="t", body_models=models, rank=0, world=1)._beat_align_on()
