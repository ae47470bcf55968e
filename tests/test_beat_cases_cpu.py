"""CPU: the inputs of tests/test_gpu_beat_align.py are fair, and the float64 restatement (tests/beat_ref.py) gives the answers the cases were built for.

Every equality the GPU test asserts on a computed envelope or on joint speeds is proven clear of its tie here, in float64: an onset decision by >= 1e-3 M (the
fp32 envelope differs from the float64 one by ~5e-6, measured below), a motion-beat decision by >= 1e-9 relative (fused multiply-adds move a double speed by
~1e-16).  The crafted plateau envelopes are exempt: they go to the pick stage as the same fp32 numbers on both sides, and the tie rule is what they test.
Also here: the restatement's beats equal scipy.signal.argrelextrema, closed-form known answers, and the BeatAlign accumulator (no GPU, no library call)."""
import numpy as np
import pytest

import beat_cases as bc
import beat_ref as br

from beat_cases import ENV_BAR, ENV_F32_GAP


def test_restatement_fft_and_frame_plan():
    x = np.random.default_rng(0).standard_normal((3, 512))
    re, im = br._fft512(x, np.float64)
    F = np.fft.fft(x)
    assert np.abs(re - F.real).max() < 1e-12 and np.abs(im - F.imag).max() < 1e-12
    assert [br.frames_of(n) for n in (0, 399, 400, 559, 560, 3120, 32000, 170000)] == [0, 0, 1, 1, 2, 18, 198, 1061]


def test_fp32_gap_of_the_envelope():
    """what fp32 arithmetic alone costs on the GPU test's waves: float64 against a float32 numpy restatement of the same steps; neither is the code under test"""
    worst = 0.0
    for n in bc.ENVELOPE_SAMPLES:
        for wave in (bc.click_train(n)[0], bc.two_tone(n)):
            e64, e32 = br.envelope(wave), br.envelope(wave, np.float32)
            assert e32.dtype == np.float32
            if len(e64):
                worst = max(worst, float(np.abs(e64 - e32.astype(np.float64)).max()))
    print(f"max |e64 - e32| = {worst:.3e} (recorded {ENV_F32_GAP:.3e}; the GPU bar is 8 x the record = {ENV_BAR:.3e})")
    assert 0.5 * ENV_F32_GAP <= worst <= ENV_F32_GAP


@pytest.mark.parametrize("n", [32000, 170000])
def test_click_train_onsets_are_the_bursts_with_clear_margins(n):
    wave, starts = bc.click_train(n)
    e = br.envelope(wave)
    mask, mg = br.margins(e)
    want = [bc.burst_frame(s) for s in starts]
    if n == 32000:
        assert want == [18, 48, 79, 123, 168]
    assert list(np.flatnonzero(mask)) == want
    print(f"n = {n}: {len(want)} onsets, smallest margin {mg.min():.3e} M, smallest pick margin {mg[mask == 1].min():.3e} M")
    assert mg.min() >= 1e-3 and mg[mask == 1].min() >= 0.1
    assert 1e-3 > 100 * ENV_BAR / float(e.max())          # the margin is two orders above what the fp32 envelope can move


def test_silence_and_short_waves():
    e = br.envelope(bc.silence())
    assert len(e) == 198 and np.array_equal(e, np.zeros(198)) and not br.pick(e).any()
    w399, w400 = bc.short_waves()
    assert len(br.envelope(w399)) == 0
    e = br.envelope(w400)
    assert len(e) == 1 and e[0] == 0.0 and not br.pick(e).any()          # e[0] = 0: M <= 0, no onset
    _, mg = br.margins(e)
    assert np.isinf(mg).all()


def test_crafted_envelopes_follow_the_tie_rule():
    cases = bc.crafted_envelopes()
    e, T, _ = cases["plateau: the first frame wins"]
    assert list(np.flatnonzero(br.pick(e, T))) == [10, 25]
    e, T, _ = cases["a peak at t = 0 and one at T - 1"]
    assert list(np.flatnonzero(br.pick(e, T))) == [0, 29]
    e, T, _ = cases["all zeros: no onset"]
    assert not br.pick(e, T).any()
    e, T, _ = cases["a constant plateau over the whole clip"]
    assert not br.pick(e, T).any()                                       # e = mean everywhere: never above mean + delta M
    e, T, _ = cases["T smaller than either window"]
    assert list(np.flatnonzero(br.pick(e, T))) == [1]
    for name, (e, T, _) in cases.items():                                # two onsets are always more than onset_window apart
        on = np.flatnonzero(br.pick(e, T))
        assert (np.diff(on) > 3).all(), name
    env, frames = bc.ragged_envelopes()
    for b in range(4):
        m = br.pick(env[b], int(frames[b]))
        assert not m[frames[b]:].any()


def _motion_cases():
    for N, F in bc.ALIGN_SHAPES:
        yield f"random {N}x{F}", bc.random_motion(N, F), np.full(N, F)
        X, L = bc.mixed_lengths(N, F)
        yield f"mixed {N}x{F}", X, L
    yield "dipping 1x60", bc.dipping_motion(1, 60), np.array([60])
    yield "dipping 3x300", bc.dipping_motion(3, 300), np.array([300] * 3)


def test_motion_cases_have_clear_margins_and_match_scipy():
    from scipy.signal import argrelextrema
    worst = np.inf
    for name, X, L in _motion_cases():
        for n in range(len(X)):
            s = br.speeds(X[n], int(L[n]), 30.0)
            assert np.isfinite(s).all(), name
            for j in range(bc.NJ):
                for k in (1, 3):
                    b = br.beats_of(s[:, j], k)
                    assert np.array_equal(np.flatnonzero(b), argrelextrema(s[:, j], np.less, order=k)[0]), (name, n, j, k)
                worst = min(worst, br.beat_margin(s[:, j], 3))
    print(f"smallest relative gap of a deciding comparison: {worst:.3e}")
    assert worst >= 1e-9
    # the static clip: every speed is exactly 0 in any arithmetic (x - x), so no frame is below another - exempt from the margin, exact by construction
    s = br.speeds(bc.static_motion(1, 8)[0], 8, 30.0)
    assert np.array_equal(s, np.zeros_like(s)) and not br.beats_of(s[:, 0], 3).any()
    for Ln, k in ((1, 1), (2, 1), (5, 3), (8, 3), (40, 1), (40, 3)):      # lengths of the speed series, as the definition's equality was checked
        v = np.random.default_rng(Ln).uniform(0, 1, Ln)
        assert np.array_equal(np.flatnonzero(br.beats_of(v, k)), argrelextrema(v, np.less, order=k)[0])


def test_dipping_motion_beats_are_the_dips_and_the_row_is_the_closed_form():
    X = bc.dipping_motion(1, 60)[0]
    s = br.speeds(X, 60, 30.0)
    for j in bc.CHOSEN:
        assert list(np.flatnonzero(br.beats_of(s[:, j], 3))) == list(bc.DIP_FRAMES)
    onsets = [18, 48, 79, 123, 168]                                      # the click train's
    mask = bc.onset_mask_at(onsets, 198)
    row, bm = br.align_row(mask, 198, X, 60)
    ta, tm = br.tau_audio(onsets), (np.array(bc.DIP_FRAMES) + 0.5) / 30.0
    delta = ta - tm                                                      # onset i is nearest to dip i, and the other way round: |delta| < 0.03 s, neighbours >= 0.3 s away
    assert np.abs(delta).max() < 0.03 and np.diff(tm).min() > 0.25 and np.diff(ta).min() > 0.25
    want = float(np.exp(-delta ** 2 / (2 * 0.1 ** 2)).sum())
    assert row[0] == 5
    for j in bc.CHOSEN:
        assert row[1 + j] == 5 and abs(row[56 + j] - want) < 1e-12 and abs(row[111 + j] - want) < 1e-12
        assert list(np.flatnonzero(bm[:, j])) == list(bc.DIP_FRAMES)
    ba, m2a = br.compute(row)
    assert abs(ba - want / 5) < 1e-12 and abs(m2a - want / 5) < 1e-12 and 0.9 < ba < 1.0
    # onsets after the motion's end are dropped everywhere: L = 40 keeps tau_a <= 1.3 s, i.e. four onsets
    row40, _ = br.align_row(mask, 198, X, 40)
    assert row40[0] == 4
    # a static clip: no beat, a2m = 0; silence: no onset, m2a = 0
    rs, bs = br.align_row(mask, 198, bc.static_motion(1, 60)[0], 60)
    assert rs[0] == 5 and not rs[1:].any() and not bs.any()
    rq, _ = br.align_row(np.zeros(198, np.uint8), 198, X, 60)
    assert rq[0] == 0 and rq[1 + 16] == 5 and not rq[56:].any()
    assert br.compute(rq) == (None, br.compute(rq)[1]) and br.compute(rs)[1] is None
    # a length outside 2..F: NaN
    assert np.isnan(br.align_row(mask, 198, X, 1)[0]).all() and np.isnan(br.align_row(mask, 198, X, 61)[0]).all()


def test_beat_align_accumulator_merges_and_names_its_nulls():
    from amuse_amd import beat_align as ba
    assert ba.ROW == br.ROW == 166 and [s.start for s in ba.ROW_SLICES.values()] == [0, 1, 56, 111]
    assert set(ba.split_row(np.zeros((2, 166)))) == {"n_onsets", "n_beats", "a2m", "m2a"}
    g = np.random.default_rng(0)
    rows = np.abs(g.standard_normal((5, 166))) + 1.0
    one = ba.BeatAlign()
    one.update(rows, [2.0] * 5, [1.9] * 5)
    a, b = ba.BeatAlign(), ba.BeatAlign()
    a.update(rows[:2], [2.0] * 2, [1.9] * 2)
    b.update(rows[2:], 6.0, 5.7)                                         # sums are taken as they come
    m = ba.BeatAlign.from_state(a.state()).merge(b)
    assert np.allclose(m.rows, one.rows, rtol=0, atol=1e-12) and m.clips == one.clips == 5 and abs(m.audio_s - 10.0) < 1e-12 and abs(m.motion_s - 9.5) < 1e-12
    c = one.compute()
    want_ba, want_m2a = br.compute(rows.sum(0))
    assert abs(c["BA"] - want_ba) < 1e-12 and abs(c["BA_motion_to_audio"] - want_m2a) < 1e-12
    assert abs(c["onsets_per_s"] - rows[:, 0].sum() / 10.0) < 1e-12 and c["joints"] == list(ba.DEFAULT_JOINTS)
    c2 = one.compute(joints=[0, 54])
    assert abs(c2["BA"] - float((rows.sum(0)[56:111][[0, 54]] / rows[:, 0].sum()).mean())) < 1e-12
    with pytest.raises(ValueError):
        one.compute(joints=[55])
    with pytest.raises(ValueError):
        one.update(np.full((1, 166), np.nan), 1.0, 1.0)
    # null with a reason where a denominator is 0
    z = ba.BeatAlign()
    e = z.compute()
    assert e["BA"] is None and "nothing" in e["BA_reason"] and e["onsets_per_s"] is None and e["motion_beats_per_s"] is None
    r = np.zeros((1, 166)); r[0, 1:56] = 3.0; r[0, 111:] = 1.5
    z.update(r, 2.0, 1.9)
    e = z.compute()
    assert e["BA"] is None and "onset" in e["BA_reason"] and abs(e["BA_motion_to_audio"] - 0.5) < 1e-12 and e["onsets_per_s"] == 0.0
    r2 = np.zeros((1, 166)); r2[0, 0] = 4.0
    q = ba.BeatAlign()
    q.update(r2, 2.0, 1.9)
    e = q.compute()
    assert e["BA"] == 0.0 and e["BA_motion_to_audio"] is None and "no motion beat" in e["BA_motion_to_audio_reason"]
    import json
    json.dumps({k: ba._plain(v) for k, v in e.items()}, allow_nan=False)
    assert ba.clip_seconds(32000, 60) == (59 / 30.0, 59 / 30.0) and ba.clip_seconds(16000, 60)[0] == 1.0
