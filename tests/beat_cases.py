"""Seeded inputs of the beat-alignment tests.  Everything is built once per process and handed out READ-ONLY; tests/test_beat_cases_cpu.py proves in float64
that every decision the GPU test compares exactly (an onset, a motion beat) is clear of its tie by a margin no fp32 envelope or fused multiply-add can cross."""
import functools

import numpy as np

NJ = 55
RATE, HOP, WIN = 16000, 160, 400
BURSTS = (3200, 8000, 12960, 20000, 27200)                  # burst starts of the 2 s click train, in samples
CHOSEN = (16, 17, 18, 19, 20, 21)                           # the joints that slow down at known frames
DIP_FRAMES = (5, 15, 24, 37, 50)                            # motion frames (speeds) at which they do, for the 2 s / 60-frame clip
ENVELOPE_SAMPLES = (400, 560, 3120, 32000, 170000)          # T = 1, 2, 18, 198, 1061 (beyond 1024)
ENV_F32_GAP = 4.63e-6        # max |float64 envelope - float32 envelope| over the envelope test's waves: tests/test_beat_cases_cpu.py measures it (4.625e-06) and holds it
ENV_BAR = 8 * ENV_F32_GAP    # the GPU envelope's bar: a factor of 8 over that for the kernel's different FFT twiddles and summation order


def _ro(a):
    a.setflags(write=False)
    return a


def burst_frame(s: int) -> int:
    """the first envelope frame whose window reaches sample s"""
    return (s - WIN) // HOP + 1


@functools.lru_cache(maxsize=None)
def click_train(n: int = 32000, seed: int = 7):
    """decaying noise bursts of 0.1 s (amplitude 0.3) on a noise floor of 1e-3 randn (it keeps every mel bin well above the log floor); n = 32000: the five
    bursts of BURSTS; a longer wave repeats the pattern every 2 s.  -> (wave float32 [n], burst starts that lie wholly inside)"""
    g = np.random.default_rng(seed)
    w = 1e-3 * g.standard_normal(n)
    starts = []
    for rep in range(0, n, 32000):
        for s in BURSTS:
            s0 = rep + s
            if s0 + 1600 <= n:
                w[s0:s0 + 1600] += 0.3 * np.exp(-3.0 * np.arange(1600) / 1600.0) * g.standard_normal(1600)
                starts.append(s0)
    return _ro(w.astype(np.float32)), tuple(starts)


@functools.lru_cache(maxsize=None)
def two_tone(n: int, seed: int = 11):
    """220 Hz + 1370 Hz with a slow tremolo, plus noise at 1e-2: a dense envelope without clear onsets (envelope tests only, never an exact pick)"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    w = 0.2 * np.sin(2 * np.pi * 220.0 * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.1 * np.sin(2 * np.pi * 1370.0 * t + 0.3) + 1e-2 * g.standard_normal(n)
    return _ro(w.astype(np.float32))


def silence(n: int = 32000):
    return _ro(np.zeros(n, np.float32))


def short_waves():
    """399 samples (T = 0) and 400 samples (T = 1) of the click train's floor"""
    w, _ = click_train(32000)
    return _ro(w[:399].copy()), _ro(w[:400].copy())


# ------------------------------------------------------------------ crafted envelopes for the pick stage: (envelope float32 [T], frames, the tie rule is in play)
def crafted_envelopes():
    g = np.random.default_rng(3)
    out = {}
    e = np.zeros(40, np.float32); e[10:14] = 1.0; e[25] = 0.5
    out["plateau: the first frame wins"] = (e, 40, True)
    e = np.zeros(30, np.float32); e[0] = 1.0; e[29] = 0.8
    out["a peak at t = 0 and one at T - 1"] = (e, 30, False)
    for T in (1, 2, 7, 65, 1060):
        e = (g.uniform(0.0, 0.05, T) + (g.uniform(0, 1, T) < 0.08) * g.uniform(0.5, 1.0, T)).astype(np.float32)
        out[f"random peaks, T = {T}"] = (e, T, False)
    e = np.array([0.1, 0.9, 0.2], np.float32)
    out["T smaller than either window"] = (e, 3, False)
    out["all zeros: no onset"] = (np.zeros(50, np.float32), 50, False)
    e = np.full(20, 0.25, np.float32)
    out["a constant plateau over the whole clip"] = (e, 20, True)
    return {k: (_ro(v[0]), v[1], v[2]) for k, v in out.items()}


def ragged_envelopes():
    """[B = 4][T = 65] with frames (65, 0, 7, 33): the pick stage on ragged frames_dev, 0 included"""
    g = np.random.default_rng(5)
    e = (g.uniform(0.0, 0.05, (4, 65)) + (g.uniform(0, 1, (4, 65)) < 0.1) * g.uniform(0.5, 1.0, (4, 65))).astype(np.float32)
    return _ro(e), _ro(np.array([65, 0, 7, 33], np.int32))


# ------------------------------------------------------------------ motions
def _background(N, F, seed):
    """a random walk of every joint: steps of ~1 cm per frame -> speeds around 0.5 m/s with beats wherever they fall"""
    g = np.random.default_rng(seed)
    return np.cumsum(g.standard_normal((N, F, NJ, 3)) * 0.01, axis=1) + g.uniform(-0.5, 0.5, (N, 1, NJ, 3))


def dip_speed(F, dips):
    """[F - 1] speeds in m/s: 0.2 at each dip, rising by 0.1 per frame of distance to the nearest one - the dips are the only local minima"""
    f = np.arange(F - 1)
    return 0.2 + 0.1 * np.abs(f[:, None] - np.asarray(dips)[None, :]).min(1)


@functools.lru_cache(maxsize=None)
def dipping_motion(N: int = 1, F: int = 60, dips=DIP_FRAMES, seed: int = 21):
    """joints float32 [N, F, 55, 3]: the random-walk background, with the CHOSEN joints moving along one axis (joint j along axis j % 3) at dip_speed: their
    beats are exactly the dips that fit (a dip at the first or last speed clips onto itself and is none)"""
    X = _background(N, F, seed)
    dips = [d for d in dips if d <= F - 2]
    if dips:
        s = dip_speed(F, dips) / 30.0
        for j in CHOSEN:
            X[:, :, j, :] = X[:, :1, j, :]
            X[:, 1:, j, j % 3] += np.cumsum(s)[None, :]
    return _ro(X.astype(np.float32))


@functools.lru_cache(maxsize=None)
def random_motion(N: int, F: int, seed: int = 31):
    return _ro(_background(N, F, seed).astype(np.float32))


@functools.lru_cache(maxsize=None)
def static_motion(N: int, F: int, seed: int = 41):
    g = np.random.default_rng(seed)
    return _ro(np.broadcast_to(g.uniform(-1, 1, (N, 1, NJ, 3)), (N, F, NJ, 3)).astype(np.float32).copy())


@functools.lru_cache(maxsize=None)
def mixed_lengths(N: int, F: int, seed: int = 51):
    """lengths cycling through {2, 3, F} (cut at F), NaN at and beyond L_n -> (joints, lengths int32)"""
    X = _background(N, F, seed).astype(np.float32)
    L = np.array([min(v, F) for v in ([2, 3, F] * N)[:N]], np.int32)
    for n in range(N):
        X[n, L[n]:] = np.nan
    return _ro(X), _ro(L)


def onset_mask_at(frames, T):
    m = np.zeros(T, np.uint8)
    m[list(frames)] = 1
    return _ro(m)


ALIGN_SHAPES = [(N, F) for N in (1, 3) for F in (2, 3, 8, 65, 300)]


def audio_for(F: int, seed: int = 61):
    """a seeded onset mask for a motion of F frames at 30 fps: T covers the motion and a second beyond it (so that onsets after the motion's end exist), onsets
    4 to 40 frames apart -> (mask uint8 [T], T)"""
    g = np.random.default_rng(seed + F)
    T = int(np.ceil(F / 30.0 * 100.0)) + 100
    m = np.zeros(T, np.uint8)
    t = int(g.integers(0, 8))
    while t < T:
        m[t] = 1
        t += int(g.integers(4, 41))
    return _ro(m), T
