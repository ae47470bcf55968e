"""A numpy restatement of every definition of the beat-alignment extension (include/amuse_hip.h, the amuse_beat block): the kaldi log-mel, the spectral-flux
envelope, the onset pick, the motion beats and the per-clip row.  float64 throughout by default; envelope(..., dtype=np.float32) restates the SAME steps in
float32 (its distance from the float64 one is the measure of what fp32 arithmetic alone costs: the GPU test's bar is 8 x that).  Neither is the code under
test.  This is the project's own statement of the metric: nothing here is librosa's or BEAT's code, and nothing is compared with either.

The tables come from amuse_amd.audio.kaldi_tables() (mel [128][257], window [400])."""
import numpy as np

NJ = 55
RATE, HOP, WIN, NFFT, NMEL = 16000, 160, 400, 512, 128
FLOOR = 1.1920929e-07
ROW = 166
DEFAULTS = dict(sigma_s=0.1, onset_delta=0.07, onset_window=3, onset_avg_window=10, motion_order=3, fps=30.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def frames_of(n: int) -> int:
    return 0 if n < WIN else 1 + (n - WIN) // HOP


def _tables():
    from amuse_amd import audio
    return audio.kaldi_tables()


def _fft512(y, dtype):
    """radix-2 decimation in time on [T, 512] real rows, every operation in `dtype` (the twiddles are rounded to it) -> (re, im)"""
    T = y.shape[0]
    idx = np.arange(NFFT)
    rev = np.zeros(NFFT, np.int64)
    for b in range(9):
        rev |= ((idx >> b) & 1) << (8 - b)
    re = np.ascontiguousarray(y[:, rev]).astype(dtype)      # re[r] = y[i] with r = bitreverse(i): rev is an involution
    im = np.zeros((T, NFFT), dtype)
    ln = 2
    while ln <= NFFT:
        half = ln // 2
        k = np.arange(half)
        ang = -2.0 * np.pi * k / ln
        cs, sn = np.cos(ang).astype(dtype), np.sin(ang).astype(dtype)
        r, i = re.reshape(T, NFFT // ln, ln), im.reshape(T, NFFT // ln, ln)
        ur, ui, vr, vi = r[:, :, :half].copy(), i[:, :, :half].copy(), r[:, :, half:].copy(), i[:, :, half:].copy()
        tr, ti = vr * cs - vi * sn, vr * sn + vi * cs
        r[:, :, :half], i[:, :, :half] = ur + tr, ui + ti
        r[:, :, half:], i[:, :, half:] = ur - tr, ui - ti
        ln *= 2
    return re, im


def logmel(wave, dtype=np.float64):
    """S [T, 128]: the kaldi fbank log energy before any normalisation, every step in `dtype`"""
    banks, window = _tables()
    x = np.asarray(wave).astype(dtype).reshape(-1)
    T = frames_of(x.size)
    if T == 0:
        return np.zeros((0, NMEL), dtype)
    fr = x[(np.arange(T) * HOP)[:, None] + np.arange(WIN)[None, :]]
    fr = fr - (fr.sum(1, dtype=dtype) * dtype(1.0 / 400.0))[:, None]                       # DC removal
    fr = (fr - dtype(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], 1)) * window.astype(dtype)[None, :]    # pre-emphasis (the first against itself), window
    y = np.zeros((T, NFFT), dtype)
    y[:, :WIN] = fr
    re, im = _fft512(y, dtype)
    P = (re * re + im * im)[:, :257]
    B = banks.astype(dtype)
    e = np.zeros((T, NMEL), dtype)
    for k in range(257):                                                                    # bins in ascending order
        e += P[:, k, None] * B[None, :, k]
    return np.log(np.maximum(e, dtype(FLOOR)))


def envelope(wave, dtype=np.float64):
    """e [T] in `dtype`: e[0] = 0, e[t] = (1/128) sum_m max(0, S[t][m] - S[t-1][m])"""
    S = logmel(wave, dtype)
    e = np.zeros(S.shape[0], dtype)
    if S.shape[0] > 1:
        e[1:] = np.maximum(S[1:] - S[:-1], dtype(0)).sum(1, dtype=dtype) * dtype(1.0 / 128.0)
    return e


def envelope_batch(waves, n_valid=None, dtype=np.float64):
    """[B, T] with T from the common length; clip b uses its first n_valid[b] samples, frames beyond its own are 0"""
    waves = np.asarray(waves)
    B, n = waves.shape
    T = frames_of(n)
    out = np.zeros((B, T), dtype)
    frames = []
    for b in range(B):
        nv = n if n_valid is None else int(min(max(int(n_valid[b]), 0), n))
        e = envelope(waves[b, :nv], dtype)
        out[b, :len(e)] = e
        frames.append(len(e))
    return out, np.asarray(frames, np.int64)


def pick(env, T=None, p=None):
    """onset mask [len(env)] (uint8) of the first T frames of an envelope; everything after the load is double, the window mean is the ascending sum"""
    p = p or DEFAULTS
    env = np.asarray(env)
    e = env.astype(np.float64)
    T = len(e) if T is None else int(min(max(T, 0), len(e)))
    mask = np.zeros(len(e), np.uint8)
    if T == 0:
        return mask
    M = float(e[:T].max())
    if not M > 0.0:
        return mask
    w, a = int(p["onset_window"]), int(p["onset_avg_window"])
    thr = float(p["onset_delta"]) * M
    for t in range(T):
        c = e[t]
        if any(not c > e[t - i] for i in range(1, w + 1) if t - i >= 0):
            continue
        if any(not c >= e[t + i] for i in range(1, w + 1) if t + i < T):
            continue
        lo, hi = max(0, t - a), min(T - 1, t + a)
        s = 0.0
        for k in range(lo, hi + 1):
            s = s + e[k]
        if c >= s / (hi - lo + 1) + thr:
            mask[t] = 1
    return mask


def margins(env, T=None, p=None):
    """For every frame of a float64 envelope: (mask, margin) where margin >= 0 says by how much (in units of M) the frame's decision is clear: a pick clears its
    threshold and every window neighbour by it; any other frame lies below its threshold, or below some window neighbour, by it."""
    p = p or DEFAULTS
    e = np.asarray(env, np.float64)
    T = len(e) if T is None else T
    mask = pick(e, T, p)
    M = float(e[:T].max()) if T else 0.0
    out = np.full(T, np.inf)
    if not M > 0.0:
        return mask, out
    w, a = int(p["onset_window"]), int(p["onset_avg_window"])
    for t in range(T):
        lo, hi = max(0, t - a), min(T - 1, t + a)
        d_thr = e[t] - (e[lo:hi + 1].mean() + p["onset_delta"] * M)
        nb = [e[t] - e[t - i] for i in range(1, w + 1) if t - i >= 0] + [e[t] - e[t + i] for i in range(1, w + 1) if t + i < T]
        if mask[t]:
            out[t] = min([d_thr] + nb) / M
        else:
            out[t] = max([-d_thr] + [-x for x in nb]) / M
    return mask, out


def speeds(X, L, fps):
    """[L - 1, 55] double: |X[f+1] - X[f]| fps on the fp32 joints"""
    X = np.asarray(X)[:L].astype(np.float64)
    d = X[1:] - X[:-1]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) * float(fps)


def beats_of(s, k):
    """mask [len(s)]: f is a beat iff s[f] < s[clip(f +- i)] for i = 1..k, strictly (an index that clips onto f fails)"""
    n = len(s)
    m = np.zeros(n, np.uint8)
    for f in range(n):
        ok = True
        for i in range(1, k + 1):
            if not (s[f] < s[min(max(f - i, 0), n - 1)] and s[f] < s[min(max(f + i, 0), n - 1)]):
                ok = False
                break
        m[f] = ok
    return m


def beat_margin(s, k):
    """smallest relative gap of the comparisons that DECIDE a frame: a beat's gap to each compared neighbour; for any other frame the largest gap by which a
    compared neighbour lies at or below it (an index clipped onto the frame itself decides with certainty: inf)"""
    n = len(s)
    worst = np.inf
    for f in range(n):
        nb = [min(max(f + d * i, 0), n - 1) for i in range(1, k + 1) for d in (-1, 1)]
        rel = lambda g: (s[g] - s[f]) / max(abs(s[g]), abs(s[f]), 1e-300)
        if all(s[f] < s[g] for g in nb):
            worst = min(worst, min(rel(g) for g in nb))
        else:
            worst = min(worst, max(np.inf if g == f else -rel(g) for g in nb))
    return worst


def tau_audio(t):
    return (160 * np.asarray(t, np.int64) + 200) / 16000.0


def align_row(onset_mask, audio_frames, X, L, p=None):
    """(row [166], beat mask [F, 55]) of one clip; a length outside 2..F gives NaN and an empty mask"""
    p = p or DEFAULTS
    X = np.asarray(X)
    F = X.shape[0]
    row, bm = np.zeros(ROW), np.zeros((F, NJ), np.uint8)
    if L < 2 or L > F:
        return np.full(ROW, np.nan), bm
    fps, k, s2 = float(p["fps"]), int(p["motion_order"]), 2.0 * float(p["sigma_s"]) * float(p["sigma_s"])
    Ta = int(min(max(audio_frames, 0), len(onset_mask)))
    on = np.flatnonzero(np.asarray(onset_mask)[:Ta])
    ta = tau_audio(on)
    ta = ta[ta <= (L - 1) / fps]
    row[0] = len(ta)
    s = speeds(X, L, fps)
    for j in range(NJ):
        b = beats_of(s[:, j], k)
        bm[:L - 1, j] = b
        tm = (np.flatnonzero(b) + 0.5) / fps
        row[1 + j] = len(tm)
        if len(tm) and len(ta):
            d2 = (ta[:, None] - tm[None, :]) ** 2
            acc = 0.0
            for v in d2.min(1):
                acc += np.exp(-v / s2)
            row[56 + j] = acc
            acc = 0.0
            for v in d2.min(0):
                acc += np.exp(-v / s2)
            row[111 + j] = acc
    return row, bm


def align_rows(onset_mask, audio_frames, joints, lengths, p=None):
    out = [align_row(onset_mask[n], int(audio_frames[n]), joints[n], int(lengths[n]), p) for n in range(len(joints))]
    return np.stack([r for r, _ in out]), np.stack([b for _, b in out])


def compute(rows_sum, joints=(16, 17, 18, 19, 20, 21)):
    """(BA, BA_motion_to_audio) of summed rows; None where a denominator is 0"""
    r = np.asarray(rows_sum, np.float64)
    j = list(joints)
    ba = float((r[56:111][j] / r[0]).mean()) if r[0] > 0 else None
    nb = r[1:56][j]
    m2a = float((r[111:166][j] / nb).mean()) if (nb > 0).all() else None
    return ba, m2a
