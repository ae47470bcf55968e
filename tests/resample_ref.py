"""A float64 numpy restatement of the resampler (include/amuse_hip.h, "sample-rate conversion"): plan, bank, resample, the PCM decoding - the reference of the
CPU and GPU tests - and the same sum in float32, tap by tap in k order, which sets the GPU bars.  Nothing here comes from the library.

The filter's constants are a recollection of torchaudio.functional.resample's defaults; torchaudio is not part of this project, so this restatement (and
scipy.signal.upfirdn on the prototype filter, tests/test_resample_cpu.py) is all the resampler is pinned against.

sin / cos come from `math` (the C library's, as the host code's do), not from numpy's vectorised loops, so that the bank can be compared bit for bit."""
import math
from functools import lru_cache

import numpy as np

LPW, ROLLOFF = 6, 0.99
PCM_U8, PCM_S16, PCM_S32, PCM_F32 = 0, 1, 2, 3                       # include/amuse_hip.h AMUSE_PCM_*
FORMAT_OF = {np.dtype(np.uint8): PCM_U8, np.dtype(np.int16): PCM_S16, np.dtype(np.int32): PCM_S32, np.dtype(np.float32): PCM_F32}


def plan(rate_in: int, rate_out: int, n_in: int = 1) -> dict:
    g = math.gcd(rate_in, rate_out)
    M, L = rate_in // g, rate_out // g
    if rate_in == rate_out:                                           # the identity
        return {"M": 1, "L": 1, "Hw": 0, "K": 1, "n_out": n_in}
    base = ROLLOFF * min(M, L)
    Hw = math.ceil(LPW * M / base)
    return {"M": M, "L": L, "Hw": Hw, "K": 2 * Hw + 2, "n_out": -(-(n_in * L) // M)}


def _tap(t: float, scale: float) -> float:
    if not abs(t) < LPW:
        return 0.0
    pt = math.pi * t
    s = 1.0 if pt == 0.0 else math.sin(pt) / pt
    c = math.cos(pt / (2.0 * LPW))
    return scale * s * (c * c)


@lru_cache(maxsize=None)
def bank(rate_in: int, rate_out: int) -> np.ndarray:
    """h[L][K] in float64 (round with .astype(np.float32) for what the kernel reads)."""
    p = plan(rate_in, rate_out)
    M, L, Hw, K = p["M"], p["L"], p["Hw"], p["K"]
    if M == L:
        return np.ones((1, 1))
    base = ROLLOFF * min(M, L)
    h = np.zeros((L, K))
    for i in range(L):
        off = i * M // L - Hw
        for k in range(K):
            h[i, k] = _tap(base * ((off + k) / M - i / L), base / M)
    h.setflags(write=False)
    return h


def prototype(rate_in: int, rate_out: int):
    """The same formula sampled at t = base r / (M L) for integer r: (taps, index of the centre) - what scipy.signal.upfirdn applies with up = L, down = M."""
    p = plan(rate_in, rate_out)
    M, L = p["M"], p["L"]
    base = ROLLOFF * min(M, L)
    R = math.ceil(LPW * M * L / base)                                 # |t| < lpw  <=>  |r| < lpw M L / base
    return np.array([_tap(base * r / (M * L), base / M) for r in range(-R, R + 1)]), R


def decode(pcm: np.ndarray) -> np.ndarray:
    """Channel 0 of interleaved frames (n,) or (n, C), as amuse_amd.trainer.load_wav converts it -> float32 (n,)."""
    x = pcm if pcm.ndim == 1 else pcm[:, 0]
    if x.dtype == np.int16:
        return x.astype(np.float32) / np.float32(32768.0)
    if x.dtype == np.int32:
        return x.astype(np.float32) / np.float32(2147483648.0)
    if x.dtype == np.uint8:
        return (x.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    assert x.dtype == np.float32, x.dtype
    return x.copy()


def _gather(x: np.ndarray, rate_in: int, rate_out: int, m: np.ndarray, dtype, exact_bank: bool = False):
    """(h rows, x windows), both (len(m), K) in `dtype`: the operands of every output's sum, zeros outside the waveform."""
    p = plan(rate_in, rate_out, len(x))
    M, L, Hw, K = p["M"], p["L"], p["Hw"], p["K"]
    m = np.asarray(m, dtype=np.int64)
    j = (m * M // L - Hw)[:, None] + np.arange(K, dtype=np.int64)[None, :]
    inside = (j >= 0) & (j < len(x))
    xs = np.where(inside, x.astype(dtype)[np.clip(j, 0, len(x) - 1)], dtype(0))
    h = bank(rate_in, rate_out)
    return (h if exact_bank else h.astype(np.float32).astype(dtype))[m % L], xs


def resample(x: np.ndarray, rate_in: int, rate_out: int, m=None, exact_bank: bool = False) -> np.ndarray:
    """float64: y[m] = sum_k float32(h)[m mod L][k] x[floor(m M / L) - Hw + k] for every output (or the outputs `m`).  The bank is the fp32 one the kernel
    reads (exact_bank: the float64 one, for the comparison with scipy), the arithmetic float64."""
    if m is None:
        m = np.arange(plan(rate_in, rate_out, len(x))["n_out"])
    h, xs = _gather(x, rate_in, rate_out, m, np.float64, exact_bank)
    return (h * xs).sum(axis=1)


def resample_f32(x: np.ndarray, rate_in: int, rate_out: int, m=None) -> np.ndarray:
    """The same sum in float32, tap by tap in k order (one rounded product, one rounded add per tap)."""
    if m is None:
        m = np.arange(plan(rate_in, rate_out, len(x))["n_out"])
    h, xs = _gather(x, rate_in, rate_out, m, np.float32)
    acc = np.zeros(len(h), np.float32)
    for k in range(h.shape[1]):
        acc = acc + h[:, k] * xs[:, k]
    return acc


def bar(x: np.ndarray, rate_in: int, rate_out: int, m=None):
    """(bar, measured): 4 x the float32 restatement's own distance from the float64 one on this input, floor 2^-20 - both relative to max|y| (the rule of
    tests/body_grad_ref.py)."""
    y = resample(x, rate_in, rate_out, m)
    d = float(np.abs(resample_f32(x, rate_in, rate_out, m).astype(np.float64) - y).max()) / max(float(np.abs(y).max()), 1e-30)
    return max(4.0 * d, 2.0 ** -20), d
