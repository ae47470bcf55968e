"""Sample-rate conversion in front of the audio front-end: a WAV at any rate becomes the 16 kHz waveform the fbank is built for (include/amuse_hip.h
amuse_resample_plan / amuse_resampler_create / amuse_resample; csrc/k_resample.hip).

AN EXTENSION, off by default - the reference never resamples: scripts/trainer.py:520 drops the file's rate, and a `set_frame_rate(16000)` line is commented out
at models/latent_diffusion/infer_ldm.py:444.  The filter (a Hann-windowed sinc, 6 zero crossings, roll-off 0.99, polyphase) is a RECOLLECTION of
torchaudio.functional.resample's defaults: torchaudio is not part of this project, the filter is pinned against its own float64 restatement and
scipy.signal.upfirdn only (tests/resample_ref.py).

The plan is the library's (`plan` calls it; nothing here restates its arithmetic), the filter is a HIP kernel; there is no other implementation."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib

TARGET_RATE = 16000        # the rate the front-end's fbank is built for (amuse_amd/audio.py sample_frequency)
_FORMATS = {torch.uint8: _lib.PCM_U8, torch.int16: _lib.PCM_S16, torch.int32: _lib.PCM_S32, torch.float32: _lib.PCM_F32}     # include/amuse_hip.h AMUSE_PCM_*
_PCM_DTYPES = tuple(np.dtype(t) for t in (np.uint8, np.int16, np.int32, np.float32))


def plan(rate_in: int, rate_out: int, n: int) -> dict:
    """amuse_resample_plan: {"up": L, "down": M, "taps": K, "n_out": ceil(n L / M)} for n samples at rate_in converted to rate_out.  No GPU needed.  Rates outside
    4,000..384,000 Hz, a rate pair whose bank of coefficients would pass 2 MiB and n < 1 raise AmuseHipError."""
    up, down, taps, n_out = C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
    _lib.check(_lib.load().amuse_resample_plan(int(rate_in), int(rate_out), int(n), C.byref(up), C.byref(down), C.byref(taps), C.byref(n_out)))
    return {"up": up.value, "down": down.value, "taps": taps.value, "n_out": n_out.value}


def bank(rate_in: int, rate_out: int = TARGET_RATE) -> np.ndarray:
    """amuse_debug_resample_bank: the fp32 coefficients [up][taps] the kernel reads.  No GPU needed."""
    p = plan(rate_in, rate_out, 1)
    h = np.empty((p["up"], p["taps"]), np.float32)
    _lib.check(_lib.load().amuse_debug_resample_bank(int(rate_in), int(rate_out), h.ctypes.data_as(C.POINTER(C.c_float))))
    return h


class Resampler:
    """One rate pair on one GPU: the bank of coefficients in device memory (built once; `Resampler.get` caches per device and rate pair)."""
    _cache: Dict[Tuple[int, int, int], "Resampler"] = {}

    def __init__(self, device, rate_in: int, rate_out: int = TARGET_RATE):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmuseHipError("the resampler runs on the GPU: amuse_amd has no CPU fallback")
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        plan(self.rate_in, self.rate_out, 1)         # the library's own refusals, before anything touches the GPU
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        self._h = _lib.load().amuse_resampler_create(index, self.rate_in, self.rate_out)
        if not self._h:
            raise _lib.AmuseHipError(f"amuse_resampler_create: {_lib.load().amuse_last_error().decode()}")

    @classmethod
    def get(cls, device, rate_in: int, rate_out: int = TARGET_RATE) -> "Resampler":
        d = torch.device(device)
        key = (d.index if d.index is not None else (torch.cuda.current_device() if d.type == "cuda" else -1), int(rate_in), int(rate_out))
        if key not in cls._cache:
            cls._cache[key] = cls(device, rate_in, rate_out)
        return cls._cache[key]

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().amuse_resampler_destroy(self._h)
            self._h = None
            for k in [k for k, v in self._cache.items() if v is self]:
                del self._cache[k]

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def __call__(self, pcm: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """pcm: device tensor (n,) or (n, C) of interleaved frames, uint8 / int16 / int32 / float32 -> (1, n_out) fp32 on the device (channel 0 only).  Runs on
        the current stream; allocates its output only (none when `out`, a contiguous fp32 device tensor of at least n_out elements, is given)."""
        if not pcm.is_cuda or pcm.device != self.device:
            raise ValueError(f"pcm must live on {self.device}, got {pcm.device}")
        pcm = pcm.contiguous()
        fmt = _FORMATS.get(pcm.dtype)
        if fmt is None or pcm.dim() not in (1, 2):
            raise ValueError(f"pcm must be (n,) or (n, C) frames of uint8 / int16 / int32 / float32, got {tuple(pcm.shape)} {pcm.dtype}")
        n, ch = int(pcm.shape[0]), (int(pcm.shape[1]) if pcm.dim() == 2 else 1)
        n_out = plan(self.rate_in, self.rate_out, n)["n_out"]
        if out is None:
            out = torch.empty(n_out, device=self.device, dtype=torch.float32)
        elif not (out.is_cuda and out.device == self.device and out.dtype == torch.float32 and out.is_contiguous()):
            raise ValueError("out must be a contiguous fp32 tensor on the resampler's device")
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().amuse_resample(self._h, C.c_void_p(pcm.data_ptr()), fmt, ch, n, C.c_void_p(out.data_ptr()), out.numel(),
                                                  torch.cuda.current_stream(self.device).cuda_stream))
        return out.reshape(-1)[:n_out][None]


def resample(wave_or_pcm, rate_in: int, device="cuda", rate_out: int = TARGET_RATE) -> torch.Tensor:
    """-> (1, n_out) fp32 on the device: channel 0 at rate_out.
    wave_or_pcm: a torch tensor is a WAVEFORM as trainer.load_wav returns it - (C, n) or (n,), float; channel 0 is uploaded; a numpy array is raw PCM as
    scipy.io.wavfile.read returns it - (n,) or (n, C) interleaved frames of uint8 / int16 / int32 / float32, uploaded as it is and converted in the kernel.
    A tensor already on a GPU stays there."""
    if isinstance(wave_or_pcm, np.ndarray):
        if wave_or_pcm.dtype not in _PCM_DTYPES or wave_or_pcm.ndim not in (1, 2):
            raise ValueError(f"raw PCM must be (n,) or (n, C) frames of uint8 / int16 / int32 / float32, got {wave_or_pcm.shape} {wave_or_pcm.dtype}")
        pcm = torch.from_numpy(np.ascontiguousarray(wave_or_pcm))
    else:
        w = torch.as_tensor(wave_or_pcm)
        pcm = (w[0] if w.dim() == 2 else w).to(torch.float32)
        if w.is_cuda:
            device = w.device
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.AmuseHipError("resample runs on the GPU: amuse_amd has no CPU fallback")
    return Resampler.get(dev, rate_in, rate_out)(pcm.to(dev))
