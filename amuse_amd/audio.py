"""Host side of the audio front-end (reference models/latent_diffusion/infer_ldm.py:180-193 process_single_seq):
waveform -> kaldi fbank -> 3 x AST -> (con, emo, sty).  All compute is in libamuse_hip.so (csrc/k_audio.hip); this
module only builds the two constant tables of the fbank, flattens the three state dicts and moves pointers."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import audio_weights as aw
from .engine import _ptr, flatten_state_dict

NORM_MEAN, NORM_STD = -9.173025, 5.062332   # configs/base_new.json TRAIN_PARAM.wav_dtw_mfcc.dataset_{mean,std}
WHICH = {"con": 0, "emo": 1, "sty": 2}
# include/amuse_hip.h amuse_audio_set_precision: "bf16" = the throughput arithmetic (default), "fp32x" = the parity mode (split-fp16 operands)
AUDIO_PREC = {"bf16": _lib.PREC_BF16, "fp32x": _lib.PREC_F32X}


def kaldi_tables() -> Tuple[np.ndarray, np.ndarray]:
    """(mel_banks [128, 257], hann window [400]) of kaldi fbank at 16 kHz / 25 ms / 512-point FFT / 20 Hz .. Nyquist
    (torchaudio.compliance.kaldi.get_mel_banks, window_type='hanning'; call site infer_ldm.py:182)."""
    f32 = np.float32
    mel = lambda f: f32(1127.0) * np.log(f32(1.0) + f / f32(700.0), dtype=f32)
    mel_low, mel_high = f32(1127.0 * math.log(1.0 + 20.0 / 700.0)), f32(1127.0 * math.log(1.0 + 8000.0 / 700.0))
    delta = f32((mel_high - mel_low) / f32(129))
    b = np.arange(128, dtype=f32)[:, None]
    left, center, right = mel_low + b * delta, mel_low + (b + f32(1)) * delta, mel_low + (b + f32(2)) * delta
    m = mel(f32(16000.0 / 512.0) * np.arange(256, dtype=f32))[None, :]
    up, down = (m - left) / (center - left), (right - m) / (right - center)
    banks = np.zeros((128, 257), dtype=f32)
    banks[:, :256] = np.maximum(np.minimum(up, down), f32(0))
    k = np.arange(400, dtype=np.float64)
    window = (0.5 - 0.5 * np.cos(2.0 * math.pi * k / 399.0)).astype(f32)
    return np.ascontiguousarray(banks), np.ascontiguousarray(window)


class AudioEngine:
    """One amuse_audio_ctx on one GPU: the three AST encoders of AST_EVP (models/audio/AST_EVP.py:53-61)."""

    def __init__(self, con_sd: Dict[str, np.ndarray], emo_sd: Dict[str, np.ndarray], sty_sd: Dict[str, np.ndarray],
                 device="cuda:0", norm_mean: float = NORM_MEAN, norm_std: float = NORM_STD, frame_based_feats: bool = True,
                 precision: str = "bf16", tail_sd: Optional[Dict[str, np.ndarray]] = None):
        self.lib = _lib.load()
        self.frame_based_feats = bool(frame_based_feats)
        self.has_tail = False
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmuseHipError("amuse_amd runs on an MI355X (torch device 'cuda:N'); there is no CPU path")
        spec = aw.ast_param_spec()
        flat = [flatten_state_dict(sd, spec) for sd in (con_sd, emo_sd, sty_sd)]
        banks, window = kaldi_tables()
        fp = C.POINTER(C.c_float)
        torch.cuda.init()
        self.ctx = self.lib.amuse_audio_create(self.device.index or 0, flat[0].ctypes.data_as(fp), flat[1].ctypes.data_as(fp),
                                               flat[2].ctypes.data_as(fp), flat[0].size, banks.ctypes.data_as(fp),
                                               window.ctypes.data_as(fp), norm_mean, norm_std, int(bool(frame_based_feats)))
        if not self.ctx:
            raise _lib.AmuseHipError(f"amuse_audio_create failed: {self.lib.amuse_last_error().decode()}")
        if precision != "bf16":
            self.set_precision(precision)
        if tail_sd is not None:
            self.set_tail(tail_sd)

    def set_tail(self, tail_sd: Dict[str, np.ndarray]) -> None:
        """Upload AST_EVP's classifier heads, fusion and decoder (audio_weights.ast_tail_param_spec; amuse_audio_set_tail): enables encode_labels'
        labels, reconstruct and metrics."""
        flat = flatten_state_dict(tail_sd, aw.ast_tail_param_spec())
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_set_tail(self.ctx, flat.ctypes.data_as(C.c_void_p), flat.size))
        self.has_tail = True

    def set_precision(self, precision: str) -> None:
        """"bf16" | "fp32x" (amuse_audio_set_precision): governs encode / features / features_ragged / process_single_seq; fbank is fp32 in both.
        The first switch to "fp32x" builds that mode's weight images (1.04 GB for the three encoders).  A refused value leaves the mode as it was."""
        if precision not in AUDIO_PREC:
            raise ValueError(f"audio precision must be one of {sorted(AUDIO_PREC)}, got {precision!r}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_set_precision(self.ctx, AUDIO_PREC[precision]))

    @property
    def precision(self) -> str:
        code = self.lib.amuse_audio_precision(self.ctx)
        return {v: k for k, v in AUDIO_PREC.items()}[code]

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.amuse_audio_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _waves(self, waves) -> torch.Tensor:
        w = torch.as_tensor(waves) if not isinstance(waves, torch.Tensor) else waves
        if w.dim() == 1:
            w = w[None]
        if w.dim() != 2:
            raise ValueError(f"waves must be (B, n_samples), got {tuple(w.shape)}")
        return w.to(device=self.device, dtype=torch.float32).contiguous()

    def fbank(self, waves) -> torch.Tensor:
        """(B, n) 16 kHz waveforms -> (B, 1024, 128) normalised, padded fbanks (infer_ldm.py:182-190)."""
        w = self._waves(waves)
        out = torch.empty(w.shape[0], 1024, 128, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_fbank(self.ctx, _ptr(w), w.shape[1], w.shape[0], _ptr(out), self._stream()))
        return out

    def encode(self, which: str, fbank, tap_block: Optional[int] = None):
        """ASTModel.forward(...)['feature'] of encoder 'con' | 'emo' | 'sty': (B, 1024, 128) -> (B, 256)
        (+ the fp32 residual stream (B, 1214, 768) after block `tap_block`, for tests)."""
        fb = torch.as_tensor(fbank).to(device=self.device, dtype=torch.float32).contiguous()
        if fb.dim() != 3 or tuple(fb.shape[1:]) != (1024, 128):
            raise ValueError(f"fbank must be (B, 1024, 128), got {tuple(fb.shape)}")
        B = fb.shape[0]
        feat = torch.empty(B, 256, device=self.device, dtype=torch.float32)
        hid = torch.empty(B, 1214, 768, device=self.device, dtype=torch.float32) if tap_block is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_encode(self.ctx, WHICH[which], _ptr(fb), B, _ptr(feat), _ptr(hid),
                                                   0 if tap_block is None else int(tap_block), self._stream()))
        return feat if tap_block is None else (feat, hid)

    def _fbanks(self, fbank) -> torch.Tensor:
        fb = torch.as_tensor(fbank).to(device=self.device, dtype=torch.float32).contiguous()
        if fb.dim() == 2:
            fb = fb[None]
        if fb.dim() != 3 or tuple(fb.shape[1:]) != (1024, 128):
            raise ValueError(f"fbank must be (B, 1024, 128), got {tuple(fb.shape)}")
        return fb

    def encode_labels(self, which: str, fbank, frame_based: Optional[bool] = None):
        """ASTModel.forward(fbank, frame_based_feats) of encoder 'con' | 'emo' | 'sty' (audio_main_new.py:174-204): -> (feature (B, 256), predicted_labels
        (B, 8) for 'emo', (B, 30) for 'sty', None for 'con', whose label_dim is 0).  frame_based None = the engine's flag."""
        fb = self._fbanks(fbank)
        B = fb.shape[0]
        feat = torch.empty(B, 256, device=self.device, dtype=torch.float32)
        logits = None if which == "con" else torch.empty(B, aw.TAIL_LABELS[which], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_encode_labels(self.ctx, WHICH[which], -1 if frame_based is None else int(bool(frame_based)), _ptr(fb), B,
                                                          _ptr(feat), _ptr(logits), self._stream()))
        return feat, logits

    def reconstruct(self, con, emo, sty, group: int = 1) -> torch.Tensor:
        """AST_EVP.reconstruct(cat(emo, sty, con), reconstruct_only=True) (AST_EVP.py:70-82): three (B, 256) embeddings -> (B, 1024, 128) fbanks.  The
        reference's layers see the batch as one sequence; `group` rows in a row form such a sequence here (group = B: the reference's call, group = 1: a clip
        on its own, as collect_audio_metrics runs it)."""
        ts = [torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous() for t in (con, emo, sty)]
        ts = [t[None] if t.dim() == 1 else t for t in ts]
        B = ts[0].shape[0]
        if any(tuple(t.shape) != (B, 256) for t in ts):
            raise ValueError(f"con / emo / sty must each be (B, 256), got {[tuple(t.shape) for t in ts]}")
        out = torch.empty(B, 1024, 128, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_reconstruct(self.ctx, _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), B, int(group), _ptr(out), self._stream()))
        return out

    def _tail_hidden(self, con, emo, sty, group: int = 1) -> torch.Tensor:
        """reconstruct up to the last Linear's input, (B, 1024) fp32 (amuse_debug_tail_hidden; tests)"""
        ts = [torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous() for t in (con, emo, sty)]
        B = ts[0].shape[0]
        out = torch.empty(B, 1024, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_debug_tail_hidden(self.ctx, _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), B, int(group), _ptr(out), self._stream()))
        return out

    def metrics(self, fbank) -> dict:
        """AST_EVP.eval_func(fbank, frame_based_feats, metrics=True) (AST_EVP.py:91-103) for ONE clip, (1, 1024, 128) or (1024, 128): the first pass is
        frame-based whatever the engine's flag (hard-coded at AST_EVP.py:93), the reconstruction is encoded again as it is, with the engine's flag.
        -> {"fbanks" (1024, 128), "emo" / "sty" / "con" and "new_emo" / "new_sty" / "new_con": {"feature" (256,), "predicted_labels" (1, L) | None}}."""
        fb = self._fbanks(fbank)
        if fb.shape[0] != 1:
            raise ValueError("metrics takes one clip, as collect_audio_metrics does (the reference squeezes the batch dimension)")
        first = {w: self.encode_labels(w, fb, True) for w in ("emo", "sty", "con")}
        fbanks = self.reconstruct(first["con"][0], first["emo"][0], first["sty"][0], group=1)
        second = {w: self.encode_labels(w, fbanks, self.frame_based_feats) for w in ("emo", "sty", "con")}
        out = {"fbanks": fbanks[0]}
        for w in ("emo", "sty", "con"):
            out[w] = {"feature": first[w][0][0], "predicted_labels": first[w][1]}
        for w in ("emo", "sty", "con"):
            out[f"new_{w}"] = {"feature": second[w][0][0], "predicted_labels": second[w][1]}
        return out

    def features(self, waves):
        """-> (con, emo, sty), each (B, 256): process_single_seq for a batch of waveforms."""
        w = self._waves(waves)
        B = w.shape[0]
        outs = [torch.empty(B, 256, device=self.device, dtype=torch.float32) for _ in range(3)]
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_audio_features(self.ctx, _ptr(w), w.shape[1], B, _ptr(outs[0]), _ptr(outs[1]),
                                                     _ptr(outs[2]), self._stream()))
        return tuple(outs)

    def features_ragged(self, waves: Sequence):
        """process_single_seq for waveforms of DIFFERENT lengths as one batch: a fbank launch per waveform (each is padded /
        cropped to 1024 frames on its own, as the reference does call by call), then every encoder once over all of them.
        Row k is bitwise what process_single_seq(waves[k]) returns: a clip's features do not depend on its batch."""
        if len(waves) == 0:
            raise ValueError("no waveforms")
        fb = torch.cat([self.fbank(torch.as_tensor(w)[0] if torch.as_tensor(w).dim() == 2 else w) for w in waves])
        return tuple(self.encode(which, fb) for which in ("con", "emo", "sty"))

    def process_single_seq(self, sliced_chunk, framerate=16000 // 2, baseline=False):
        """(C, n) or (n,) waveform -> (con, emo, sty), each (1, 256) (infer_ldm.py:180-193; channel 0 as kaldi does)."""
        w = torch.as_tensor(sliced_chunk)
        if w.dim() == 2:
            w = w[0]
        return self.features(w[None])
