"""Preview video: the renderer's frames as a Motion-JPEG AVI with the speech (include/amuse_hip.h amuse_mjpeg_*, csrc/k_mjpeg.hip).

AN EXTENSION, off by default.  The reference ends a run with a Blender render and an ffmpeg mux; neither is rebuilt here.  JpegEncoder turns RGB frames that
are still in device memory into baseline JPEG files in HIP kernels (fixed Huffman tables, no chroma subsampling: a preview encoder, compared with libjpeg
through PIL only); AviWriter puts them, and 16-bit PCM audio, into an AVI 1.0 file with the standard library alone.  There is no CPU fallback for the encoder.

    python -m amuse_amd.render FILE_motion_smplx.npz --smplx-models DIR --video [--audio FILE.wav] [--quality 90]
    python -m amuse_amd.main --fn infer_gesture ... --preview --preview-video [--preview-quality 90]"""
from __future__ import annotations

import ctypes as C
import struct
from pathlib import Path
from typing import List, Optional

import numpy as np

from . import _lib

AVI_MAX_BYTES = 2 ** 31 - 1          # AVI 1.0: one RIFF chunk; OpenDML (the > 2 GB extension) is out of scope
AVIF_HASINDEX, AVIF_ISINTERLEAVED, AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def tables(quality: int):
    """amuse_mjpeg_tables: (luma, chroma) uint8 [64] in natural order; no GPU needed"""
    lu, ch = (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    _lib.check(_lib.load().amuse_mjpeg_tables(int(quality), lu, ch))
    return np.frombuffer(bytes(lu), np.uint8).copy(), np.frombuffer(bytes(ch), np.uint8).copy()


def plan(width: int, height: int, frames: int) -> dict:
    """amuse_mjpeg_plan: the library's own statement of the MCU grid, the header's length, the workspace and the worst case; no GPU needed"""
    mx, my, hb, ws, wc = C.c_int(), C.c_int(), C.c_int(), C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().amuse_mjpeg_plan(int(width), int(height), int(frames), C.byref(mx), C.byref(my), C.byref(hb), C.byref(ws), C.byref(wc)))
    return {"mcus_x": mx.value, "mcus_y": my.value, "header_bytes": hb.value, "workspace_bytes": ws.value, "worst_case_bytes_per_frame": wc.value}


def header(width: int, height: int, quality: int) -> bytes:
    """amuse_debug_mjpeg_header: SOI .. SOS of every frame of that size and quality; no GPU needed"""
    buf, n = (C.c_ubyte * 1024)(), C.c_int()
    _lib.check(_lib.load().amuse_debug_mjpeg_header(int(width), int(height), int(quality), buf, 1024, C.byref(n)))
    return bytes(buf[:n.value])


class JpegEncoder:
    """One image size at one quality on one GPU.  Calls are stream-ordered on torch's current stream."""

    def __init__(self, device, width: int, height: int, quality: int = 90):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmuseHipError("amuse_amd.video has no CPU fallback: the JPEG encoder is a HIP kernel family (tests/mjpeg_ref.py is a test's restatement)")
        self.width, self.height, self.quality, self.reserved = int(width), int(height), int(quality), 0
        self.ctx = self.lib.amuse_mjpeg_create(self.device.index or 0, self.width, self.height, self.quality)
        if not self.ctx:
            raise _lib.AmuseHipError(f"amuse_mjpeg_create: {self.lib.amuse_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.amuse_mjpeg_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, frames):
        import torch
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4 \
            and tuple(frames.shape[1:]) == (self.height, self.width, 3), f"frames: device uint8 [M, {self.height}, {self.width}, 3], contiguous"
        return int(frames.shape[0])

    def reserve(self, frames: int):
        if frames > self.reserved:
            _lib.check(self.lib.amuse_mjpeg_reserve(self.ctx, int(frames)))
            self.reserved = int(frames)

    def encode_into(self, frames, out, capacity: Optional[int] = None):
        """The call itself: frames into the device uint8 tensor `out`, of which only the first `capacity` bytes (default: all) may be written.
        -> (offsets int64 [M], sizes int32 [M], total int64 [1]) on the device (the bits are the library's unsigned values); nothing is synchronised."""
        import torch
        M = self._check(frames)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        capacity = out.numel() if capacity is None else int(capacity)
        assert 0 <= capacity <= out.numel()
        self.reserve(M)
        offsets = torch.empty(M, dtype=torch.int64, device=self.device)
        sizes = torch.empty(M, dtype=torch.int32, device=self.device)
        total = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.amuse_mjpeg_encode(self.ctx, frames.data_ptr(), M, out.data_ptr(), capacity, offsets.data_ptr(), sizes.data_ptr(), total.data_ptr(),
                                               self._stream()))
        return offsets, sizes, total

    def encode(self, frames) -> List[bytes]:
        """device uint8 [M, H, W, 3] -> M complete JPEG files.  `out` is allocated at the raw RGB size of the batch; if the files are larger (noise at a high
        quality), the call is made once more with exactly the total it reported."""
        import torch
        M = self._check(frames)
        out = torch.empty(M * self.height * self.width * 3, dtype=torch.uint8, device=self.device)
        offsets, sizes, total = self.encode_into(frames, out)
        n = int(total.item())
        if n > out.numel():
            out = torch.empty(n, dtype=torch.uint8, device=self.device)
            offsets, sizes, total = self.encode_into(frames, out)
            if int(total.item()) != n:
                raise _lib.AmuseHipError(f"amuse_mjpeg_encode: the total moved between two calls on the same frames ({n} -> {int(total.item())})")
        data = out[:n].cpu().numpy().tobytes()
        off, sz = offsets.cpu().tolist(), sizes.cpu().tolist()
        return [data[o:o + s] for o, s in zip(off, sz)]

    def coefficients(self, frames):
        """tests: the transform alone -> device int16 [M, mcus_y, mcus_x, 3, 64], zigzag order"""
        import torch
        M = self._check(frames)
        coef = torch.empty(M, -(-self.height // 8), -(-self.width // 8), 3, 64, dtype=torch.int16, device=self.device)
        _lib.check(self.lib.amuse_debug_mjpeg_coefficients(self.ctx, frames.data_ptr(), M, coef.data_ptr(), self._stream()))
        return coef


# ------------------------------------------------------------------ audio: the file's own samples as 16-bit PCM
def pcm16_from_float(x) -> np.ndarray:
    """float [channels, samples] in [-1, 1) -> int16 [samples, channels]: clip(round(x 32768), -32768, 32767)"""
    a = np.asarray(x, np.float64)
    if a.ndim == 1:
        a = a[None]
    return np.ascontiguousarray(np.clip(np.rint(a * 32768.0), -32768, 32767).astype(np.int16).T)


def clip_pcm16(waveform, clip: int, samples: int = 160000, rate: int = 16000):
    """Clip `clip` of a dataset take's `ld_waveform` - float (C, n) or (n,) at 16 kHz, a tensor or an array - as the AVI carries it: the samples
    [clip samples, (clip + 1) samples) -> (int16 [<= samples, C], rate); None when the waveform ends before the clip begins."""
    w = waveform.detach().cpu().numpy() if hasattr(waveform, "detach") else np.asarray(waveform)
    if w.ndim == 1:
        w = w[None]
    part = w[:, int(clip) * samples:(int(clip) + 1) * samples]
    return (pcm16_from_float(part), int(rate)) if part.shape[1] else None


def preview_wav(entry):
    """What the trainer recorded for an NPZ (trainer.preview_audio) -> what Previewer.preview takes as `wav`: a WAV path as it is; ("ld_waveform", waveform, c)
    as clip c's 16-bit PCM at 16 kHz; None (the video stream alone) for no entry"""
    if entry is None or isinstance(entry, (str, Path)):
        return entry
    return clip_pcm16(entry[1], entry[2])


def load_pcm16(path):
    """A WAV as the AVI carries it: (int16 [samples, channels], rate) - the file's own samples at the rate and channel count its header states, no mean removed,
    nothing resampled.  int16 data passes through bit for bit; every other format goes through trainer.load_wav_rate and pcm16_from_float."""
    from scipy.io import wavfile
    rate, data = wavfile.read(str(path))
    if data.dtype == np.int16:
        return np.ascontiguousarray(data.reshape(data.shape[0], -1)), int(rate)
    from .trainer import load_wav_rate
    x, rate = load_wav_rate(path)
    return pcm16_from_float(x.numpy()), int(rate)


# ------------------------------------------------------------------ AVI 1.0, on the standard library alone
def _chunk_header(tag: bytes, size: int) -> bytes:
    return tag + struct.pack("<I", size)


class AviWriter:
    """RIFF 'AVI ' { LIST hdrl { avih, LIST strl { strh vids/MJPG, strf BITMAPINFOHEADER }, [LIST strl { strh auds, strf WAVEFORMATEX PCM }] }, LIST movi, idx1 }.
    Frames are appended as they arrive, as '00dc' chunks padded to even length, each followed - when there is audio - by the '01wb' chunk of the samples
    [floor(k rate / fps), floor((k + 1) rate / fps)); what the audio holds beyond the last frame goes into one final chunk.  The sizes in the headers are
    patched on close(), so a long video never sits in memory (the index does: 16 bytes per chunk).  audio = (int16 [samples, channels], rate) or None.
    A file that would pass 2^31 - 1 bytes is refused (ValueError) before the chunk that would do it is written."""

    def __init__(self, path, width: int, height: int, fps: int = 30, audio=None):
        if int(fps) != fps or fps < 1 or width < 1 or height < 1:
            raise ValueError(f"AviWriter: {width} x {height} at {fps} frames per second: positive integers are required")
        self.path, self.width, self.height, self.fps = Path(path), int(width), int(height), int(fps)
        self.pcm, self.rate = None, 0
        if audio is not None:
            pcm, rate = audio
            pcm = np.asarray(pcm)
            if pcm.dtype != np.int16 or pcm.ndim != 2 or pcm.shape[1] < 1 or int(rate) < 1:
                raise ValueError(f"AviWriter: audio is (int16 [samples, channels], rate), got {pcm.dtype} {tuple(pcm.shape)} at {rate} Hz")
            self.pcm, self.rate = np.ascontiguousarray(pcm.astype("<i2", copy=False)), int(rate)
        self.frames, self.samples, self.max_chunk, self.index = 0, 0, 0, []
        self.f = open(self.path, "wb")
        self.f.write(self._headers())
        self.movi = self.f.tell() - 4            # the offset of the 'movi' fourcc: idx1 offsets count from here

    def _headers(self) -> bytes:
        """everything up to and including LIST movi's fourcc, with the counts known so far"""
        ch = self.pcm.shape[1] if self.pcm is not None else 0
        block = 2 * ch
        streams = 2 if ch else 1
        movi_bytes = getattr(self, "movi_bytes", 4)
        per_sec = (movi_bytes * self.fps) // max(self.frames, 1) if self.frames else 0
        avih = struct.pack("<14I", 1000000 // self.fps, per_sec, 0, AVIF_HASINDEX | (AVIF_ISINTERLEAVED if ch else 0), self.frames, 0, streams, self.max_chunk,
                           self.width, self.height, 0, 0, 0, 0)
        strh_v = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, 1, self.fps, 0, self.frames, self.max_chunk, 0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf_v = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + _chunk_header(b"strh", len(strh_v)) + strh_v + _chunk_header(b"strf", len(strf_v)) + strf_v
        hdrl = b"hdrl" + _chunk_header(b"avih", len(avih)) + avih + _chunk_header(b"LIST", len(strl)) + strl
        if ch:
            strh_a = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, block, self.rate * block, 0, self.samples, self.rate * block // self.fps + block,
                                 0xFFFFFFFF, block, 0, 0, 0, 0)
            strf_a = struct.pack("<HHIIHHH", 1, ch, self.rate, self.rate * block, block, 16, 0)
            strl = b"strl" + _chunk_header(b"strh", len(strh_a)) + strh_a + _chunk_header(b"strf", len(strf_a)) + strf_a
            hdrl += _chunk_header(b"LIST", len(strl)) + strl
        riff_bytes = getattr(self, "riff_bytes", 0)
        return _chunk_header(b"RIFF", riff_bytes) + b"AVI " + _chunk_header(b"LIST", len(hdrl)) + hdrl + _chunk_header(b"LIST", movi_bytes) + b"movi"

    def _append(self, tag: bytes, data: bytes):
        size = len(data)
        end = self.f.tell() + 8 + size + (size & 1) + 8 + 16 * (len(self.index) + 1)      # this chunk, then idx1 with one more entry
        if end > AVI_MAX_BYTES:
            raise ValueError(f"AviWriter: {self.path} would pass {AVI_MAX_BYTES} bytes (AVI 1.0 holds one RIFF chunk; OpenDML is not written): "
                             f"{self.frames} frames are in; use a smaller size, a lower quality or a shorter clip")
        self.index.append((tag, AVIIF_KEYFRAME, self.f.tell() - self.movi, size))
        self.f.write(_chunk_header(tag, size) + data + (b"\0" if size & 1 else b""))
        self.max_chunk = max(self.max_chunk, size)

    def _audio(self, upto: int):
        upto = min(upto, self.pcm.shape[0])
        if upto > self.samples:
            self._append(b"01wb", self.pcm[self.samples:upto].tobytes())
            self.samples = upto

    def write_frame(self, jpeg: bytes):
        self._append(b"00dc", jpeg)
        self.frames += 1
        if self.pcm is not None:
            self._audio(self.frames * self.rate // self.fps)

    def close(self):
        if self.f is None:
            return
        refused = None
        if self.pcm is not None:
            try:
                self._audio(self.pcm.shape[0])
            except ValueError as e:      # the tail would pass the size limit: what is in stays a valid file, then the refusal is raised
                refused = e
        end = self.f.tell()
        self.f.write(_chunk_header(b"idx1", 16 * len(self.index)) + b"".join(struct.pack("<4sIII", *e) for e in self.index))
        self.riff_bytes, self.movi_bytes = self.f.tell() - 8, end - self.movi
        self.f.seek(0)
        self.f.write(self._headers())
        self.f.close()
        self.f = None
        if refused is not None:
            raise refused

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
