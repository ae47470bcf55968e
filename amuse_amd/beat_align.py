"""Beat alignment - an extension, off by default: do the hands move with the voice?  Speech onsets of the 16 kHz waveform against the motion beats (local
minima of joint speed) of every SMPL-X joint, scored by how close the two sets lie in time.  Everything from the waveform and the posed joints to the per-clip
row runs in HIP (include/amuse_hip.h amuse_beat_*, csrc/k_beat.hip); this module moves pointers and divides sums.

This is THIS PROJECT'S OWN statement of the metric, in the manner of BEAT's `alignment` and of librosa's spectral-flux onset detector, both written down from
memory.  librosa is not on the build machine; nothing here is pinned against librosa or against BEAT's code, and no number this module gives has been compared
with either.  It is checked against its own float64 restatement (tests/beat_ref.py) and, for the motion beats, scipy.signal.argrelextrema.  DEVIATIONS, stated
(DESIGN.md 4.16): a kaldi log-mel (the front-end's tables) instead of librosa's mel spectrogram in dB; no normalisation of the envelope by its maximum (the
threshold offset is a fraction of the maximum instead); no greedy `wait` pass (the strict-left / loose-right maximum test already keeps onsets more than
onset_window frames apart); times are window centres; every joint is scored and the joints that enter BA are a parameter of compute(), not of the kernel.

  python -m amuse_amd.beat_align FILE_motion_smplx.npz FILE.wav [more pairs ...] --smplx-models DIR [--out JSON] [--joints 16 17 ...] [--sigma 0.1]"""
from __future__ import annotations

import ctypes as C
import json
from contextlib import closing
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

from .motion_metrics import _plain      # (JSON-ready values: one definition for both reports)

NJ = 55
FPS = 30.0                   # the NPZ's mocap_frame_rate (npz_writer.smplx_npz_fields)
RATE = 16000                 # the front-end's sample rate
HOP, WIN = 160, 400          # the fbank's frame shift and window, in samples
DEFAULT_JOINTS = (16, 17, 18, 19, 20, 21)     # SMPL-X shoulders, elbows, wrists

# The row of amuse_beat_align: (block, length) in order - include/amuse_hip.h states the same table, csrc/amuse_beat_host.hpp its offsets.  Every offset below
# comes from this table; tests hold its total to amuse_beat_align_row().
ROW_BLOCKS = (("n_onsets", 1), ("n_beats", NJ), ("a2m", NJ), ("m2a", NJ))
ROW = sum(n for _, n in ROW_BLOCKS)
ROW_SLICES: Dict[str, slice] = {}
_o = 0
for _name, _n in ROW_BLOCKS:
    ROW_SLICES[_name] = slice(_o, _o + _n)
    _o += _n
del _o, _name, _n


def split_row(rows) -> dict:
    """rows [..., 166] -> {block: [..., length]} (views)"""
    rows = np.asarray(rows)
    assert rows.shape[-1] == ROW, rows.shape
    return {k: rows[..., s] for k, s in ROW_SLICES.items()}


def default_params() -> dict:
    """amuse_beat_default_params: the library's own defaults, restated nowhere in Python"""
    from . import _lib
    p = _lib.BeatParamsC()
    _lib.check(_lib.load().amuse_beat_default_params(C.byref(p)))
    return {k: getattr(p, k) for k, _ in _lib.BeatParamsC._fields_}


def _params(params: Optional[dict]):
    from . import _lib
    p = _lib.BeatParamsC()
    _lib.check(_lib.load().amuse_beat_default_params(C.byref(p)))
    for k, v in (params or {}).items():
        if k not in dict(_lib.BeatParamsC._fields_):
            raise ValueError(f"beat_align: unknown parameter {k!r} (amuse_beat_params has {', '.join(k for k, _ in _lib.BeatParamsC._fields_)})")
        setattr(p, k, v)
    return p


def plan(n_samples: int) -> int:
    """amuse_beat_plan: envelope frames of a waveform of n_samples (needs no GPU)"""
    from . import _lib
    T = C.c_int(0)
    _lib.check(_lib.load().amuse_beat_plan(int(n_samples), C.byref(T)))
    return T.value


class BeatEngine:
    """One amuse_beat context on one GPU (it owns the fbank tables of audio.kaldi_tables()).  Every call works on torch device tensors, on torch's current
    stream; none synchronises."""

    def __init__(self, device="cuda:0"):
        import torch
        from . import _lib, audio
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AmuseHipError("amuse_amd runs on an MI355X (torch device 'cuda:N'); there is no CPU path")
        banks, window = audio.kaldi_tables()
        fp = C.POINTER(C.c_float)
        torch.cuda.init()
        self.ctx = self.lib.amuse_beat_create(self.device.index or 0, banks.ctypes.data_as(fp), window.ctypes.data_as(fp))
        if not self.ctx:
            raise _lib.AmuseHipError(f"amuse_beat_create: {self.lib.amuse_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.amuse_beat_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _i32(self, x, n, what):
        import torch
        x = torch.as_tensor(x).to(self.device, torch.int32).contiguous().reshape(-1)
        if x.numel() != n:
            raise ValueError(f"{what} is an int32 tensor [{n}], got {x.numel()} entries")
        return x

    def onsets(self, waves, n_valid=None, params: Optional[dict] = None):
        """waves float32 [B, n] (or [n]) at 16 kHz, n_valid int32 [B] (None: every clip has n samples) -> (envelope float32 [B, T], onset mask uint8 [B, T]),
        T = plan(n).  Frames beyond a clip's own count hold envelope 0 and mask 0."""
        import torch
        from . import _lib
        w = torch.as_tensor(waves)
        if w.dim() == 1:
            w = w[None]
        if w.dim() != 2 or w.shape[1] < 1:
            raise ValueError(f"waves must be (B, n_samples >= 1), got {tuple(w.shape)}")
        w = w.to(self.device, torch.float32).contiguous()
        B, n = int(w.shape[0]), int(w.shape[1])
        T = plan(n)
        nv = None if n_valid is None else self._i32(n_valid, B, "n_valid")
        env = torch.empty(B, T, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, T, dtype=torch.uint8, device=self.device)
        if T == 0:                # (torch gives an empty tensor no address, and the library refuses two NULL outputs: there is nothing to write)
            return env, mask
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_beat_onsets(self.ctx, w.data_ptr(), None if nv is None else nv.data_ptr(), n, B, C.byref(_params(params)),
                                                  env.data_ptr(), mask.data_ptr(), self._stream()))
        return env, mask

    def pick(self, envelope, frames, params: Optional[dict] = None):
        """the pick stage alone: envelope float32 [B, T], frames int32 [B] -> onset mask uint8 [B, T]"""
        import torch
        from . import _lib
        e = torch.as_tensor(envelope).to(self.device, torch.float32).contiguous()
        if e.dim() != 2 or e.shape[1] < 1:
            raise ValueError(f"envelope must be (B, T >= 1), got {tuple(e.shape)}")
        B, T = int(e.shape[0]), int(e.shape[1])
        fr = self._i32(frames, B, "frames")
        mask = torch.empty(B, T, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_beat_pick(e.data_ptr(), fr.data_ptr(), B, T, C.byref(_params(params)), mask.data_ptr(), self._stream()))
        return mask

    def align_rows(self, onset_mask, audio_frames, joints, lengths=None, params: Optional[dict] = None, return_beats: bool = False):
        """onset mask uint8 [N, T], audio_frames int32 [N], joints float32 [N, F, 55, 3] (amuse_body_forward's), lengths int32 [N] (None: every clip has F
        frames) -> rows float64 [N, 166] (+ the beat mask uint8 [N, F, 55] with return_beats).  A clip whose length lies outside 2..F gets a row of NaN."""
        import torch
        from . import _lib
        m = torch.as_tensor(onset_mask).to(self.device, torch.uint8).contiguous()
        J = torch.as_tensor(joints)
        if not (J.is_cuda and J.dtype == torch.float32 and J.is_contiguous()):
            raise ValueError("align_rows: joints are a device float32 tensor, contiguous")
        if J.dim() != 4 or tuple(J.shape[2:]) != (NJ, 3):
            raise ValueError(f"align_rows: joints must be [N, F, {NJ}, 3], got {tuple(J.shape)}")
        N, F = int(J.shape[0]), int(J.shape[1])
        if m.dim() != 2 or m.shape[0] != N:
            raise ValueError(f"align_rows: onset_mask must be [N = {N}, T], got {tuple(m.shape)}")
        T = int(m.shape[1])
        af = self._i32(audio_frames, N, "audio_frames")
        ln = torch.full((N,), F, dtype=torch.int32, device=self.device) if lengths is None else self._i32(lengths, N, "lengths")
        assert self.lib.amuse_beat_align_row() == ROW
        rows = torch.empty(N, ROW, dtype=torch.float64, device=self.device)
        beats = torch.empty(N, F, NJ, dtype=torch.uint8, device=self.device) if return_beats else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.amuse_beat_align(m.data_ptr() if T else None, af.data_ptr(), T, J.data_ptr(), ln.data_ptr(), N, F, C.byref(_params(params)),
                                                 rows.data_ptr(), beats.data_ptr() if return_beats else None, self._stream()))
        return (rows, beats) if return_beats else rows


class BeatAlign:
    """The additive accumulator: the SUM of the per-clip rows, the clip count, the seconds of audio and of motion.  Ranks and batches add."""

    def __init__(self):
        self.rows = np.zeros(ROW, np.float64)
        self.clips = 0
        self.audio_s = 0.0
        self.motion_s = 0.0

    def update(self, rows, audio_s, motion_s) -> None:
        """rows [n, 166] (or one row); audio_s / motion_s: the seconds each clip's onsets / beats were taken over, [n] or their sums"""
        rows = np.asarray(rows.detach().cpu().numpy() if hasattr(rows, "detach") else rows, np.float64).reshape(-1, ROW)
        if not np.isfinite(rows).all():
            raise ValueError("BeatAlign.update: a row is not finite (a clip's length outside 2..F gives a row of NaN)")
        self.rows += rows.sum(0)
        self.clips += len(rows)
        self.audio_s += float(np.sum(audio_s))
        self.motion_s += float(np.sum(motion_s))

    def state(self) -> dict:
        return {"rows": self.rows.copy(), "clips": int(self.clips), "audio_s": float(self.audio_s), "motion_s": float(self.motion_s)}

    def merge(self, other) -> "BeatAlign":
        st = other.state() if isinstance(other, BeatAlign) else other
        self.rows += np.asarray(st["rows"], np.float64)
        self.clips += int(st["clips"])
        self.audio_s += float(st["audio_s"])
        self.motion_s += float(st["motion_s"])
        return self

    @classmethod
    def from_state(cls, st: dict) -> "BeatAlign":
        return cls().merge(st)

    def compute(self, joints: Sequence[int] = DEFAULT_JOINTS) -> dict:
        """BA: the mean over `joints` of sum a2m[j] / sum n_onsets - how much of an onset has a motion beat of that joint near it;
        BA_motion_to_audio: the mean of sum m2a[j] / sum n_beats[j].  A value whose denominator is 0 is None, with a reason beside it."""
        joints = [int(j) for j in joints]
        if not joints or min(joints) < 0 or max(joints) >= NJ:
            raise ValueError(f"BeatAlign.compute: joints are indices in 0..{NJ - 1}, got {joints}")
        b = split_row(self.rows)
        n_on, n_b = float(b["n_onsets"][0]), b["n_beats"]
        out = {"clips": int(self.clips), "joints": joints, "n_onsets": n_on, "n_beats_per_joint": n_b.copy(),
               "audio_s": float(self.audio_s), "motion_s": float(self.motion_s)}
        nul = np.full(NJ, np.nan)
        out["BA_per_joint"] = b["a2m"] / n_on if n_on > 0 else nul
        with np.errstate(invalid="ignore", divide="ignore"):
            out["BA_motion_to_audio_per_joint"] = np.where(n_b > 0, b["m2a"] / np.where(n_b > 0, n_b, 1.0), np.nan)
        if self.clips < 1:
            out["BA"], out["BA_reason"] = None, "nothing was accumulated"
            out["BA_motion_to_audio"], out["BA_motion_to_audio_reason"] = None, "nothing was accumulated"
        else:
            if n_on > 0:
                out["BA"] = float(out["BA_per_joint"][joints].mean())
            else:
                out["BA"], out["BA_reason"] = None, "no speech onset was found: BA divides by their count"
            if all(n_b[j] > 0 for j in joints):
                out["BA_motion_to_audio"] = float(out["BA_motion_to_audio_per_joint"][joints].mean())
            else:
                out["BA_motion_to_audio"] = None
                out["BA_motion_to_audio_reason"] = f"joints {[j for j in joints if not n_b[j] > 0]} have no motion beat: BA_motion_to_audio divides by their count"
        if self.audio_s > 0:
            out["onsets_per_s"] = n_on / self.audio_s
        else:
            out["onsets_per_s"], out["onsets_per_s_reason"] = None, "no audio was accumulated"
        if self.motion_s > 0:
            out["motion_beats_per_s"] = float(n_b[joints].mean() / self.motion_s)
            out["motion_beats_per_s_per_joint"] = n_b / self.motion_s
        else:
            out["motion_beats_per_s"], out["motion_beats_per_s_reason"] = None, "no motion was accumulated"
        return out


def clip_seconds(n_samples: int, frames: int, fps: float = FPS):
    """(seconds of audio the onsets were taken over, seconds of motion the beats were taken over): the audio is cut at the motion's end, as the onsets are"""
    motion_s = max(frames - 1, 0) / fps
    return min(n_samples / RATE, motion_s), motion_s


# ------------------------------------------------------------------ pairs of files
def load_wave_16k(path, device, resample_other_rates: bool = True):
    """the existing reader (trainer.load_wav_rate); a file at another rate goes through the existing resampler (amuse_amd/resample.py) -> float32 [n] on device"""
    import torch
    from .trainer import load_wav_rate
    wave, rate = load_wav_rate(path)
    if rate != RATE and wave.shape[1] > 0 and resample_other_rates:
        from . import resample
        return resample.resample(wave, rate, device=device).reshape(-1)
    return wave[0].to(device, torch.float32).contiguous()


def score_pairs(pairs, models: dict, device="cuda:0", params: Optional[dict] = None, joints: Sequence[int] = DEFAULT_JOINTS, load_wave=None) -> dict:
    """pairs [(npz path, wav path), ...]: every NPZ is posed by its own gender's body model with its own betas (as motion_metrics.compare_directories does) and
    scored against its WAV.  load_wave(path) -> float32 [n] at 16 kHz replaces the default reader (the trainer passes the front-end's).  Needs no checkpoint.
    -> {"per_file": {npz: values}, "overall": values, "state": the additive state}"""
    import torch
    from . import body, motion_file
    par = dict(default_params(), **(params or {}))
    fps = float(par["fps"])
    total, per_file = BeatAlign(), {}
    with closing(BeatEngine(device)) as beat, closing(body.Poser(models, device)) as poser:
        for npz, wav in pairs:
            m = motion_file.read(npz)
            if m.gender not in models:
                raise SystemExit(f"beat_align: {npz} names the gender '{m.gender}'; the body models are {', '.join(models)}")
            F = int(m.poses.shape[0])
            if F < 2:
                raise SystemExit(f"beat_align: {npz} holds {F} frames; a speed needs two")
            eng, rot, tr = poser.pose(m)
            J = eng.joints(rot, tr)
            wave = load_wave(wav) if load_wave is not None else load_wave_16k(wav, device)
            wave = torch.as_tensor(wave).reshape(-1).to(device, torch.float32)
            n = int(wave.numel())
            T = plan(n)
            if T > 0:
                _, mask = beat.onsets(wave[None], None, par)
            else:
                mask = torch.zeros(1, 0, dtype=torch.uint8, device=device)
            rows = beat.align_rows(mask, [T], J, None, par)
            one = BeatAlign()
            one.update(rows, *clip_seconds(n, F, fps))
            total.merge(one)
            per_file[str(npz)] = {"wav": str(wav), "samples": n, "frames": F,
                                  **{k: _plain(v) for k, v in one.compute(joints).items() if not k.endswith("_per_joint")}}
    return {"per_file": per_file, "overall": {k: _plain(v) for k, v in total.compute(joints).items()}, "state": total.state(), "params": par}


def write_report(path, per_file: dict, state: dict, params: dict, precision: str, joints: Sequence[int] = DEFAULT_JOINTS) -> Path:
    """<model_path>/viz/beat_align_<stamp>_E<epoch>.json: per file and overall, the parameters and the precision"""
    rep = {"precision": precision, "params": dict(params), "joints": [int(j) for j in joints],
           "note": "this project's own statement of beat alignment; not compared with librosa or with BEAT's code",
           "files": per_file, "overall": {k: _plain(v) for k, v in BeatAlign.from_state(state).compute(joints).items()}}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(rep, indent=1, allow_nan=False))
    return path


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m amuse_amd.beat_align",
                                 description="beat alignment of *_motion_smplx.npz files against their WAVs: NPZ WAV [NPZ WAV ...] (the NPZ names carry no WAV name)")
    ap.add_argument("pairs", nargs="+", help="FILE_motion_smplx.npz FILE.wav, repeated")
    ap.add_argument("--smplx-models", required=True, help="directory holding SMPLX_MALE.npz, SMPLX_FEMALE.npz, SMPLX_NEUTRAL.npz")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="write the JSON here instead of printing it")
    ap.add_argument("--joints", type=int, nargs="+", default=list(DEFAULT_JOINTS), help="SMPL-X joints BA is averaged over (default: shoulders, elbows, wrists)")
    ap.add_argument("--sigma", type=float, default=None, help="width of the time-distance kernel in seconds (default: the library's 0.1)")
    args = ap.parse_args(argv)
    if len(args.pairs) % 2:
        raise SystemExit("beat_align: the files come in pairs: FILE_motion_smplx.npz FILE.wav")
    pairs = [(Path(a), Path(b)) for a, b in zip(args.pairs[0::2], args.pairs[1::2])]
    for a, b in pairs:
        if a.suffix != ".npz" or b.suffix.lower() != ".wav":
            raise SystemExit(f"beat_align: a pair is an .npz then a .wav, got {a} {b}")
        for p in (a, b):
            if not p.is_file():
                raise SystemExit(f"beat_align: {p} is not a file")
    if min(args.joints) < 0 or max(args.joints) >= NJ:
        raise SystemExit(f"beat_align: --joints are indices in 0..{NJ - 1}")
    from . import body
    rep = score_pairs(pairs, body.require_models(args.smplx_models, "beat_align: "), args.device, {"sigma_s": args.sigma} if args.sigma is not None else None, args.joints)
    rep.pop("state")
    rep["note"] = "this project's own statement of beat alignment; not compared with librosa or with BEAT's code"
    for name, v in rep["per_file"].items():
        print(f"[beat_align] {name}: BA {v['BA']}  motion->audio {v['BA_motion_to_audio']}  onsets {v['n_onsets']:.0f}")
    print(f"[beat_align] overall: BA {rep['overall']['BA']}  motion->audio {rep['overall']['BA_motion_to_audio']}")
    text = json.dumps(rep, indent=1, allow_nan=False)
    if args.out:
        Path(args.out).write_text(text)
    else:
        print(text)
    return rep


if __name__ == "__main__":
    main()
