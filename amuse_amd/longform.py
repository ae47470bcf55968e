"""Long-form inference: a waveform of any length as overlapping windows of the model's 10 s clip, joined by a rotation crossfade (include/amuse_hip.h
amuse_longform_plan / amuse_stitch_windows; csrc/k_stitch.hip).

AN EXTENSION - the reference has no such path: it asks for pre-cut audio ("Make sure each audio is a 10 sec wav file", scripts/trainer.py:506).  The windows are
sampled INDEPENDENTLY (the Denoiser's state is one latent per clip; nothing is shared between windows inside the sampler); the crossfade over the frames two
neighbouring windows both produced hides the seam, it does not make the windows agree.  (amuse_amd/seam.py - `--long-form-candidates K`, infer_long(candidates=K) -
samples K candidates of every window and joins the ones that agree best where they meet; for K = 1 the sentence stands.)

The plan is the library's (`plan` calls it; nothing here restates its arithmetic), the join is a HIP kernel (`stitch`); there is no other implementation."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

CLIP_FRAMES, CLIP_SAMPLES, DEFAULT_HOP = 300, 160000, 270


def plan(n_samples: int, hop: int = DEFAULT_HOP) -> dict:
    """amuse_longform_plan: {"windows": W, "frames": L, "hop_samples": hs} for a waveform of n_samples samples (16 kHz) at a stride of `hop` frames (a multiple
    of 3 in 150..300) between window starts.  No GPU needed.  A bad hop or a negative n raises AmuseHipError."""
    out = [C.c_int(0) for _ in range(3)]
    _lib.check(_lib.load().amuse_longform_plan(int(n_samples), int(hop), *(C.byref(o) for o in out)))
    return {"windows": out[0].value, "frames": out[1].value, "hop_samples": out[2].value}


def window_slices(n_samples: int, hop: int = DEFAULT_HOP) -> List[Tuple[int, int]]:
    """[(start, stop), ...]: the samples window w reads, [w hs, min(w hs + 160000, n)).  The last one may be short (the front-end pads it)."""
    p = plan(n_samples, hop)
    return [(w * p["hop_samples"], min(w * p["hop_samples"] + CLIP_SAMPLES, int(n_samples))) for w in range(p["windows"])]


def blend_weights(overlap: int) -> torch.Tensor:
    """The product's crossfade: w_i = 0.5 - 0.5 cos(pi (i + 1) / (O + 1)), i = 0..O-1 - the later window's weight, strictly inside (0, 1), symmetric about the
    overlap's middle.  Computed in double, rounded to fp32 (a CPU tensor: the kernel and any restatement then see the same numbers)."""
    i = np.arange(int(overlap), dtype=np.float64)
    return torch.from_numpy((0.5 - 0.5 * np.cos(np.pi * (i + 1.0) / (int(overlap) + 1.0))).astype(np.float32))


def stitch(poses: torch.Tensor, trans: Optional[torch.Tensor], windows: Sequence[int], frames: Sequence[int], hop: int, F: int = CLIP_FRAMES,
           blend: Optional[torch.Tensor] = None):
    """amuse_stitch_windows on device tensors.  poses (sum W_s, F, 55, 3) axis-angle and trans (sum W_s, F, 3) or None - the windows of S sequences back to back,
    as diffusion_backward returns them; windows / frames: W_s and L_s per sequence.  -> (poses (sum L_s, 55, 3), trans (sum L_s, 3) or None), the sequences back
    to back.  blend: (F - hop,) weights of the later window (default blend_weights(F - hop)).  Runs on the current stream; allocates its outputs only."""
    if not poses.is_cuda:
        raise _lib.AmuseHipError("longform.stitch runs on the GPU: amuse_amd has no CPU fallback")
    windows, frames = [int(w) for w in windows], [int(l) for l in frames]
    if len(windows) != len(frames) or not windows:
        raise ValueError(f"windows ({len(windows)}) and frames ({len(frames)}) must name the same, non-zero number of sequences")
    dev = poses.device
    poses = poses.to(torch.float32).contiguous()
    if tuple(poses.shape) != (sum(windows), int(F), 55, 3):
        raise ValueError(f"poses must be ({sum(windows)}, {F}, 55, 3), got {tuple(poses.shape)}")
    if trans is not None:
        trans = trans.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(trans.shape) != (sum(windows), int(F), 3):
            raise ValueError(f"trans must be ({sum(windows)}, {F}, 3), got {tuple(trans.shape)}")
    if blend is None:
        blend = blend_weights(max(int(F) - int(hop), 0))
    blend = torch.as_tensor(blend).to(device=dev, dtype=torch.float32).contiguous()
    if blend.numel() != max(int(F) - int(hop), 0):
        raise ValueError(f"blend must hold F - hop = {int(F) - int(hop)} weights, got {blend.numel()}")
    total = max(sum(frames), 0)
    poses_out = torch.empty(total, 55, 3, device=dev, dtype=torch.float32)
    trans_out = torch.empty(total, 3, device=dev, dtype=torch.float32) if trans is not None else None
    S = len(windows)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_stitch_windows(ptr(poses), ptr(trans), S, (C.c_int * S)(*windows), (C.c_int * S)(*frames), int(F), int(hop), ptr(blend),
                                                    ptr(poses_out), ptr(trans_out), torch.cuda.current_stream(dev).cuda_stream))
    return poses_out, trans_out
