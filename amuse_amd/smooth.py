"""Motion smoothing: a Savitzky-Golay filter over time, on SO(3) for the 55 joints and on R^3 for the translation (include/amuse_hip.h amuse_smooth_banks /
amuse_smooth_motion; csrc/k_smooth.hip).

AN EXTENSION, off by default - the reference writes the decoder's rows as they come.  Every joint is fitted in the tangent space at the frame being filtered
(the relative rotations to the frame's own quaternion, their logarithms weighted by the bank row, the exponential back), not on Euler angles or raw rotation
vectors.  It is this project's own statement of the method, in the manner of "geometric Savitzky-Golay filtering" on SO(3), written down from memory: pinned
against no other implementation, except the Euclidean half (the bank, the translation) against scipy.signal.  The default of a 9-frame window at order 3
(30 fps) is a recollection of common practice, not a measurement.

The bank is the library's (`banks` calls it; nothing here restates its arithmetic), the filter is a HIP kernel (`smooth`); there is no other implementation.

    python -m amuse_amd.smooth FILE_motion_smplx.npz [more ...] [-o DIR] [--window 9] [--order 3] [--hands-window N]

smooths the NPZ of any earlier run (the reference's own included) into *_smoothed_motion_smplx.npz; it needs no checkpoint."""
from __future__ import annotations

import argparse
import ctypes as C
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, motion_file

MAX_HALF, MAX_ORDER, BANK_FLOATS, SLOTS = 15, 5, 5455, 56
HAND_JOINTS = range(25, 55)      # the SMPL-X fingers: 15 joints of the left hand, 15 of the right
DEFAULT_WINDOW, DEFAULT_ORDER = 9, 3

_banks_dev: Dict[tuple, torch.Tensor] = {}


def bank_offset(m: int) -> int:
    """H_m's first float in the bank (include/amuse_hip.h): 9 + 25 + ... + (2 m - 1)^2."""
    n = int(m) - 1
    return n * (4 * n * n + 12 * n + 11) // 3


def banks(order: int = DEFAULT_ORDER) -> np.ndarray:
    """amuse_smooth_banks: the fp32 hat matrices H_1 .. H_15 back to back, (5455,).  No GPU needed.  An order outside 0..5 raises AmuseHipError."""
    out = np.empty(BANK_FLOATS, dtype=np.float32)
    _lib.check(_lib.load().amuse_smooth_banks(int(order), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def check_window(window: int, what: str = "window") -> int:
    window = int(window)
    if window % 2 != 1 or not 3 <= window <= 2 * MAX_HALF + 1:
        raise ValueError(f"{what} {window}: an odd number of frames in 3..{2 * MAX_HALF + 1}")
    return window


def check_order(order: int) -> int:
    order = int(order)
    if not 0 <= order <= MAX_ORDER:
        raise ValueError(f"order {order}: 0..{MAX_ORDER}")
    return order


def half_windows(window: int = DEFAULT_WINDOW, hands_window: Optional[int] = None) -> List[int]:
    """The 56 half-windows of a run: (window - 1) / 2 for the joints and the translation, (hands_window - 1) / 2 for joints 25..54, the SMPL-X fingers, when
    hands_window is given.  Windows are odd, 3..31."""
    m = (check_window(window) - 1) // 2
    hw = [m] * SLOTS
    if hands_window is not None:
        mh = (check_window(hands_window, "hands_window") - 1) // 2
        for j in HAND_JOINTS:
            hw[j] = mh
    return hw


def _banks_on(dev: torch.device, order: int) -> torch.Tensor:
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), int(order))
    if key not in _banks_dev:
        _banks_dev[key] = torch.from_numpy(banks(order)).to(dev)
    return _banks_dev[key]


def smooth(poses: torch.Tensor, trans: Optional[torch.Tensor], frames: Sequence[int], window: int = DEFAULT_WINDOW, order: int = DEFAULT_ORDER,
           hands_window: Optional[int] = None, half_window: Optional[Sequence[int]] = None):
    """amuse_smooth_motion on device tensors.  poses (sum L_s, 55, 3) axis-angle and trans (sum L_s, 3) or None - S sequences back to back, as longform.stitch
    returns them; frames: L_s per sequence.  -> (poses, trans or None) of the same shapes, new tensors.  half_window: the 56 values themselves (0..15), instead
    of window / hands_window.  A slot whose window does not fit its sequence (L_s < window) keeps its input bits.  Runs on the current stream; allocates its
    outputs only (and, once per (device, order), the bank)."""
    if not poses.is_cuda:
        raise _lib.AmuseHipError("smooth.smooth runs on the GPU: amuse_amd has no CPU fallback")
    frames = [int(l) for l in frames]
    if not frames:
        raise ValueError("frames must name at least one sequence")
    hw = [int(m) for m in half_window] if half_window is not None else half_windows(window, hands_window)
    if len(hw) != SLOTS or not all(0 <= m <= MAX_HALF for m in hw):
        raise ValueError(f"half_window must hold {SLOTS} values in 0..{MAX_HALF}")
    order = check_order(order)
    dev = poses.device
    poses = poses.to(torch.float32).contiguous()
    total = sum(frames)
    if tuple(poses.shape) != (total, 55, 3):
        raise ValueError(f"poses must be ({total}, 55, 3), got {tuple(poses.shape)}")
    if trans is not None:
        trans = trans.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(trans.shape) != (total, 3):
            raise ValueError(f"trans must be ({total}, 3), got {tuple(trans.shape)}")
    bk = _banks_on(dev, order)
    poses_out = torch.empty_like(poses)
    trans_out = torch.empty_like(trans) if trans is not None else None
    S = len(frames)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_smooth_motion(ptr(poses), ptr(trans), S, (C.c_int * S)(*frames), (C.c_ubyte * SLOTS)(*hw), ptr(bk), ptr(poses_out),
                                                   ptr(trans_out), torch.cuda.current_stream(dev).cuda_stream))
    return poses_out, trans_out


def options(window: Optional[int] = None, order: Optional[int] = None, hands_window: Optional[int] = None) -> dict:
    """The checked per-run options as trainer.run_jobs / PretrainedLPDM_v1.infer_long take them (`smooth=`) and TRAIN_PARAM.test.smooth stores them; None: the default."""
    o = {"window": check_window(DEFAULT_WINDOW if window is None else window), "order": check_order(DEFAULT_ORDER if order is None else order)}
    if hands_window is not None:
        o["hands_window"] = check_window(hands_window, "hands_window")
    return o


def smooth_batch(poses: torch.Tensor, trans: Optional[torch.Tensor], opts: dict):
    """poses (B, L, 55, 3), trans (B, L, 3) or None - B motions of L frames, as diffusion_backward and the long-form join hand them on - each filtered as a
    sequence of its own; the same shapes back."""
    B, L = int(poses.shape[0]), int(poses.shape[1])
    p, t = smooth(poses.reshape(B * L, 55, 3), None if trans is None else trans.reshape(B * L, 3), [L] * B, **options(**opts))
    return p.reshape(B, L, 55, 3), None if t is None else t.reshape(B, L, 3)


# ------------------------------------------------------------------ python -m amuse_amd.smooth
def output_path(src: Path, out_dir: Optional[Path] = None) -> Path:
    return motion_file.sibling(src, "_smoothed_motion_smplx.npz", out_dir)


def smooth_npz(src, out_dir=None, window: int = DEFAULT_WINDOW, order: int = DEFAULT_ORDER, hands_window: Optional[int] = None, device="cuda") -> Path:
    """One *_motion_smplx.npz -> *_smoothed_motion_smplx.npz, written through npz_writer.smplx_npz_fields: the lower-body lock and the zero `trans` hold as in
    every NPZ of this project; betas, gender and frame rate are carried over."""
    from .npz_writer import smplx_npz_fields
    m = motion_file.read(src)
    F = m.poses.shape[0]
    out, _ = smooth(torch.from_numpy(m.poses).to(device), None, [F], window, order, hands_window)
    return motion_file.save(output_path(m.path, out_dir), **smplx_npz_fields(out.cpu().numpy().reshape(F, 165), m.gender, m.betas, m.fps))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m amuse_amd.smooth", description="Savitzky-Golay smoothing on SO(3) of *_motion_smplx.npz files, in HIP")
    ap.add_argument("files", nargs="+", help="*_motion_smplx.npz of any earlier run")
    ap.add_argument("-o", "--out-dir", default=None, help="where the *_smoothed_motion_smplx.npz go (default: beside each input)")
    ap.add_argument("--window", type=int, default=DEFAULT_WINDOW, help="frames per window, odd, 3..31 (default 9: a recollection of common practice at 30 fps)")
    ap.add_argument("--order", type=int, default=DEFAULT_ORDER, help="polynomial order 0..5 (default 3)")
    ap.add_argument("--hands-window", type=int, default=None, help="another window for the 30 finger joints (default: --window)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    try:
        options(args.window, args.order, args.hands_window)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None) -> List[Path]:
    args = parse_args(argv)
    written = [smooth_npz(f, args.out_dir, args.window, args.order, args.hands_window, args.device) for f in args.files]
    for p in written:
        print(f"[amuse_amd] smoothed: {p}")
    return written


if __name__ == "__main__":
    main()
