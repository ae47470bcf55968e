"""*_motion_smplx.npz on disk: the one reader, the one naming rule for a file beside it and the one atomic writer of every module that touches these files
(npz_writer.py states what goes into one; this module is how one is opened, named and replaced)."""
from __future__ import annotations

import os
from collections import namedtuple
from contextlib import contextmanager
from pathlib import Path

import numpy as np

Motion = namedtuple("Motion", "poses trans gender betas fps path")


def read(path) -> Motion:
    """-> Motion(poses float32 [F, 55, 3], trans float32 [F, 3], gender str, betas float64 1-D as the file stores them, fps float, path).  Only `poses` must be
    there: no trans -> zeros, no gender -> "neutral", no betas -> zeros(300), no mocap_frame_rate -> 30.  Anything but F >= 1 frames of 55 joints is refused;
    what a consumer cannot use (a gender without a model, too few frames for a speed) is that consumer's refusal."""
    path = Path(path)
    with np.load(path, allow_pickle=False) as z:
        poses = np.asarray(z["poses"], dtype=np.float32)
        F = poses.shape[0]
        if F < 1 or poses[0].size != 165:
            raise ValueError(f"{path}: poses hold {F} frames of {poses[0].size // 3 if F else 0} joints, not SMPL-X's 55")
        return Motion(poses.reshape(F, 55, 3),
                      np.asarray(z["trans"], dtype=np.float32).reshape(F, 3) if "trans" in z.files else np.zeros((F, 3), np.float32),
                      str(z["gender"]) if "gender" in z.files else "neutral",
                      np.asarray(z["betas"], dtype=np.float64).reshape(-1) if "betas" in z.files else np.zeros(300),
                      float(z["mocap_frame_rate"]) if "mocap_frame_rate" in z.files else 30.0, path)


def sibling(path, suffix: str, out_dir=None, strip: str = "_motion_smplx.npz") -> Path:
    """<name><strip> -> <name><suffix> (a name that does not end with `strip` gives its stem), beside the file or in out_dir"""
    p = Path(path)
    stem = p.name[:-len(strip)] if p.name.endswith(strip) else p.stem
    return (Path(out_dir) if out_dir is not None else p.parent) / (stem + suffix)


@contextmanager
def atomic(path):
    """A binary file that becomes `path` (its directory made) when the block ends without an exception.  It is written beside the target and moved over it: a
    reader that still holds an older file of the same name open (two runs inside one second share the time-stamped directory and the seeded tags) keeps
    reading that file, never a half-written or replaced one."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(path.name + ".part")
    with open(tmp, "wb") as fh:
        yield fh
    os.replace(tmp, path)


def save(path, **fields) -> Path:
    with atomic(path) as fh:
        np.savez(fh, **fields)
    return Path(path)
