"""Long-form candidates: K samples of every window, the seam-cost matrix between neighbouring windows' candidates, the path of least total cost, and the gather
of its windows (include/amuse_hip.h amuse_seam_plan / amuse_seam_cost / amuse_seam_path / amuse_seam_select; csrc/k_seam.hip).

AN EXTENSION of long-form inference (amuse_amd/longform.py), off by default.  The windows of a long waveform are sampled independently; with K candidates per
window the crossfade blends two motions that were CHOSEN to agree where they meet.  This is the project's own method, compared with no other implementation; its
kernels are checked against a float64 restatement (tests/seam_ref.py).  Nobody has measured whether the candidates of a trained checkpoint differ enough at the
seams for the choice to matter (profiles/seam_cost.txt has random-init weights only).

Batch layout everywhere here: row g * K + c is candidate c of window g; K = 1 is longform.stitch's layout.  Everything runs on the current stream; there is no
CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib

MAX_CANDIDATES = 64
FROZEN_JOINTS = (1, 2, 4, 5, 7, 8, 10, 11)      # the joints the NPZ writer freezes


def default_weights(overlap: int) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """(row_weight (overlap,), joint_weight (55,), trans_weight) of the product, CPU tensors: every overlap row 1; every joint 1, except 0 for the eight joints
    the NPZ writer freezes (1, 2, 4, 5, 7, 8, 10, 11); translation 0 (the writer zeroes it).  A CHOICE - what the written file shows is what is scored - not a
    measurement."""
    jw = torch.ones(55, dtype=torch.float32)
    jw[list(FROZEN_JOINTS)] = 0.0
    return torch.ones(max(int(overlap), 0), dtype=torch.float32), jw, 0.0


def plan(windows: Sequence[int], K: int, hop: int, F: int = 300) -> dict:
    """amuse_seam_plan: {"seams": sum (W_s - 1), "workspace_bytes": ...}.  No GPU needed."""
    S = len(windows)
    seams, ws = C.c_longlong(0), C.c_size_t(0)
    _lib.check(_lib.load().amuse_seam_plan(S, (C.c_int * max(S, 1))(*[int(w) for w in windows]), int(K), int(F), int(hop), C.byref(seams), C.byref(ws)))
    return {"seams": seams.value, "workspace_bytes": ws.value}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _ints(v):
    return (C.c_int * len(v))(*v)


def _need_gpu(t, what):
    if not t.is_cuda:
        raise _lib.AmuseHipError(f"seam.{what} runs on the GPU: amuse_amd has no CPU fallback")


def cost(poses: torch.Tensor, trans: Optional[torch.Tensor], windows: Sequence[int], frames: Sequence[int], K: int, hop: int, F: int = 300,
         row_weight: Optional[torch.Tensor] = None, joint_weight: Optional[torch.Tensor] = None, trans_weight: Optional[float] = None,
         workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """amuse_seam_cost on device tensors.  poses (sum W_s * K, F, 55, 3), trans (sum W_s * K, F, 3) or None -> cost (seams, K, K) float64.  Weights default to
    default_weights(F - hop); they must be finite and >= 0 (not checked on the device).  workspace: a uint8 tensor of plan(...)["workspace_bytes"] bytes and
    `out`: the (seams, K, K) float64 result, for a caller that keeps both (a captured graph); allocated here otherwise."""
    _need_gpu(poses, "cost")
    windows, frames, K, hop, F = [int(w) for w in windows], [int(l) for l in frames], int(K), int(hop), int(F)
    if len(windows) != len(frames) or not windows:
        raise ValueError(f"windows ({len(windows)}) and frames ({len(frames)}) must name the same, non-zero number of sequences")
    dev = poses.device
    poses = poses.to(torch.float32).contiguous()
    if tuple(poses.shape) != (sum(windows) * K, F, 55, 3):
        raise ValueError(f"poses must be ({sum(windows) * K}, {F}, 55, 3), got {tuple(poses.shape)}")
    if trans is not None:
        trans = trans.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(trans.shape) != (sum(windows) * K, F, 3):
            raise ValueError(f"trans must be ({sum(windows) * K}, {F}, 3), got {tuple(trans.shape)}")
    O = max(F - hop, 0)
    d_row, d_joint, d_tw = default_weights(O)
    row_weight = torch.as_tensor(d_row if row_weight is None else row_weight).to(device=dev, dtype=torch.float32).contiguous()
    joint_weight = torch.as_tensor(d_joint if joint_weight is None else joint_weight).to(device=dev, dtype=torch.float32).contiguous()
    trans_weight = float(d_tw if trans_weight is None else trans_weight)
    if row_weight.numel() != O or joint_weight.numel() != 55:
        raise ValueError(f"row_weight must hold F - hop = {O} weights and joint_weight 55, got {row_weight.numel()} and {joint_weight.numel()}")
    p = plan(windows, K, hop, F)
    if workspace is None:
        workspace = torch.empty(p["workspace_bytes"], device=dev, dtype=torch.uint8)
    if workspace.device != dev or workspace.numel() * workspace.element_size() < p["workspace_bytes"]:
        raise ValueError(f"workspace must hold {p['workspace_bytes']} bytes on {dev}")
    if out is None:
        out = torch.empty(p["seams"], K, K, device=dev, dtype=torch.float64)
    if out.device != dev or out.dtype != torch.float64 or tuple(out.shape) != (p["seams"], K, K) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 ({p['seams']}, {K}, {K}) tensor on {dev}")
    S = len(windows)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_seam_cost(_ptr(poses), _ptr(trans), S, _ints(windows), _ints(frames), K, F, hop, _ptr(row_weight), _ptr(joint_weight),
                                               trans_weight, _ptr(workspace), _ptr(out), torch.cuda.current_stream(dev).cuda_stream))
    return out


def path(cost_matrix: torch.Tensor, windows: Sequence[int], K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """amuse_seam_path: cost (seams, K, K) float64 -> (choice (sum W_s,) int32: the chosen batch row g * K + c of every window, total (S,) float64)."""
    _need_gpu(cost_matrix, "path")
    windows, K = [int(w) for w in windows], int(K)
    if not windows:
        raise ValueError("windows must name at least one sequence")
    dev = cost_matrix.device
    seams = sum(w - 1 for w in windows)
    if cost_matrix.dtype != torch.float64 or tuple(cost_matrix.shape) != (seams, K, K):
        raise ValueError(f"cost must be float64 ({seams}, {K}, {K}), got {cost_matrix.dtype} {tuple(cost_matrix.shape)}")
    cost_matrix = cost_matrix.contiguous()
    choice = torch.empty(sum(windows), device=dev, dtype=torch.int32)
    total = torch.empty(len(windows), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_seam_path(_ptr(cost_matrix), len(windows), _ints(windows), K, _ptr(choice), _ptr(total),
                                               torch.cuda.current_stream(dev).cuda_stream))
    return choice, total


def select(poses: torch.Tensor, trans: Optional[torch.Tensor], choice: torch.Tensor, poses_out: Optional[torch.Tensor] = None,
           trans_out: Optional[torch.Tensor] = None):
    """amuse_seam_select: the rows `choice` (n,) int32 names, bit for bit -> (poses (n, F, 55, 3), trans (n, F, 3) or None).  Outputs given by the caller must
    not overlap the inputs (refused by the library)."""
    _need_gpu(poses, "select")
    dev = poses.device
    poses = poses.to(torch.float32).contiguous()
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (55, 3):
        raise ValueError(f"poses must be (rows, F, 55, 3), got {tuple(poses.shape)}")
    n_in, F = int(poses.shape[0]), int(poses.shape[1])
    if trans is not None:
        trans = trans.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(trans.shape) != (n_in, F, 3):
            raise ValueError(f"trans must be ({n_in}, {F}, 3), got {tuple(trans.shape)}")
    choice = choice.to(device=dev, dtype=torch.int32).contiguous()
    n = int(choice.numel())
    if poses_out is None:
        poses_out = torch.empty(n, F, 55, 3, device=dev, dtype=torch.float32)
    if trans is not None and trans_out is None:
        trans_out = torch.empty(n, F, 3, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_seam_select(_ptr(poses), _ptr(trans), _ptr(choice), n, n_in, F, _ptr(poses_out), _ptr(trans_out),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return poses_out, trans_out


def best_windows(poses: torch.Tensor, trans: Optional[torch.Tensor], windows: Sequence[int], frames: Sequence[int], K: int, hop: int, F: int = 300,
                 row_weight=None, joint_weight=None, trans_weight=None):
    """cost -> path -> select: the (sum W_s * K) candidate rows become the (sum W_s) rows longform.stitch reads.  -> (poses, trans, info) with info = {"choice":
    (sum W_s,) int32 batch rows, "total": (S,) float64 cost of the chosen path, "total_first": (S,) float64 cost of the all-candidate-0 path - what K = 1 would
    have joined - summed from the same matrix in seam order, "cost": the matrix}, all on the device: nothing here synchronises."""
    windows, K = [int(w) for w in windows], int(K)
    m = cost(poses, trans, windows, frames, K, hop, F, row_weight, joint_weight, trans_weight)
    choice, total = path(m, windows, K)
    po, to = select(poses, trans, choice)
    # the all-first-candidates path: the same kernel on the [0][0] entries as a K = 1 matrix, so it is summed in the order every path is summed in (a path
    # through a non-finite entry totals +infinity there, as it would here)
    _, first = path(m[:, :1, :1].contiguous(), windows, 1)
    return po, to, {"choice": choice, "total": total, "total_first": first, "cost": m}


def report(info: dict, windows: Sequence[int], K: int) -> list:
    """The small host report of best_windows' info, per sequence: [{"choice": [candidate per window], "total": x, "total_first": y}, ...].  This is the one place
    that reads the device (one synchronisation)."""
    choice = info["choice"].cpu().tolist()
    total, first = info["total"].cpu().tolist(), info["total_first"].cpu().tolist()
    out, g = [], 0
    for s, W in enumerate(windows):
        out.append({"choice": [int(r) % int(K) for r in choice[g:g + W]], "total": float(total[s]), "total_first": float(first[s])})
        g += W
    return out
