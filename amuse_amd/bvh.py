"""BVH export: the SMPL-X motions this project writes (*_motion_smplx.npz) as Biovision BVH - a text format Maya, MotionBuilder, Unreal, Blender without
add-ons and the GENEA / BEAT toolchains read (include/amuse_hip.h amuse_bvh_layout / amuse_bvh_format / amuse_bvh_motion / amuse_bvh_decode; csrc/k_bvh.hip).

AN EXTENSION, off by default - the reference retargets its NPZ output to BVH through Blender; this writes the SMPL-X skeleton itself: 55 joints named as the
public `smplx` package names them, offsets from the rest joints of the file's gender and betas, Euler channels in degrees.  Retargeting to another skeleton
stays out of scope.

The hierarchy is written on the host (standard library and numpy).  The MOTION block - axis-angle to Euler channels, robust at gimbal lock, and every number as
the text of C's "%11.6f" - is written by HIP kernels; there is no other implementation.  The column order is the library's (`layout`; nothing here restates it).

Metadata.  BVH has no comment syntax: its grammar starts with the keyword HIERARCHY, and importers that check the first token (Blender's does) refuse a file
that starts with anything else.  Gender, betas, scale, the root's rest position and the frame rate therefore travel in a side file, *_motion.bvh.json, which
`--to-npz` reads when it is there (without it: neutral gender, zero betas, scale 100, rest position zero).

No BVH importer is run anywhere in this project: the files are held to the format's grammar through `read_bvh`, their numbers to scipy (tests/test_gpu_bvh.py).
The default unit, centimetres (scale 100), is a recollection of what most BVH consumers expect, not a measurement.

    python -m amuse_amd.bvh FILE_motion_smplx.npz [more ...] --smplx-models DIR [-o DIR] [--order ZYX] [--scale 100] [--unwrap]
    python -m amuse_amd.bvh --to-npz FILE_motion.bvh [more ...] [-o DIR]

The first converts the NPZ of any earlier run (the reference's own included) and needs no checkpoint; the second goes back, for files of this skeleton, and
writes *_from_bvh_motion_smplx.npz."""
from __future__ import annotations

import argparse
import ctypes as C
import json
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib, motion_file

NJ, COLS, FIELD = 55, 168, 12
ROW_BYTES = COLS * FIELD
ORDERS = ("XYZ", "XZY", "YXZ", "YZX", "ZXY", "ZYX")          # AMUSE_BVH_XYZ .. AMUSE_BVH_ZYX: channel list "A B C" means R = R_A R_B R_C (scipy's intrinsic 'ABC')
DEFAULT_ORDER, DEFAULT_SCALE = "ZYX", 100.0                  # ZYX: the order of the reference's SMPLX_TPOSE_FLAT.bvh; 100: centimetres
MAX_ROWS_PER_CALL = 400_000                                  # 0.8 GB of text per call; a sequence's bytes do not depend on the call it falls in
_FINGERS = ("index", "middle", "pinky", "ring", "thumb")
JOINT_NAMES = (["pelvis", "left_hip", "right_hip", "spine1", "left_knee", "right_knee", "spine2", "left_ankle", "right_ankle", "spine3", "left_foot", "right_foot",
                "neck", "left_collar", "right_collar", "head", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow", "left_wrist", "right_wrist", "jaw",
                "left_eye_smplhf", "right_eye_smplhf"]
               + [f"{side}_{f}{k}" for side in ("left", "right") for f in _FINGERS for k in (1, 2, 3)])
assert len(JOINT_NAMES) == NJ == len(set(JOINT_NAMES))


class BvhRangeError(ValueError):
    """a value of the motion does not fit the 11-character field"""


def _order_index(order: str) -> int:
    o = str(order).upper()
    if o not in ORDERS:
        raise ValueError(f"order {order!r}: one of {', '.join(ORDERS)}")
    return ORDERS.index(o)


def options(order: Optional[str] = None, scale: Optional[float] = None, unwrap: bool = False) -> dict:
    """The checked per-run options; None: the default."""
    order, scale = DEFAULT_ORDER if order is None else order, float(DEFAULT_SCALE if scale is None else scale)
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"scale {scale}: positive and finite")
    return {"order": ORDERS[_order_index(order)], "scale": scale, "unwrap": bool(unwrap)}


def layout(parents) -> np.ndarray:
    """amuse_bvh_layout: the joint of every MOTION column triple - the depth-first order of `parents`, children in ascending index.  No GPU needed."""
    p = np.ascontiguousarray(np.asarray(parents), dtype=np.int32)
    out = np.empty(max(p.size, 1), dtype=np.int32)
    ip = C.POINTER(C.c_int)
    _lib.check(_lib.load().amuse_bvh_layout(p.ctypes.data_as(ip), int(p.size), out.ctypes.data_as(ip)))
    return out[:p.size]


def rest_joints(model, betas=None) -> np.ndarray:
    """(55, 3) float64: the joints at the zero pose and zero translation for `betas` - the first two lines of body.torch_forward (J = J_regressor (v_template +
    shapedirs betas)), which is all the zero pose leaves of it."""
    b = np.zeros(model.n_betas) if betas is None else np.asarray(betas, dtype=np.float64).reshape(-1)
    n = min(b.size, model.n_betas)
    vs = model.v_template.astype(np.float64) + model.shapedirs[:, :, :n].astype(np.float64) @ b[:n]
    return model.J_regressor.astype(np.float64) @ vs


# ------------------------------------------------------------------ the header (host)
def header_text(parents, J_rest, frames: int, fps: float = 30.0, order: str = DEFAULT_ORDER, scale: float = DEFAULT_SCALE, names: Sequence[str] = JOINT_NAMES) -> str:
    """HIERARCHY .. "Frame Time:" - everything in front of the MOTION rows.  The root has OFFSET 0 0 0 and carries its full position in its channels (the same
    motion whether a reader adds the root's channels to its OFFSET or replaces it); every other joint has OFFSET (J_rest[j] - J_rest[parent]) x scale; every leaf
    an End Site at half its own offset."""
    parents = np.asarray(parents).astype(np.int64)
    J = np.asarray(J_rest, dtype=np.float64)
    order = ORDERS[_order_index(order)]
    rot = " ".join(f"{c}rotation" for c in order)
    kids: Dict[int, List[int]] = {j: [] for j in range(len(parents))}
    for j in range(1, len(parents)):
        kids[int(parents[j])].append(j)
    out = ["HIERARCHY"]
    f6 = lambda v: " ".join("%.6f" % x for x in v)

    def emit(j: int, depth: int):
        t = "\t" * depth
        off = np.zeros(3) if j == 0 else (J[j] - J[parents[j]]) * scale
        out.append(f"{t}{'ROOT' if j == 0 else 'JOINT'} {names[j]}")
        out.append(t + "{")
        out.append(f"{t}\tOFFSET {f6(off)}")
        out.append(f"{t}\tCHANNELS 6 Xposition Yposition Zposition {rot}" if j == 0 else f"{t}\tCHANNELS 3 {rot}")
        for k in kids[j]:
            emit(k, depth + 1)
        if not kids[j]:
            out.extend([f"{t}\tEnd Site", t + "\t{", f"{t}\t\tOFFSET {f6(off * 0.5)}", t + "\t}"])
        out.append(t + "}")

    emit(0, 0)
    out.extend(["MOTION", f"Frames: {int(frames)}", "Frame Time: %.6f" % (1.0 / float(fps))])
    return "\n".join(out) + "\n"


def sidecar_path(bvh_path) -> Path:
    p = Path(bvh_path)
    return p.with_name(p.name + ".json")


def write_bvh(path, header: str, block: bytes, meta: Optional[dict] = None) -> Path:
    """header ++ block -> path, atomically, as every motion file is written; meta -> path + ".json" the same way."""
    path = Path(path)
    for dst, data in ((path, header.encode("ascii") + bytes(block)),) + (((sidecar_path(path), json.dumps(meta).encode("ascii")),) if meta is not None else ()):
        with motion_file.atomic(dst) as fh:
            fh.write(data)
    return path


# ------------------------------------------------------------------ the reader (host)
def read_bvh(path) -> dict:
    """A BVH file of THIS skeleton, by the format's grammar: a small tokenizer on the hierarchy, numpy on the MOTION block.  -> names (file order), parents and
    offsets (SMPL-X index order), end_sites {joint: offset}, dfs (the joint of each column triple), order, frames, frame_time, channels (F, 168) float64, and
    meta (the side file's dictionary, or None).  Refused: joints other than the 55 names, once each; a root without 6 channels (positions first) or a joint without
    3; channel orders that differ between joints; a MOTION block that does not hold Frames x 168 numbers."""
    path = Path(path)
    text = path.read_text("ascii")
    cut = text.find("MOTION")
    if not text.lstrip().startswith("HIERARCHY") or cut < 0:
        raise ValueError(f"{path}: not a BVH file (HIERARCHY .. MOTION)")
    tok = text[:cut].split()
    pos = 1
    idx = {n: j for j, n in enumerate(JOINT_NAMES)}
    names: List[str] = []
    parents = np.full(NJ, -2, dtype=np.int32)
    offsets = np.zeros((NJ, 3))
    end_sites: Dict[int, np.ndarray] = {}
    orders: List[str] = []

    def need(word):
        nonlocal pos
        if pos >= len(tok) or tok[pos] != word:
            raise ValueError(f"{path}: expected {word!r} at token {pos}, found {tok[pos] if pos < len(tok) else 'the end'!r}")
        pos += 1

    def joint(parent: int):
        nonlocal pos
        kind, name = tok[pos], tok[pos + 1]
        if kind != ("ROOT" if parent < 0 else "JOINT"):
            raise ValueError(f"{path}: expected {'ROOT' if parent < 0 else 'JOINT'}, found {kind!r}")
        if name not in idx or parents[idx[name]] != -2:
            raise ValueError(f"{path}: joint {name!r} is not one of the 55 SMPL-X joints, or is there twice: only files of this skeleton are read")
        j = idx[name]
        names.append(name)
        parents[j] = parent
        pos += 2
        need("{")
        need("OFFSET")
        offsets[j] = [float(x) for x in tok[pos:pos + 3]]
        pos += 3
        need("CHANNELS")
        n = int(tok[pos])
        ch = tok[pos + 1:pos + 1 + n]
        pos += 1 + n
        if n != (6 if parent < 0 else 3) or (parent < 0 and ch[:3] != ["Xposition", "Yposition", "Zposition"]):
            raise ValueError(f"{path}: joint {name!r} has channels {ch}: the root carries Xposition Yposition Zposition and three rotations, every other joint three rotations")
        rot = ch[-3:]
        if any(not c.endswith("rotation") for c in rot):
            raise ValueError(f"{path}: joint {name!r} has channels {ch}")
        orders.append("".join(c[0] for c in rot))
        while tok[pos] == "JOINT":
            joint(j)
        if tok[pos] == "End":
            need("End"); need("Site"); need("{"); need("OFFSET")
            end_sites[j] = np.array([float(x) for x in tok[pos:pos + 3]])
            pos += 3
            need("}")
        need("}")

    try:
        joint(-1)
    except IndexError:
        raise ValueError(f"{path}: the hierarchy ends inside a joint") from None
    if pos != len(tok) or len(names) != NJ:
        raise ValueError(f"{path}: {len(names)} joints, {len(tok) - pos} tokens behind the root: only files of this skeleton's 55 joints are read")
    if len(set(orders)) != 1 or orders[0] not in ORDERS:
        raise ValueError(f"{path}: channel orders {sorted(set(orders))}: one Tait-Bryan order for all joints")
    body = text[cut:].split("\n", 3)
    if len(body) < 4 or not body[1].startswith("Frames:") or not body[2].startswith("Frame Time:"):
        raise ValueError(f"{path}: MOTION is not followed by 'Frames:' and 'Frame Time:' lines")
    frames, frame_time = int(body[1].split(":")[1]), float(body[2].split(":")[1])
    values = np.array(body[3].split(), dtype=np.float64)
    if frames < 1 or values.size != frames * COLS:
        raise ValueError(f"{path}: {values.size} numbers in the MOTION block, Frames: {frames} x {COLS} expected")
    side = sidecar_path(path)
    meta = json.loads(side.read_text("ascii")) if side.exists() else None
    return {"names": names, "parents": parents, "offsets": offsets, "end_sites": end_sites, "dfs": np.array([idx[n] for n in names], dtype=np.int32),
            "order": orders[0], "frames": frames, "frame_time": frame_time, "channels": values.reshape(frames, COLS), "meta": meta}


# ------------------------------------------------------------------ the kernels
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _need_gpu(t, who):
    if not t.is_cuda:
        raise _lib.AmuseHipError(f"bvh.{who} runs on the GPU: amuse_amd has no CPU fallback")


def format_values(values, per_row: int = COLS):
    """amuse_bvh_format on a device tensor of n fp32 values -> (text (12 n,) uint8 on the device, status (1,) int32): field i is C's "%11.6f" of values[i] and a
    separator, '\\n' after every per_row-th.  A value that does not fit leaves '#' and a non-zero status; nothing raises here."""
    import torch
    _need_gpu(values, "format_values")
    v = values.to(torch.float32).contiguous().reshape(-1)
    text = torch.empty(v.numel() * FIELD, dtype=torch.uint8, device=v.device)
    status = torch.zeros(1, dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        _lib.check(_lib.load().amuse_bvh_format(_ptr(v), int(v.numel()), int(per_row), _ptr(text), _ptr(status), torch.cuda.current_stream(v.device).cuda_stream))
    return text, status


def motion_channels(poses, trans, root_rest, frames: Sequence[int], dfs, order: str = DEFAULT_ORDER, scale: float = DEFAULT_SCALE, unwrap: bool = False,
                    euler: bool = False, text: bool = True):
    """amuse_bvh_motion on device tensors.  poses (sum F_s, 55, 3) axis-angle, trans (sum F_s, 3) or None, root_rest (S, 3): S sequences back to back; frames:
    F_s per sequence; dfs: `layout(parents)`.  -> (euler (rows, 168) fp32 or None, text (rows x 2016,) uint8 or None, status (S,) int32), all on the device;
    status[s] != 0: sequence s holds a value that does not fit the field.  Runs on the current stream; allocates its outputs only."""
    import torch
    _need_gpu(poses, "motion_channels")
    frames = [int(f) for f in frames]
    if not frames:
        raise ValueError("frames must name at least one sequence")
    o = options(order, scale, unwrap)
    dev, S, rows = poses.device, len(frames), sum(frames)
    poses = poses.to(torch.float32).contiguous()
    if tuple(poses.shape) != (rows, NJ, 3):
        raise ValueError(f"poses must be ({rows}, 55, 3), got {tuple(poses.shape)}")
    if trans is not None:
        trans = trans.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(trans.shape) != (rows, 3):
            raise ValueError(f"trans must be ({rows}, 3), got {tuple(trans.shape)}")
    root_rest = torch.as_tensor(root_rest).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(root_rest.shape) != (S, 3):
        raise ValueError(f"root_rest must be ({S}, 3), got {tuple(root_rest.shape)}")
    dfs = [int(j) for j in np.asarray(dfs).reshape(-1)]
    if len(dfs) != NJ:
        raise ValueError(f"dfs must hold {NJ} joints")
    e = torch.empty(rows, COLS, dtype=torch.float32, device=dev) if euler else None
    t = torch.empty(rows * ROW_BYTES, dtype=torch.uint8, device=dev) if text else None
    status = torch.zeros(S, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_bvh_motion(_ptr(poses), _ptr(trans), _ptr(root_rest), S, (C.c_int * S)(*frames), (C.c_int * NJ)(*dfs), _order_index(o["order"]),
                                                C.c_float(o["scale"]), int(o["unwrap"]), _ptr(e), _ptr(t), _ptr(status), torch.cuda.current_stream(dev).cuda_stream))
    return e, t, status


def decode(channels, frames: Sequence[int], dfs, order: str, scale: float, root_rest):
    """amuse_bvh_decode: channels (sum F_s, 168) degrees and positions on the device -> (poses (rows, 55, 3) axis-angle with angle <= pi, trans (rows, 3))."""
    import torch
    _need_gpu(channels, "decode")
    frames = [int(f) for f in frames]
    o = options(order, scale)
    dev, S, rows = channels.device, len(frames), sum(frames)
    ch = channels.to(torch.float32).contiguous()
    if tuple(ch.shape) != (rows, COLS) or not frames:
        raise ValueError(f"channels must be ({rows}, {COLS}), got {tuple(ch.shape)}")
    root_rest = torch.as_tensor(root_rest).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(root_rest.shape) != (S, 3):
        raise ValueError(f"root_rest must be ({S}, 3), got {tuple(root_rest.shape)}")
    dfs = [int(j) for j in np.asarray(dfs).reshape(-1)]
    poses, trans = torch.empty(rows, NJ, 3, dtype=torch.float32, device=dev), torch.empty(rows, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().amuse_bvh_decode(_ptr(ch), S, (C.c_int * S)(*frames), (C.c_int * NJ)(*dfs), _order_index(o["order"]), C.c_float(o["scale"]),
                                                _ptr(root_rest), _ptr(poses), _ptr(trans), torch.cuda.current_stream(dev).cuda_stream))
    return poses, trans


# ------------------------------------------------------------------ files
def bvh_path(npz_path, out_dir=None) -> Path:
    """*_motion_smplx.npz -> *_motion.bvh, beside it or in out_dir"""
    return motion_file.sibling(npz_path, "_motion.bvh", out_dir)


def npz_path_of(bvh_file, out_dir=None) -> Path:
    """*_motion.bvh -> *_from_bvh_motion_smplx.npz (never the name of the NPZ the BVH was made from)"""
    return motion_file.sibling(bvh_file, "_from_bvh_motion_smplx.npz", out_dir, strip="_motion.bvh")


def motion_to_bvh_batch(npz_paths: Sequence, models: dict, out_dir=None, order: str = DEFAULT_ORDER, scale: float = DEFAULT_SCALE, unwrap: bool = False,
                        device="cuda") -> List[Path]:
    """Every *_motion_smplx.npz -> *_motion.bvh (and its .json side file) holding what the NPZ holds.  models: {gender: BodyModel} (body.load_models).  All files
    go through the kernels in ONE call (in calls of MAX_ROWS_PER_CALL rows when there are more) and come back in one copy; a file's bytes do not depend on the
    files beside it.  A motion with a value the field cannot hold raises BvhRangeError naming the file; nothing of that file is written."""
    import torch
    o = options(order, scale, unwrap)
    paths = [Path(p) for p in npz_paths]
    out: List[Path] = []
    rest: Dict[tuple, np.ndarray] = {}
    dfs_of: Dict[str, np.ndarray] = {}
    i = 0
    while i < len(paths):
        group, rows = [], 0
        while i < len(paths) and (not group or rows + group[-1][0].poses.shape[0] <= MAX_ROWS_PER_CALL):
            m = motion_file.read(paths[i])
            if m.gender not in models:
                raise ValueError(f"{paths[i]}: no SMPL-X model for gender {m.gender!r} among {sorted(models)}")
            key = (m.gender, m.betas.tobytes())
            if key not in rest:
                rest[key] = rest_joints(models[m.gender], m.betas)
            if m.gender not in dfs_of:
                dfs_of[m.gender] = layout(models[m.gender].parents)
            rows += m.poses.shape[0]
            group.append((m, rest[key]))
            i += 1
        # one call per parent list (the SMPL-X models of the three genders share theirs: one call)
        by_dfs: Dict[bytes, list] = {}
        for m, J in group:
            by_dfs.setdefault(dfs_of[m.gender].tobytes(), []).append((m, J))
        for part in by_dfs.values():
            frames = [m.poses.shape[0] for m, _ in part]
            _, text, status = motion_channels(torch.from_numpy(np.concatenate([m.poses for m, _ in part])).to(device),
                                              torch.from_numpy(np.concatenate([m.trans for m, _ in part])).to(device),
                                              torch.from_numpy(np.stack([J[0] for _, J in part]).astype(np.float32)), frames, dfs_of[part[0][0].gender], **o)
            text, status = text.cpu().numpy(), status.cpu().numpy()
            r0 = 0
            for (m, J), F, st in zip(part, frames, status):
                if st:
                    raise BvhRangeError(f"{m.path}: a channel of this motion does not fit the BVH field (|value| >= 1000 at six decimals): lower --bvh-scale"
                                        + (", or drop --bvh-unwrap (an unwrapped curve may wind past 1000 degrees)" if o["unwrap"] else ""))
                meta = {"gender": m.gender, "betas": [float(b) for b in m.betas], "scale": o["scale"], "order": o["order"],
                        "root_rest": [float(x) for x in J[0]], "mocap_frame_rate": m.fps}
                out.append(write_bvh(bvh_path(m.path, out_dir), header_text(models[m.gender].parents, J, F, m.fps, o["order"], o["scale"]),
                                     text[r0 * ROW_BYTES:(r0 + F) * ROW_BYTES].tobytes(), meta))
                r0 += F
    return out


def bvh_to_motion(bvh_files: Sequence, out_dir=None, device="cuda", scale: Optional[float] = None) -> List[Path]:
    """Every *_motion.bvh of this skeleton -> *_from_bvh_motion_smplx.npz (poses, trans, gender, betas, mocap_frame_rate), decoded by amuse_bvh_decode.  Gender,
    betas, scale, the root's rest position and the frame rate come from the side file; without one: neutral, zeros, `scale` (default 100), zero, 1 / Frame Time."""
    import torch
    out = []
    for f in bvh_files:
        b = read_bvh(f)
        m = b["meta"] or {}
        sc = float(m.get("scale", DEFAULT_SCALE if scale is None else scale))
        poses, trans = decode(torch.from_numpy(b["channels"].astype(np.float32)).to(device), [b["frames"]], b["dfs"], b["order"], sc,
                              np.asarray(m.get("root_rest", [0.0, 0.0, 0.0]), dtype=np.float32)[None])
        out.append(motion_file.save(npz_path_of(f, out_dir), poses=poses.cpu().numpy(), trans=trans.cpu().numpy().astype(np.float64),
                                    gender=np.array(m.get("gender", "neutral"), dtype="<U7"), betas=np.asarray(m.get("betas", np.zeros(300)), dtype=np.float64),
                                    mocap_frame_rate=np.array(m.get("mocap_frame_rate", round(1.0 / b["frame_time"], 2)), dtype="float64")))
    return out


# ------------------------------------------------------------------ python -m amuse_amd.bvh
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m amuse_amd.bvh", description="*_motion_smplx.npz files as BVH of the SMPL-X skeleton (MOTION block written in HIP), and back")
    ap.add_argument("files", nargs="+", help="*_motion_smplx.npz of any earlier run; with --to-npz, *_motion.bvh files of this skeleton")
    ap.add_argument("--to-npz", action="store_true", help="the other way: BVH files written by this tool -> *_from_bvh_motion_smplx.npz")
    ap.add_argument("--smplx-models", default=None, help="directory with SMPLX_MALE / FEMALE / NEUTRAL.npz: the rest joints the offsets are taken from")
    ap.add_argument("-o", "--out-dir", default=None, help="where the files go (default: beside each input)")
    ap.add_argument("--order", default=None, help=f"rotation channel order, one of {', '.join(ORDERS)} (default {DEFAULT_ORDER})")
    ap.add_argument("--scale", type=float, default=None, help="length unit of the file per metre (default 100: centimetres, a recollection of what BVH consumers expect)")
    ap.add_argument("--unwrap", action="store_true", help="continuous curves: each frame takes the Euler triple nearest the frame before (same rotations)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.to_npz:
        if args.order is not None or args.unwrap or args.smplx_models:
            ap.error("--order / --unwrap / --smplx-models belong to the NPZ -> BVH direction: --to-npz reads the order from the file's CHANNELS lines")
    else:
        if not args.smplx_models:
            ap.error("--smplx-models DIR is needed: the hierarchy's offsets are the rest joints of the SMPL-X body models")
        try:
            options(args.order, args.scale)
        except ValueError as e:
            ap.error(str(e))
    return args


def main(argv=None) -> List[Path]:
    args = parse_args(argv)
    for f in args.files:
        if not Path(f).is_file():
            raise SystemExit(f"{f} does not exist")
    if args.to_npz:
        written = bvh_to_motion(args.files, args.out_dir, args.device, args.scale)
    else:
        from . import body
        try:
            written = motion_to_bvh_batch(args.files, body.require_models(args.smplx_models), args.out_dir, args.order, args.scale, args.unwrap, args.device)
        except BvhRangeError as e:
            raise SystemExit(str(e).replace("--bvh-scale", "--scale").replace("--bvh-unwrap", "--unwrap"))
    for p in written:
        print(f"[amuse_amd] bvh: {p}")
    return written


if __name__ == "__main__":
    main()
