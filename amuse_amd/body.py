"""SMPL-X body model: joints, vertices and the vertex-displacement sums of a motion, without a PyTorch `smplx` install.

BodyModel holds the arrays a user loads from their own SMPLX_*.npz (the assets are licensed; the code needs none of them: the algorithm - linear blend
skinning - is generic in the vertex count).  BodyEngine runs it in HIP (include/amuse_hip.h amuse_body_*, csrc/k_body.hip); torch_forward / torch_loss_sums are
the plain float64 torch twin that serves `--device cpu` training.  `smplx` is not a dependency: both restate the published algorithm
(SMPLX(num_betas, use_pca=False, flat_hand_mean=True) called with expression = 0, as the reference's trainer builds it)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib

NJ = 55
NPZ_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kintree_table")   # as recollected from the published package's model files


class BodyModel:
    """v_template [V,3], shapedirs [V,3,B], posedirs [486,V*3], J_regressor [55,V], weights [V,55] (float32), parents [55] (int32, parents[0] = -1);
    faces [T,3] (int32, optional: the mesh's triangles, which only the preview renderer reads - amuse_amd/render.py)."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, parents, faces=None):
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        self.v_template, self.shapedirs, self.posedirs = f(v_template), f(shapedirs), f(posedirs)
        self.J_regressor, self.weights = f(J_regressor), f(weights)
        self.parents = np.ascontiguousarray(np.asarray(parents).astype(np.int64).astype(np.int32))
        V = self.V = int(self.v_template.shape[0])
        self.n_betas = int(self.shapedirs.shape[-1])
        want = {"v_template": (V, 3), "shapedirs": (V, 3, self.n_betas), "posedirs": (486, V * 3), "J_regressor": (NJ, V), "weights": (V, NJ), "parents": (NJ,)}
        for k, shp in want.items():
            if tuple(getattr(self, k).shape) != shp:
                raise ValueError(f"BodyModel: {k} has shape {tuple(getattr(self, k).shape)}, expected {shp}")
        if self.parents[0] != -1 or any(not (0 <= self.parents[j] < j) for j in range(1, NJ)):
            raise ValueError("BodyModel: parents must have parents[0] = -1 and 0 <= parents[j] < j")
        self.faces = None
        if faces is not None:
            fc = np.asarray(faces)
            if fc.ndim != 2 or fc.shape[1] != 3 or fc.shape[0] < 1 or int(fc.min()) < 0 or int(fc.max()) >= V:
                raise ValueError(f"BodyModel: faces has shape {tuple(fc.shape)}: expected [T, 3] vertex indices in 0..{V - 1}")
            self.faces = np.ascontiguousarray(fc.astype(np.int64).astype(np.int32))

    @classmethod
    def from_dict(cls, d: dict) -> "BodyModel":
        return cls(d["v_template"], d["shapedirs"], d["posedirs"], d["J_regressor"], d["weights"], d["parents"], d.get("faces"))

    @classmethod
    def from_npz(cls, path, num_betas: int = 300) -> "BodyModel":
        """A user's SMPL-X model file.  posedirs is [V][3][486] in the file and is transposed here; shapedirs keeps its first num_betas columns (the
        expression columns behind them multiply zeros in the reference's call); kintree_table's first row is the parent list."""
        with np.load(str(path), allow_pickle=False) as z:   # only the six numeric arrays are read: nothing of a user-supplied file is unpickled
            for k in NPZ_KEYS:
                if k not in z.files:
                    raise KeyError(f"{path}: SMPL-X model file lacks the key '{k}' (needs {', '.join(NPZ_KEYS)})")
            d = {k: np.asarray(z[k]) for k in NPZ_KEYS}
            faces = np.asarray(z["f"]) if "f" in z.files else None   # the triangles: optional, the preview renderer's only
        V = d["v_template"].shape[0]
        parents = d["kintree_table"][0].astype(np.int64)[:NJ].copy()
        parents[0] = -1   # stored as 2^32 - 1
        posedirs = np.asarray(d["posedirs"], np.float32).reshape(V * 3, -1).T
        return cls(d["v_template"], np.asarray(d["shapedirs"])[:, :, :num_betas], posedirs, np.asarray(d["J_regressor"])[:NJ], np.asarray(d["weights"])[:, :NJ], parents, faces)

    def to_npz(self, path) -> None:
        """the file layout from_npz reads (tests; a user's own models)"""
        kt = np.stack([self.parents.astype(np.int64) % (1 << 32), np.arange(NJ)]).astype(np.uint32)
        extra = {} if self.faces is None else {"f": self.faces.astype(np.uint32)}     # written only when set: a file without it keeps its bytes
        np.savez(str(path), v_template=self.v_template, shapedirs=self.shapedirs, posedirs=self.posedirs.T.reshape(self.V, 3, 486), J_regressor=self.J_regressor,
                 weights=self.weights, kintree_table=kt, **extra)


# ------------------------------------------------------------------ the float64 torch twin
def _rodrigues(rv: torch.Tensor) -> torch.Tensor:
    angle = torch.linalg.vector_norm(rv + 1e-8, dim=-1, keepdim=True)
    d = rv / angle
    c, s = torch.cos(angle)[..., None], torch.sin(angle)[..., None]
    rx, ry, rz = d.unbind(-1)
    z = torch.zeros_like(rx)
    K = torch.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], -1).reshape(rv.shape[:-1] + (3, 3))
    return torch.eye(3, dtype=rv.dtype, device=rv.device) + s * K + (1 - c) * (K @ K)


def _rot6d(d6: torch.Tensor) -> torch.Tensor:
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / torch.linalg.vector_norm(a1, dim=-1, keepdim=True).clamp_min(1e-12)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / torch.linalg.vector_norm(b2, dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -2)


def _split_rows(rows: torch.Tensor, kind: str):
    """feature rows [N,F,333] (6d) / motion rows [N,F,168] (aa) -> rotations [N,F,55,6|3], translation [N,F,3]"""
    w = 6 if kind == "6d" else 3
    return rows[..., :NJ * w].reshape(rows.shape[:-1] + (NJ, w)), rows[..., NJ * w:NJ * w + 3]


def torch_forward(model: BodyModel, betas, rot, trans=None, subject=None, kind: str = "aa", frames_per_pass: int = 64, differentiable: bool = False):
    """float64 on rot's device: betas [S,B], rot [N,F,55,3] / [N,F,55,6], trans [N,F,3] or None, subject [N] (default: clip n -> row n % S)
    -> joints [N,F,55,3], vertices [N,F,V,3].  differentiable: rot / trans are not detached, so autograd reaches them (the oracle of the HIP backward pass)."""
    dev = rot.device
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=dev) if not torch.is_tensor(a) else a.to(dev, torch.float64)
    rot = (rot if differentiable else rot.detach()).to(torch.float64)
    N, F = rot.shape[:2]
    V = model.V
    betas = t64(betas)
    sub = torch.arange(N, device=dev) % betas.shape[0] if subject is None else torch.as_tensor(subject, device=dev).long().clamp(0, betas.shape[0] - 1)
    tr = torch.zeros(N, F, 3, dtype=torch.float64, device=dev) if trans is None else (trans if differentiable else trans.detach()).to(torch.float64)
    vs = t64(model.v_template)[None] + torch.einsum("vcb,nb->nvc", t64(model.shapedirs), betas[sub])
    J = torch.einsum("jv,nvc->njc", t64(model.J_regressor), vs)
    P, W = t64(model.posedirs), t64(model.weights)
    joints, verts = [], []
    for f0 in range(0, F, frames_per_pass):
        r, t = rot[:, f0:f0 + frames_per_pass], tr[:, f0:f0 + frames_per_pass]
        f = r.shape[1]
        R = _rodrigues(r) if kind == "aa" else _rot6d(r)
        pf = (R[:, :, 1:] - torch.eye(3, dtype=torch.float64, device=dev)).reshape(N, f, 486)
        vp = vs[:, None] + (pf @ P).reshape(N, f, V, 3)
        GR, Gt = [None] * NJ, [None] * NJ
        for j in range(NJ):
            p = int(model.parents[j])
            if p < 0:
                GR[j], Gt[j] = R[:, :, j], J[:, None, j].expand(N, f, 3)
            else:
                GR[j] = GR[p] @ R[:, :, j]
                Gt[j] = (GR[p] @ (J[:, None, j] - J[:, None, p])[..., None])[..., 0] + Gt[p]
        GR, Gt = torch.stack(GR, 2), torch.stack(Gt, 2)
        At = Gt - (GR @ J[:, None, :, :, None])[..., 0]
        A = torch.cat([GR, At[..., None]], -1).reshape(N, f, NJ, 12)
        T = torch.einsum("vj,nfjk->nfvk", W, A).reshape(N, f, V, 3, 4)
        joints.append(Gt + t[:, :, None])
        verts.append((T[..., :3] @ vp[..., None])[..., 0] + T[..., 3] + t[:, :, None])
    return torch.cat(joints, 1), torch.cat(verts, 1)


def _smooth_l1_sum(a, ref):
    d = (a - ref).abs()
    return torch.where(d < 1.0, 0.5 * d * d, d - 0.5).sum()


def torch_loss_sums(model: BodyModel, betas, ref, a, b=None, subject=None, kind: str = "6d", frames_per_pass: int = 32, differentiable: bool = False) -> torch.Tensor:
    """SmoothL1 (beta 1) SUMS of (a, ref) and (b, ref) over the vertices, float64 [2]; ref / a / b are rows: [N,F,333] (6d) or [N,F,168] (aa).
    differentiable: the sums carry gradient to a and b (never to ref, as in amuse_body_vertex_loss_grad)."""
    if differentiable:
        parts = [[], []]
        for f0 in range(0, ref.shape[1], frames_per_pass):
            sl = slice(f0, f0 + frames_per_pass)
            vr = torch_forward(model, betas, *_split_rows(ref[:, sl], kind), subject=subject, kind=kind)[1]
            for i, c in enumerate((a, b)):
                if c is not None:
                    parts[i].append(_smooth_l1_sum(torch_forward(model, betas, *_split_rows(c[:, sl], kind), subject=subject, kind=kind, differentiable=True)[1], vr))
        zero = torch.zeros((), dtype=torch.float64, device=ref.device)
        return torch.stack([torch.stack(p).sum() if p else zero for p in parts])
    out = torch.zeros(2, dtype=torch.float64, device=ref.device)
    F = ref.shape[1]
    for f0 in range(0, F, frames_per_pass):
        sl = slice(f0, f0 + frames_per_pass)
        vr = torch_forward(model, betas, *_split_rows(ref[:, sl], kind), subject=subject, kind=kind)[1]
        for i, c in enumerate((a, b)):
            if c is not None:
                out[i] += _smooth_l1_sum(torch_forward(model, betas, *_split_rows(c[:, sl], kind), subject=subject, kind=kind)[1], vr)
    return out


# ------------------------------------------------------------------ the HIP engine
_PREC = {"fp32x": _lib.PREC_F32X, "fp16": _lib.PREC_F16}
_KIND = {"aa": _lib.BODY_ROT_AA, "6d": _lib.BODY_ROT_6D}


class BodyEngine:
    """One body model on one GPU.  Every compute call is stream-ordered on torch's current stream; after reserve() (or a first call of the same size) none of
    them allocates or synchronises, so they can be captured in a graph.  `subject` is a DEVICE int32 tensor [N] (rows of set_subjects); None = all zeros."""

    def __init__(self, device, model: BodyModel, precision: str = "fp32x"):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("BodyEngine runs on a GPU; on the CPU use body.torch_forward / body.torch_loss_sums")
        self.model, self.precision = model, precision
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        m = _lib.BodyModelC(model.V, model.n_betas, model.v_template.ctypes.data_as(fp), model.shapedirs.ctypes.data_as(fp), model.posedirs.ctypes.data_as(fp),
                            model.J_regressor.ctypes.data_as(fp), model.weights.ctypes.data_as(fp), model.parents.ctypes.data_as(ip))
        self.ctx = self.lib.amuse_body_create(self.device.index or 0, C.byref(m))
        if not self.ctx:
            raise _lib.AmuseHipError(f"amuse_body_create: {self.lib.amuse_last_error().decode()}")
        self.n_subjects = 0
        self._zeros = torch.zeros(4096, dtype=torch.int32, device=self.device)   # subject None: allocated here, not inside a captured call

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.amuse_body_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def info(self) -> dict:
        return {k: self.lib.amuse_body_info(self.ctx, i) for i, k in enumerate(("V", "skin_nnz", "posedirs_shift", "subjects", "grad"))}

    def enable_grad(self) -> None:
        """Upload the transposed posedirs image vertex_loss_grad needs (about 86 MB at V = 10,475) and let reserve() size the backward partials too.  Allocates
        and copies synchronously: call it BEFORE capturing a graph, and reserve() after it.  Idempotent."""
        _lib.check(self.lib.amuse_body_enable_grad(self.ctx))

    def set_subjects(self, betas) -> None:
        b = np.ascontiguousarray(np.asarray(betas, dtype=np.float32).reshape(-1, self.model.n_betas))
        _lib.check(self.lib.amuse_body_set_subjects(self.ctx, b.ctypes.data_as(C.POINTER(C.c_float)), b.shape[0]))
        self.n_subjects = b.shape[0]

    def reserve(self, frames: int) -> None:
        """Size the workspace for calls of up to `frames` = N * F frames.  Growing allocates, so call this (or run the call once eagerly) BEFORE capturing a graph;
        an outgrown workspace stays alive until close(), graphs captured earlier keep replaying.  One workspace per engine: its calls must not overlap on two streams."""
        _lib.check(self.lib.amuse_body_reserve(self.ctx, int(frames)))

    def _subject(self, subject, N):
        if subject is None:
            if self._zeros.numel() < N:
                self._zeros = torch.zeros(N, dtype=torch.int32, device=self.device)
            return self._zeros
        assert subject.dtype == torch.int32 and subject.is_cuda and subject.is_contiguous() and subject.numel() >= N, "subject: device int32 [N]"
        return subject

    def _f32(self, x):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(), "device float32, contiguous"
        return x

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def forward(self, rot, trans=None, subject=None, kind: str = "aa", joints: bool = True, vertices: bool = True, precision: Optional[str] = None):
        """kind "aa": rot [N,F,55,3] (+ trans [N,F,3] or None); "6d": rot = feature rows [N,F,333].  -> (joints [N,F,55,3] | None, vertices [N,F,V,3] | None)"""
        rot = self._f32(rot)
        N, F = int(rot.shape[0]), int(rot.shape[1])
        assert rot.numel() == N * F * (165 if kind == "aa" else 333), tuple(rot.shape)
        jo = torch.empty(N, F, NJ, 3, device=self.device) if joints else None
        vo = torch.empty(N, F, self.model.V, 3, device=self.device) if vertices else None
        tp = self._f32(trans).data_ptr() if (trans is not None and kind == "aa") else None
        _lib.check(self.lib.amuse_body_forward(self.ctx, rot.data_ptr(), _KIND[kind], tp, self._subject(subject, N).data_ptr(), N, F, _PREC[precision or self.precision],
                                               jo.data_ptr() if joints else None, vo.data_ptr() if vertices else None, self._stream()))
        return jo, vo

    def joints(self, rot, trans=None, subject=None, kind: str = "aa"):
        return self.forward(rot, trans, subject, kind, vertices=False)[0]

    def vertices(self, rot, trans=None, subject=None, kind: str = "aa", precision: Optional[str] = None):
        return self.forward(rot, trans, subject, kind, joints=False, precision=precision)[1]

    def vertex_loss(self, ref, a, b=None, subject=None, kind: str = "6d", out: Optional[torch.Tensor] = None, precision: Optional[str] = None) -> torch.Tensor:
        """SmoothL1 SUMS of (a, ref) and (b, ref) over all vertex coordinates: device float64 [2] (`out` to write in place).  Rows [N,F,333] (6d) or [N,F,168] (aa)."""
        ref, a = self._f32(ref), self._f32(a)
        N, F = int(ref.shape[0]), int(ref.shape[1])
        w = 333 if kind == "6d" else 168
        assert ref.numel() == N * F * w and a.shape == ref.shape and (b is None or b.shape == ref.shape), (tuple(ref.shape), tuple(a.shape))
        out = torch.empty(2, dtype=torch.float64, device=self.device) if out is None else out
        assert out.dtype == torch.float64 and out.is_cuda and out.numel() >= 2
        _lib.check(self.lib.amuse_body_vertex_loss(self.ctx, ref.data_ptr(), a.data_ptr(), self._f32(b).data_ptr() if b is not None else None, _KIND[kind],
                                                   self._subject(subject, N).data_ptr(), N, F, _PREC[precision or self.precision], out.data_ptr(), self._stream()))
        return out


    def vertex_loss_grad(self, ref, a, b=None, subject=None, scale=(1.0, 1.0), out=None, precision: Optional[str] = None):
        """scale[i] x d(SmoothL1 sum of (a | b, ref))/d(a | b): feature rows [N,F,333] (6D only) -> (grad_a, grad_b | None), device float32 [N,F,333].  `out`:
        a pair of tensors to write into (rows of skipped clips are left as they are; without `out` they are zero).  Needs enable_grad().  Deterministic."""
        ref, a = self._f32(ref), self._f32(a)
        N, F = int(ref.shape[0]), int(ref.shape[1])
        assert ref.numel() == N * F * 333 and a.shape == ref.shape and (b is None or b.shape == ref.shape), (tuple(ref.shape), tuple(a.shape))
        ga, gb = out if out is not None else (torch.zeros_like(a), torch.zeros_like(a) if b is not None else None)
        assert self._f32(ga).shape == a.shape and (b is None or self._f32(gb).shape == a.shape)
        _lib.check(self.lib.amuse_body_vertex_loss_grad(self.ctx, ref.data_ptr(), a.data_ptr(), self._f32(b).data_ptr() if b is not None else None, _lib.BODY_ROT_6D,
                                                        self._subject(subject, N).data_ptr(), N, F, _PREC[precision or self.precision], float(scale[0]), float(scale[1]),
                                                        ga.data_ptr(), gb.data_ptr() if b is not None else None, self._stream()))
        return ga, (gb if b is not None else None)


class VertexLossFn(torch.autograd.Function):
    """sums [2] (float64) = BodyEngine.vertex_loss(ref, a, b) for EVERY engine of `engines` ([(engine, subject int32 [N]), ...]: the gendered split, each engine
    skipping the other's clips), differentiable in a and b (6D feature rows).  Backward runs amuse_body_vertex_loss_grad for the inputs that require grad - each
    engine writes its own clips' rows of one zero-initialised buffer - and multiplies by grad_output once.  A candidate that needs no gradient is not passed
    to the backward kernels at all."""

    @staticmethod
    def forward(ctx, engines, ref, a, b, precision):
        total = None
        for eng, sub in engines:
            s = eng.vertex_loss(ref, a, b, sub, "6d", precision=precision)
            total = s if total is None else total + s
        ctx.engines, ctx.precision, ctx.has_b = engines, precision, b is not None
        ctx.save_for_backward(ref, a, *([b] if b is not None else []))
        return total

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        ref, a, b = saved[0], saved[1], (saved[2] if ctx.has_b else None)
        need_a, need_b = ctx.needs_input_grad[2], ctx.has_b and ctx.needs_input_grad[3]
        ga = gb = None
        if need_a or need_b:
            # the kernel's first candidate is the one that needs a gradient; the second rides along only if both do
            first, second = (a, b if need_b else None) if need_a else (b, None)
            g1, g2 = torch.zeros_like(first), (torch.zeros_like(first) if second is not None else None)
            for eng, sub in ctx.engines:
                eng.vertex_loss_grad(ref, first, second, sub, out=(g1, g2), precision=ctx.precision)
            go = grad_out.to(torch.float32)
            if need_a:
                ga = g1 * go[0]
                gb = g2 * go[1] if need_b else None
            else:
                gb = g1 * go[1]
        return None, None, ga, gb, None


SMPLX_FILES = {"male": "SMPLX_MALE.npz", "female": "SMPLX_FEMALE.npz", "neutral": "SMPLX_NEUTRAL.npz"}


def models_present(directory) -> bool:
    return all((Path(directory) / f).is_file() for f in SMPLX_FILES.values())


def load_models(directory, num_betas: int = 300) -> dict:
    """{"male" | "female" | "neutral": BodyModel} from <directory>/SMPLX_{MALE,FEMALE,NEUTRAL}.npz (the reference's trainer.py:94-104 loads the same three)."""
    return {g: BodyModel.from_npz(Path(directory) / f, num_betas) for g, f in SMPLX_FILES.items()}


def require_models(directory, who: str = "", hint: str = "(--smplx-models DIR names the directory)", faces: bool = False, load: bool = True) -> Optional[dict]:
    """What every command line calls: the three files are in `directory` - else SystemExit names them and the directory, `who` ("--bvh: ") in front and `hint`
    behind - and are loaded (load=False: checked only); faces: every model must carry its triangles (the preview renderer's need)."""
    if not models_present(directory):
        raise SystemExit(f"{who}{', '.join(SMPLX_FILES.values())} were not all found in {directory} {hint}")
    models = load_models(directory) if load else None
    for g, m in (models or {}).items():
        if faces and m.faces is None:
            raise SystemExit(f"{who}{Path(directory) / SMPLX_FILES[g]} lacks the key 'f' (the mesh's triangles, [T][3]): without them there is nothing to rasterise")
    return models


def fit_betas(betas, n_betas: int) -> np.ndarray:
    """a motion file's betas as a model takes them: float32 [n_betas], cut to the model's count, zero-padded if the file holds fewer"""
    b = np.asarray(betas, dtype=np.float32).reshape(-1)[:n_betas]
    return np.pad(b, (0, n_betas - b.size))


class Poser:
    """What a module that poses motion files owns: the BodyEngine of every gender over `models` ({gender: BodyModel}), created on first use, closed by close()"""

    def __init__(self, models: dict, device="cuda:0"):
        self.models, self.device, self.engines = models, device, {}

    def engine(self, gender: str) -> BodyEngine:
        if gender not in self.engines:
            self.engines[gender] = BodyEngine(self.device, self.models[gender])
        return self.engines[gender]

    def pose(self, motion):
        """a motion_file.read record -> (its gender's engine with the file's betas set as subject 0, rot [1, F, 55, 3], trans [1, F, 3] on the device), ready for
        engine.joints(rot, trans) / .vertices(rot, trans).  A gender without a model is a KeyError: whether to refuse or to fall back is the caller's."""
        eng = self.engine(motion.gender)
        eng.set_subjects(fit_betas(motion.betas, eng.model.n_betas)[None])
        return eng, torch.from_numpy(motion.poses[None]).to(eng.device), torch.from_numpy(motion.trans[None]).to(eng.device)

    def close(self) -> None:
        for e in self.engines.values():
            e.close()
        self.engines = {}


class BodyLosses:
    """The `body` of train_gesture.LatentPriorLosses: the reference's _get_vertices + the two SmoothL1 terms (latent_losses.py:135-146,173-250) as VALUES (the
    reference computes them under no_grad).  Dataset version "v0": every clip goes through the male or the female model by its actor's gender; "v1": all through
    the neutral one.  Betas: the per-actor table this project ships (npz_writer.fetchbetas).  On a GPU each model is a BodyEngine and the gendered split is
    DEVICE data - one int32 subject row per model, -1 where the clip belongs to the other one - so a captured training step replays with new batches; on the CPU
    the float64 torch twin runs on the selected clips.
    DEVIATION from the reference, stated: the trainer feeds the 6D feature rows it already has (rotation by rotation_6d_to_matrix's Gram-Schmidt); the reference
    converts matrix -> axis-angle -> matrix first, which is the identity up to fp32 rounding (tests/test_body_host_cpu.py holds the two together)."""

    def __init__(self, models: dict, device, version: str = "v0", precision: str = "fp32x", actors=None, grad: bool = False):
        from . import npz_writer
        self.device, self.version, self.grad = torch.device(device), version, bool(grad)
        if version not in ("v0", "v1"):
            raise ValueError(f"dataset version {version!r}: v0 (gendered models) or v1 (neutral)")
        self.genders = ("male", "female") if version == "v0" else ("neutral",)
        for g in self.genders:
            if g not in models:
                raise KeyError(f"BodyLosses: no '{g}' body model (dataset version {version} needs {', '.join(self.genders)})")
        self.models = {g: models[g] for g in self.genders}
        self.V = self.models[self.genders[0]].V
        assert all(m.V == self.V for m in self.models.values()), "the body models differ in their vertex count"
        self.actors = list(actors if actors is not None else npz_writer.MALE + npz_writer.FEMALE)
        rows, self.row_of = [], {}
        for a in self.actors:
            try:
                b = npz_writer.fetchbetas(a)
            except NotImplementedError:
                continue                       # no MoSh fit: the reference raises when such an actor turns up in a batch, and so does subjects()
            self.row_of[a] = len(rows)
            rows.append(np.asarray(b, np.float32)[:self.models[self.genders[0]].n_betas])
        self.betas = np.stack(rows)
        self.engines = {}
        if self.device.type == "cuda":
            for g in self.genders:
                self.engines[g] = BodyEngine(self.device, self.models[g], precision)
                self.engines[g].set_subjects(self.betas)
                if self.grad:
                    self.engines[g].enable_grad()
            self._out = {g: torch.zeros(2, dtype=torch.float64, device=self.device) for g in self.genders}

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines = {}

    def subject_rows(self, attr) -> np.ndarray:
        """ld_attr [(actor, gender), ...] -> int32 [len(genders)][B]: the clip's betas row in its model's list, -1 in the other's"""
        from . import npz_writer
        out = np.full((len(self.genders), len(attr)), -1, np.int32)
        for n, a in enumerate(attr):
            actor = a[0]
            if actor not in self.row_of:
                raise NotImplementedError(f"Actor not found {actor}")
            g = "neutral" if self.version == "v1" else (a[1] if len(a) > 1 and a[1] in ("male", "female") else npz_writer.subject2gender(actor))
            out[self.genders.index(g), n] = self.row_of[actor]
        return out

    def subjects(self, attr) -> torch.Tensor:
        return torch.from_numpy(self.subject_rows(attr)).to(self.device)

    def reserve(self, frames: int) -> None:
        for e in self.engines.values():
            e.reserve(frames)

    def _terms_grad(self, m_ref, m_rst, gen_m_rst, attr, subjects):
        """terms() with gradient: DEVIATION from the reference, opt-in (its vertices are computed under no_grad, latent_losses.py:173).  The two means carry
        gradient to m_rst, and to gen_m_rst when that requires grad; the reference motion gets none.  The gendered split stays device data."""
        B, F = int(m_ref.shape[0]), int(m_ref.shape[1])
        subjects = self.subjects(attr) if subjects is None else subjects
        f = lambda x: None if x is None else x.to(torch.float32).contiguous()
        ref, rst, gen = f(m_ref.detach()), f(m_rst), f(gen_m_rst)
        if self.device.type == "cuda":
            for e in self.engines.values():
                e.enable_grad()
            total = VertexLossFn.apply([(self.engines[g], subjects[i]) for i, g in enumerate(self.genders)], ref, rst, gen, None)
        else:
            rows = subjects.cpu().numpy()
            total = torch.zeros(2, dtype=torch.float64)
            for i, g in enumerate(self.genders):
                idx = np.nonzero(rows[i] >= 0)[0]
                if len(idx):
                    pick = lambda x: None if x is None else x[idx]
                    total = total + torch_loss_sums(self.models[g], self.betas, pick(ref), pick(rst), pick(gen), subject=rows[i][idx], kind="6d", differentiable=True)
        mean = (total / float(B * F * self.V * 3)).to(torch.float32)
        return mean[0], mean[1]

    def terms(self, m_ref, m_rst, gen_m_rst=None, attr=None, subjects=None, grad: Optional[bool] = None):
        """feature rows [B,F,333] -> (rec_vtex_displacement, gen_vtex_displacement): SmoothL1 means over B F V 3, float32 scalars on the device, no gradient
        (grad, default the constructor's: with gradient, see _terms_grad); gen is 0 without a generation (a CPU run has no in-loop sampler)."""
        if self.grad if grad is None else grad:
            return self._terms_grad(m_ref, m_rst, gen_m_rst, attr, subjects)
        with torch.no_grad():
            B, F = int(m_ref.shape[0]), int(m_ref.shape[1])
            subjects = self.subjects(attr) if subjects is None else subjects
            f = lambda x: None if x is None else x.detach().to(torch.float32).contiguous()
            ref, rst, gen = f(m_ref), f(m_rst), f(gen_m_rst)
            total = None
            if self.device.type == "cuda":
                for i, g in enumerate(self.genders):
                    s = self.engines[g].vertex_loss(ref, rst, gen, subjects[i], "6d", out=self._out[g])
                    total = s if total is None else total + s
            else:
                rows = subjects.cpu().numpy()
                total = torch.zeros(2, dtype=torch.float64)
                for i, g in enumerate(self.genders):
                    idx = np.nonzero(rows[i] >= 0)[0]
                    if len(idx):
                        pick = lambda x: None if x is None else x[idx]
                        total = total + torch_loss_sums(self.models[g], self.betas, pick(ref), pick(rst), pick(gen), subject=rows[i][idx], kind="6d")
            mean = (total / float(B * F * self.V * 3)).to(torch.float32)
            return mean[0], mean[1]
