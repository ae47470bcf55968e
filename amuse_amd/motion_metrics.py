"""Motion metrics - an extension, off by default: APE / AVE on posed SMPL-X joints (the per-clip sums in HIP: include/amuse_hip.h amuse_motion_metrics,
csrc/k_motion_metrics.hip) and FID / Diversity on the motion prior's latents.

The reference states the intent in models/latent_diffusion/utils/val_metrics.py (ComputeMetrics, TM2TMetrics), a file that cannot run: torchmetrics is absent
and Rifke, l2_norm, variance, calculate_frechet_distance_np and calculate_diversity_np are defined nowhere in its tree; its trainer passes metricsmodel=None.
What is here restates the accumulation (val_metrics.py:63-137) without torchmetrics.  DEVIATIONS, stated:
  - no heading normalisation (Rifke is not in the reference tree): the joints are compared as the body model poses them;
  - SMPL-X joints in metres instead of MMM features, so force_in_meter's factor is 1;
  - the variance and the Frechet distance are recollections of MLD's helpers, pinned only against their own restatement (tests/motion_metrics_ref.py);
  - velocity / acceleration sums are added: val_metrics.py has no jitter measure, and a sampler in reduced precision needs one;
  - no R-precision / Matching score: they need a text / audio-to-motion embedding this model does not have.

  python -m amuse_amd.motion_metrics GEN_DIR REF_DIR --smplx-models DIR      the joint half for two directories of *_motion_smplx.npz, matched by file name"""
from __future__ import annotations

import json
from contextlib import closing
from pathlib import Path
from typing import Dict, Optional

import numpy as np

NJ = 55
FPS = 30.0                   # the NPZ's mocap_frame_rate (npz_writer.smplx_npz_fields)
LATENT = 128

# The row of amuse_motion_metrics: (block, length) in order - include/amuse_hip.h states the same table, csrc/amuse_motion_metrics_host.hpp its offsets.  Every
# offset below comes from this table; tests hold its total to amuse_motion_metrics_row().
ROW_BLOCKS = (("ape_root", 1), ("ape_traj", 1), ("ape_pose", NJ - 1), ("ape_joints", NJ), ("ave_root", 1), ("ave_traj", 1), ("ave_pose", NJ - 1),
              ("ave_joints", NJ), ("vel_gen", NJ), ("vel_ref", NJ), ("acc_gen", NJ), ("acc_ref", NJ))
ROW = sum(n for _, n in ROW_BLOCKS)
ROW_SLICES: Dict[str, slice] = {}
_o = 0
for _name, _n in ROW_BLOCKS:
    ROW_SLICES[_name] = slice(_o, _o + _n)
    _o += _n
del _o, _name, _n


def split_row(rows) -> dict:
    """rows [..., 442] -> {block: [..., length]} (views)"""
    rows = np.asarray(rows)
    assert rows.shape[-1] == ROW, rows.shape
    return {k: rows[..., s] for k, s in ROW_SLICES.items()}


def joint_rows(G, R, lengths=None):
    """amuse_motion_metrics on torch device tensors: G, R float32 [N, F, 55, 3] (amuse_body_forward's joints), lengths device int32 [N] (None: every clip has F
    frames) -> device float64 [N, 442].  Stream-ordered on torch's current stream.  A clip whose length lies outside 2..F gets a row of NaN."""
    import torch
    from . import _lib
    lib = _lib.load()
    for x in (G, R):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("joint_rows: device float32, contiguous")
    if G.dim() != 4 or tuple(G.shape[2:]) != (NJ, 3) or G.shape != R.shape:
        raise ValueError(f"joint_rows: joints must be two [N, F, {NJ}, 3] tensors, got {tuple(G.shape)} and {tuple(R.shape)}")
    N, F = int(G.shape[0]), int(G.shape[1])
    if lengths is None:
        lengths = torch.full((N,), F, dtype=torch.int32, device=G.device)
    if not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous() and lengths.numel() == N):
        raise ValueError("joint_rows: lengths is a device int32 tensor [N]")
    assert lib.amuse_motion_metrics_row() == ROW
    rows = torch.empty(N, ROW, dtype=torch.float64, device=G.device)
    with torch.cuda.device(G.device):
        _lib.check(lib.amuse_motion_metrics(G.data_ptr(), R.data_ptr(), lengths.data_ptr(), N, F, rows.data_ptr(), torch.cuda.current_stream(G.device).cuda_stream))
    return rows


class JointMetrics:
    """ComputeMetrics (val_metrics.py:14-137) without torchmetrics: the additive state is the SUM of the per-clip rows, `count` (frames) and `count_seq`
    (clips); ranks and batches add (the reference's dist_reduce_fx="sum")."""

    def __init__(self):
        self.rows = np.zeros(ROW, np.float64)
        self.count = 0
        self.count_seq = 0

    def update(self, rows, lengths) -> None:
        rows = np.asarray(rows.detach().cpu().numpy() if hasattr(rows, "detach") else rows, np.float64).reshape(-1, ROW)
        lengths = np.asarray(lengths.detach().cpu().numpy() if hasattr(lengths, "detach") else lengths).astype(np.int64).reshape(-1)
        if len(lengths) != len(rows):
            raise ValueError(f"JointMetrics.update: {len(rows)} rows, {len(lengths)} lengths")
        if not np.isfinite(rows).all():
            raise ValueError("JointMetrics.update: a row is not finite (a clip's length outside 2..F gives a row of NaN)")
        self.rows += rows.sum(0)
        self.count += int(lengths.sum())
        self.count_seq += len(lengths)

    def state(self) -> dict:
        return {"rows": self.rows.copy(), "count": int(self.count), "count_seq": int(self.count_seq)}

    @classmethod
    def from_state(cls, st: dict) -> "JointMetrics":
        m = cls()
        return m.merge(st)

    def merge(self, other) -> "JointMetrics":
        st = other.state() if isinstance(other, JointMetrics) else other
        self.rows += np.asarray(st["rows"], np.float64)
        self.count += int(st["count"])
        self.count_seq += int(st["count_seq"])
        return self

    def compute(self) -> dict:
        """val_metrics.py:63-92: the APE entries over `count`, the AVE entries over `count_seq`; velocities in m/s and accelerations in m/s^2 (30 fps), averaged
        over the joints and over the frame differences counted (count - count_seq first differences, count - 2 count_seq second differences)."""
        if self.count_seq < 1:
            raise ValueError("JointMetrics.compute: nothing was accumulated")
        b = split_row(self.rows)
        c, cs = float(self.count), float(self.count_seq)
        out = {"APE_root": float(b["ape_root"][0] / c), "APE_traj": float(b["ape_traj"][0] / c),
               "APE_mean_pose": float(b["ape_pose"].mean() / c), "APE_mean_joints": float(b["ape_joints"].mean() / c),
               "AVE_root": float(b["ave_root"][0] / cs), "AVE_traj": float(b["ave_traj"][0] / cs),
               "AVE_mean_pose": float(b["ave_pose"].mean() / cs), "AVE_mean_joints": float(b["ave_joints"].mean() / cs),
               "APE_pose_per_joint": b["ape_pose"] / c, "APE_joints_per_joint": b["ape_joints"] / c,
               "AVE_pose_per_joint": b["ave_pose"] / cs, "AVE_joints_per_joint": b["ave_joints"] / cs}
        nv, na = c - cs, c - 2.0 * cs
        for tag in ("gen", "ref"):
            v = b[f"vel_{tag}"] * FPS / nv if nv > 0 else np.full(NJ, np.nan)
            a = b[f"acc_{tag}"] * FPS * FPS / na if na > 0 else np.full(NJ, np.nan)
            out[f"vel_{tag}"], out[f"acc_{tag}"] = float(v.mean()), float(a.mean())
            out[f"vel_{tag}_per_joint"], out[f"acc_{tag}_per_joint"] = v, a
        return out


def frechet_distance(mu1, cov1, mu2, cov2) -> float:
    """|mu1 - mu2|^2 + tr C1 + tr C2 - 2 tr (C1 C2)^(1/2), without scipy: tr (C1 C2)^(1/2) is the sum of the square roots of the eigenvalues of
    C1^(1/2) C2 C1^(1/2) - a symmetric positive semi-definite matrix with the non-zero spectrum of C1 C2 - from numpy.linalg.eigh in float64.  Rounding
    residue is clipped at 0: negative eigenvalues, and - because a square root turns a residue of 1e-16 into 1e-8, once per zero eigenvalue of a rank-deficient
    covariance (fewer clips than 128 dimensions) - everything below n eps lambda_max, numpy.linalg.matrix_rank's threshold.  The product is formed in the range
    of C1 (its eigenvectors above that threshold), so the null space of a rank-deficient C1 never enters."""
    mu1, mu2 = np.asarray(mu1, np.float64), np.asarray(mu2, np.float64)
    cov1, cov2 = np.atleast_2d(np.asarray(cov1, np.float64)), np.atleast_2d(np.asarray(cov2, np.float64))
    tiny = lambda ev: len(ev) * np.finfo(np.float64).eps * max(float(ev.max(initial=0.0)), 0.0)
    w, V = np.linalg.eigh((cov1 + cov1.T) * 0.5)
    keep = w > tiny(w)
    h = V[:, keep] * np.sqrt(w[keep])                     # C1^(1/2) restricted to C1's range: [n][k]
    M = h.T @ cov2 @ h
    ev = np.linalg.eigvalsh((M + M.T) * 0.5) if M.size else np.zeros(0)
    ev = np.where(ev > tiny(ev), ev, 0.0)
    d = mu1 - mu2
    return float(d @ d + np.trace(cov1) + np.trace(cov2) - 2.0 * np.sqrt(ev).sum())


def moments(x):
    x = np.asarray(x, np.float64)
    return x.mean(0), np.cov(x, rowvar=False)


def diversity(x, times: int, rng) -> float:
    """mean L2 distance between two index sets of `times` drawn without replacement (the reference's missing calculate_diversity_np, as MLD states it)"""
    x = np.asarray(x, np.float64)
    a, b = rng.choice(len(x), times, replace=False), rng.choice(len(x), times, replace=False)
    return float(np.linalg.norm(x[a] - x[b], axis=1).mean())


class LatentMetrics:
    """TM2TMetrics (val_metrics.py) WITHOUT its text half: FID, Diversity and gt_Diversity on the motion prior's deterministic latents (mu).  R-precision and
    Matching score need a text / audio-to-motion embedding this model does not have: they are left out."""

    def __init__(self):
        self.gen, self.ref = [], []

    def update(self, mu_gen, mu_ref) -> None:
        f = lambda x: np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, np.float64).reshape(-1, LATENT)
        g, r = f(mu_gen), f(mu_ref)
        if len(g) != len(r):
            raise ValueError(f"LatentMetrics.update: {len(g)} generated and {len(r)} reference latents")
        self.gen.append(g)
        self.ref.append(r)

    def arrays(self):
        z = np.zeros((0, LATENT))
        return (np.concatenate(self.gen) if self.gen else z), (np.concatenate(self.ref) if self.ref else z)

    def state(self) -> dict:
        g, r = self.arrays()
        return {"gen": g, "ref": r}

    def merge(self, other) -> "LatentMetrics":
        st = other.state() if isinstance(other, LatentMetrics) else other
        self.update(st["gen"], st["ref"])
        return self

    @property
    def n(self) -> int:
        return sum(len(g) for g in self.gen)

    def fid(self) -> float:
        g, r = self.arrays()
        if len(g) < 2:
            raise ValueError(f"LatentMetrics: FID needs at least 2 clips for a covariance, {len(g)} were evaluated")
        return frechet_distance(*moments(g), *moments(r))

    def compute(self, diversity_times: int = 300, seed: Optional[int] = None) -> dict:
        g, r = self.arrays()
        if not len(g) > diversity_times:      # the reference asserts num_samples > diversity_times
            raise ValueError(f"LatentMetrics.compute: Diversity draws {diversity_times} clips without replacement and needs more than that; {len(g)} were evaluated")
        rng = np.random.default_rng(seed)
        return {"FID": self.fid(), "Diversity": diversity(g, diversity_times, rng), "gt_Diversity": diversity(r, diversity_times, rng)}


class MotionMetrics:
    """The glue: (gen_motion, ref_motion, attr) - motions (B, 300, 168) = 55 x 3 axis-angle ++ translation, as trainer.metrics[...] holds them, attr the
    ld_attr rows [(actor, gender, ...)] - -> joints of both through the gendered BodyLosses engines -> joint_rows -> JointMetrics; mu of both through the
    engine's encode path (smplx_to_feats, amuse_vae_encode with eps = NULL) -> LatentMetrics."""

    def __init__(self, model, body_losses):
        if getattr(model, "diffusion_only", False) or getattr(getattr(model, "engine", None), "diffusion_only", False):
            raise ValueError("MotionMetrics: a diffusion_only setup has no motion prior, so there is no latent to take FID / Diversity on; use joint_rows / "
                             "JointMetrics for the joint half")
        if not getattr(body_losses, "engines", None):
            raise ValueError("MotionMetrics: the body models run on a GPU (BodyLosses built on a cuda device)")
        self.model, self.body = model, body_losses
        self.joint, self.latent = JointMetrics(), LatentMetrics()

    def joints(self, motion, subjects):
        """motion device float32 [B, F, 168] -> joints [B, F, 55, 3]: every gender's engine poses its own clips and leaves the others' rows alone"""
        import torch
        B, F = int(motion.shape[0]), int(motion.shape[1])
        rot, trans = motion[..., :NJ * 3].reshape(B, F, NJ, 3).contiguous(), motion[..., NJ * 3:].contiguous()
        out = torch.zeros(B, F, NJ, 3, device=motion.device)
        for i, g in enumerate(self.body.genders):
            j = self.body.engines[g].joints(rot, trans, subjects[i].contiguous(), "aa")
            out = torch.where((subjects[i] >= 0)[:, None, None, None], j, out)
        return out

    def latents(self, motion):
        import torch
        eng, B = self.model.engine, int(motion.shape[0])
        feats = eng.smplx_to_feats(motion[..., :NJ * 3].reshape(B, -1, NJ, 3).contiguous(), motion[..., NJ * 3:].contiguous())
        return eng.vae_encode(feats, None, getattr(self.model, "precision", "fp32x"), eps=None)["mu"]

    def update(self, gen_motion, ref_motion, attr, lengths=None) -> dict:
        import torch
        dev = self.body.device
        f = lambda m: torch.as_tensor(m).to(dev, torch.float32).contiguous()
        gen, ref = f(gen_motion), f(ref_motion)
        if gen.shape != ref.shape or gen.dim() != 3 or gen.shape[-1] != NJ * 3 + 3:
            raise ValueError(f"MotionMetrics.update: motions are two (B, F, 168) tensors, got {tuple(gen.shape)} and {tuple(ref.shape)}")
        B, F = int(gen.shape[0]), int(gen.shape[1])
        subjects = self.body.subjects(attr)
        ln = torch.full((B,), F, dtype=torch.int32, device=dev) if lengths is None else torch.as_tensor(lengths).to(dev, torch.int32).contiguous()
        rows = joint_rows(self.joints(gen, subjects), self.joints(ref, subjects), ln)
        mu_g, mu_r = self.latents(gen), self.latents(ref)
        self.joint.update(rows, ln)
        self.latent.update(mu_g, mu_r)
        return {"rows": rows, "mu_gen": mu_g, "mu_ref": mu_r}

    def state(self) -> dict:
        return {"joint": self.joint.state(), "latent": self.latent.state()}


# ------------------------------------------------------------------ the report
def _plain(v):
    if isinstance(v, np.ndarray):
        return [_plain(x) for x in v.tolist()]
    if isinstance(v, float) and not np.isfinite(v):
        return None
    return v


def summarize(state: dict, diversity_times: int = 300, seed: Optional[int] = 0) -> dict:
    """one task's (or the overall) additive state {"joint": ..., "latent": ...} -> the JSON entry: the computed values, count, count_seq; FID / Diversity are
    null with a reason when too few clips were evaluated"""
    jm = JointMetrics.from_state(state["joint"])
    lm = LatentMetrics().merge(state["latent"])
    out = {"count": jm.count, "count_seq": jm.count_seq}
    if jm.count_seq:
        out.update({k: _plain(v) for k, v in jm.compute().items()})
    out["latent_clips"] = lm.n
    for k in ("FID", "Diversity", "gt_Diversity"):
        out[k] = None
    try:
        out["FID"] = lm.fid()
    except ValueError as e:
        out["FID_reason"] = str(e)
    try:
        out.update(lm.compute(diversity_times, seed))
    except ValueError as e:
        out["Diversity_reason"] = str(e)
    return out


def merge_states(states) -> dict:
    jm, lm = JointMetrics(), LatentMetrics()
    for st in states:
        jm.merge(st["joint"])
        lm.merge(st["latent"])
    return {"joint": jm.state(), "latent": lm.state()}


def write_report(path, task_states: Dict[str, dict], precision: str, diversity_times: int = 300, seed: Optional[int] = 0) -> Path:
    """<model_path>/viz/motion_metrics_<stamp>_E<epoch>.json: per task and overall"""
    rep = {"precision": precision, "diversity_times": int(diversity_times), "fps": FPS,
           "tasks": {name: summarize(st, diversity_times, seed) for name, st in task_states.items()},
           "overall": summarize(merge_states(task_states.values()), diversity_times, seed)}
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(rep, indent=1, allow_nan=False))
    return path


# ------------------------------------------------------------------ two directories of NPZ files
def compare_directories(gen_dir, ref_dir, models: dict, device="cuda:0") -> dict:
    """The joint half for two directories of *_motion_smplx.npz matched by file name (the reference's own outputs included): each pair is one clip, posed by the
    body model of the reference file's gender with that file's betas.  Needs no checkpoint."""
    import torch
    from . import body, motion_file
    gen_dir, ref_dir = Path(gen_dir), Path(ref_dir)
    names = sorted(p.name for p in gen_dir.glob("*_motion_smplx.npz") if (ref_dir / p.name).is_file())
    if not names:
        raise SystemExit(f"motion_metrics: no *_motion_smplx.npz of {gen_dir} has a file of the same name in {ref_dir}")
    by_gender: Dict[str, list] = {}
    for n in names:
        r, g = motion_file.read(ref_dir / n), motion_file.read(gen_dir / n)
        if r.gender not in models:
            raise SystemExit(f"motion_metrics: {ref_dir / n} names the gender '{r.gender}'; the body models are {', '.join(models)}")
        if g.poses.shape != r.poses.shape:
            raise SystemExit(f"motion_metrics: {n}: {g.poses.shape[0]} generated and {r.poses.shape[0]} reference frames")
        by_gender.setdefault(r.gender, []).append((n, g, r))
    jm, per_file = JointMetrics(), {}
    with closing(body.Poser(models, device)) as poser:
        for gender, items in by_gender.items():
            eng = poser.engine(gender)
            for F in sorted({r.poses.shape[0] for _, _, r in items}):      # one call per clip length: a call's clips share F
                grp = [it for it in items if it[2].poses.shape[0] == F]
                eng.set_subjects(np.stack([body.fit_betas(r.betas, eng.model.n_betas) for _, _, r in grp]))      # one betas row per file: the reference file's
                sub = torch.arange(len(grp), dtype=torch.int32, device=device)
                t = lambda arrays: torch.from_numpy(np.stack(arrays)).to(device).contiguous()
                rows = joint_rows(eng.joints(t([g.poses for _, g, _ in grp]), t([g.trans for _, g, _ in grp]), sub, "aa"),
                                  eng.joints(t([r.poses for _, _, r in grp]), t([r.trans for _, _, r in grp]), sub, "aa"))
                jm.update(rows, [F] * len(grp))
                for (n, _, _), row in zip(grp, rows.cpu().numpy()):
                    one = JointMetrics()
                    one.update(row, [F])
                    per_file[n] = {k: _plain(v) for k, v in one.compute().items() if not k.endswith("_per_joint")}
    return {"files": len(names), "count": jm.count, "count_seq": jm.count_seq, **{k: _plain(v) for k, v in jm.compute().items()}, "per_file": per_file}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m amuse_amd.motion_metrics", description="APE / AVE / velocity / acceleration between two directories of *_motion_smplx.npz")
    ap.add_argument("gen_dir")
    ap.add_argument("ref_dir")
    ap.add_argument("--smplx-models", required=True, help="directory holding SMPLX_MALE.npz, SMPLX_FEMALE.npz, SMPLX_NEUTRAL.npz")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None, help="write the JSON here instead of printing it")
    args = ap.parse_args(argv)
    from . import body
    rep = compare_directories(args.gen_dir, args.ref_dir, body.require_models(args.smplx_models, "motion_metrics: "), args.device)
    text = json.dumps(rep, indent=1, allow_nan=False)
    if args.out:
        Path(args.out).write_text(text)
    else:
        print(text)
    return rep


if __name__ == "__main__":
    main()
