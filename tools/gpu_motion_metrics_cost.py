"""Cost of the motion metrics on the GPU (csrc/k_motion_metrics.hip, amuse_amd/motion_metrics.py) -> profiles/motion_metrics_cost.txt.  256 clips x 300 frames,
HIP events around every call, 5 warm-up calls, 30 timed, the cells interleaved; ms median (min):
  amuse_motion_metrics alone, on joints already on the device
  the body forward (joints only) of the same clips, both motion sets, through the gendered engines (synthetic V = 10,475 models)
  the encode path of both sets (amuse_smplx_to_feats + amuse_vae_encode, mu only)
  the whole MotionMetrics.update call (the three above + the host copies of the rows and latents + the float64 accumulation)
usage: python tools/gpu_motion_metrics_cost.py [out file]"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import body_cases as bc  # noqa: E402
from amuse_amd import body, motion_metrics as mm, weights as wts  # noqa: E402
from amuse_amd.infer_ldm import PretrainedLPDM_v1  # noqa: E402

DEV = "cuda:0"
N, F, WARM, REPS = 256, 300, 5, 30


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "motion_metrics_cost.txt"
    models = {g: body.BodyModel.from_dict(bc.make_model(10475, seed=7 + i, dense_rows=0)) for i, g in enumerate(("male", "female"))}
    bl = body.BodyLosses(models, DEV)
    model = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV, seed=2024)
    model.precision = "fp32x"
    g = torch.Generator().manual_seed(0)
    gen, ref = ((0.3 * torch.randn(N, F, 168, generator=g)).to(DEV) for _ in range(2))
    attr = [("scott", "male"), ("miranda", "female")] * (N // 2)
    ev = mm.MotionMetrics(model, bl)
    sub = bl.subjects(attr)
    jg, jr = ev.joints(gen, sub), ev.joints(ref, sub)
    ln = torch.full((N,), F, dtype=torch.int32, device=DEV)
    cells = {"amuse_motion_metrics": lambda: mm.joint_rows(jg, jr, ln),
             "body forward, joints only, both sets": lambda: (ev.joints(gen, sub), ev.joints(ref, sub)),
             "encode (smplx_to_feats + vae_encode, mu), both sets": lambda: (ev.latents(gen), ev.latents(ref)),
             "MotionMetrics.update (all of it, host copies included)": lambda: mm.MotionMetrics(model, bl).update(gen, ref, attr)}
    for fn in cells.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in cells}
    for _ in range(REPS):
        for k, fn in cells.items():
            t[k].append(once(fn))
    lines = [f"tools/gpu_motion_metrics_cost.py on {torch.cuda.get_device_name(0)}: {N} clips x {F} frames, HIP events, {WARM} warm-up + {REPS} timed calls per cell, "
             f"cells interleaved; ms median (min); sampler / encode precision fp32x; body models synthetic, V = 10475",
             f"(amuse_motion_metrics reads 2 sets x {N * F * 165 * 4 / 1e6:.1f} MB twice - the second pass through L2 - and writes {N * 442 * 8 / 1e3:.0f} KB; the timed "
             f"wrapper call includes its torch.empty of the rows)"]
    for k, v in t.items():
        a = np.array(v)
        lines.append(f"  {k:58s} {np.median(a):8.3f} ({a.min():.3f}) ms")
    km, fw = np.median(t["amuse_motion_metrics"]), np.median(t["body forward, joints only, both sets"])
    lines.append(f"amuse_motion_metrics / body forward of the same clips = {km / fw:.2f}")
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    bl.close()
    model.engine.close()


if __name__ == "__main__":
    main()
