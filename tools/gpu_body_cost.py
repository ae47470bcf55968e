"""Cost of the SMPL-X body-model kernels on the GPU (csrc/k_body.hip) -> profiles/body_cost.txt.  HIP events, 20 calls per cell, precisions alternating:
  vertex_loss at the training shape (32 x 300 frames, three motion sets, synthetic V = 10,475 model) in fp32x and fp16, beside the pose-blend product's FLOPs
  forward, joints only, at 256 x 300 frames
  vertex_loss_grad (the skinning backward pass, csrc/k_body_bwd.hip) at the training shape, reference + one candidate, beside the two-set loss call of the same run
  train_gesture it/s with the vertex terms on, with them on AND carrying gradient (--vtex-grad), and without them, in the same job
usage: python tools/gpu_body_cost.py [out file]"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import body_cases as bc  # noqa: E402
from amuse_amd import body  # noqa: E402

DEV = "cuda:0"
PEAK16 = 2.5e15   # dense 16-bit MFMA peak of the MI355X (data sheet), FLOP/s


def timed(fn, n=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "body_cost.txt"
    lines = [f"tools/gpu_body_cost.py on {torch.cuda.get_device_name(0)}: HIP events, 20 calls per cell, precisions alternating; ms median (min)"]
    model = body.BodyModel.from_dict(bc.make_model(10475, seed=7))
    eng = body.BodyEngine(DEV, model)
    eng.set_subjects(bc.make_betas(4))
    N, F = 32, 300
    g = torch.Generator().manual_seed(0)
    rows = [(0.1 * torch.randn(N, F, 168, generator=g)).to(DEV) for _ in range(3)]
    sub = (torch.arange(N, dtype=torch.int32) % 4).to(DEV)
    res = torch.zeros(2, dtype=torch.float64, device=DEV)
    for p in ("fp32x", "fp16"):
        eng.vertex_loss(*rows, subject=sub, kind="aa", out=res, precision=p)   # warm-up: sizes the workspace
    torch.cuda.synchronize()
    t = {"fp32x": [], "fp16": []}
    for _ in range(20):
        for p in t:
            t[p].append(timed(lambda: eng.vertex_loss(*rows, subject=sub, kind="aa", out=res, precision=p), 1)[0])
    flop = 3 * N * F * 486 * 31425 * 2.0
    lines.append(f"vertex_loss  {N} x {F} frames x 3 sets, V = 10475 (synthetic model, skinning rows of 1..4 non-zeros + 3 dense; lists padded to {eng.info()['skin_nnz']}): "
                 f"pose-blend product {flop / 1e9:.0f} GFLOP per call (one product)")
    for p, k in (("fp32x", 3), ("fp16", 1)):
        a = np.array(t[p])
        lines.append(f"  {p:6s} {np.median(a):8.3f} ({a.min():.3f}) ms   {k} MFMA product(s): {k * flop / np.median(a) / 1e9:9.1f} TFLOP/s on the matrix cores = "
                     f"{100 * k * flop / (np.median(a) * 1e-3) / PEAK16:.1f} % of the 16-bit MFMA peak")
    # the realistic list length: the same model without dense rows
    eng2 = body.BodyEngine(DEV, body.BodyModel.from_dict(bc.make_model(10475, seed=7, dense_rows=0)))
    eng2.set_subjects(bc.make_betas(4))
    for p in ("fp32x", "fp16"):
        eng2.vertex_loss(*rows, subject=sub, kind="aa", out=res, precision=p)
    t = {"fp32x": [], "fp16": []}
    for _ in range(20):
        for p in t:
            t[p].append(timed(lambda: eng2.vertex_loss(*rows, subject=sub, kind="aa", out=res, precision=p), 1)[0])
    lines.append(f"the same without the dense rows (lists of {eng2.info()['skin_nnz']}):")
    for p, k in (("fp32x", 3), ("fp16", 1)):
        a = np.array(t[p])
        lines.append(f"  {p:6s} {np.median(a):8.3f} ({a.min():.3f}) ms   {100 * k * flop / (np.median(a) * 1e-3) / PEAK16:.1f} % of the 16-bit MFMA peak")
    # the gradient call: 6D feature rows, reference + one candidate (what the trainer's backward pass runs), beside the two-set loss call measured in the same loop
    rows6 = [(0.1 * torch.randn(N, F, 333, generator=g)).to(DEV) for _ in range(2)]
    for r in rows6:
        r[..., 0:330:6] += 1.0   # near-identity 6D rows: a1 ~ x, a2 ~ y
        r[..., 4:330:6] += 1.0
    gout = (torch.zeros(N, F, 333, device=DEV), None)
    for label, e in (("with the dense rows", eng), ("without the dense rows", eng2)):
        e.enable_grad()
        e.reserve(N * F)
        for p in ("fp32x", "fp16"):
            e.vertex_loss_grad(rows6[0], rows6[1], None, sub, out=gout, precision=p)
            e.vertex_loss(rows6[0], rows6[1], None, sub, "6d", out=res, precision=p)
        torch.cuda.synchronize()
        tg, tl = {"fp32x": [], "fp16": []}, {"fp32x": [], "fp16": []}
        for _ in range(20):
            for p in tg:
                tg[p].append(timed(lambda: e.vertex_loss_grad(rows6[0], rows6[1], None, sub, out=gout, precision=p), 1)[0])
                tl[p].append(timed(lambda: e.vertex_loss(rows6[0], rows6[1], None, sub, "6d", out=res, precision=p), 1)[0])
        lines.append(f"vertex_loss_grad  {N} x {F} frames, reference + 1 candidate, {label} (lists of {e.info()['skin_nnz']}); vertex_loss of the same two sets in the same loop:")
        for p in tg:
            a, b = np.array(tg[p]), np.array(tl[p])
            lines.append(f"  {p:6s} grad {np.median(a):8.3f} ({a.min():.3f}) ms   loss {np.median(b):8.3f} ({b.min():.3f}) ms   grad / loss = {np.median(a) / np.median(b):.2f}")
    eng2.close()
    N2 = 256
    rot, tr = (0.3 * torch.randn(N2, F, 55, 3, generator=g)).to(DEV), torch.randn(N2, F, 3, generator=g).to(DEV)
    sub2 = (torch.arange(N2, dtype=torch.int32) % 4).to(DEV)
    eng.joints(rot, tr, sub2)
    a = timed(lambda: eng.joints(rot, tr, sub2))
    lines.append(f"forward, joints only, {N2} x {F} frames: {np.median(a):.3f} ({a.min():.3f}) ms (includes the output allocation of the Python wrapper)")
    eng.close()
    # the training step with and without the terms (graphs on, batch 32, synthetic data)
    from amuse_amd.train_gesture import build_trainer, synthetic_batch
    models = {k: model for k in ("male", "female")}
    for label, with_body, vg in (("vertex terms ON ", True, False), ("vertex terms ON, --vtex-grad", True, True), ("vertex terms off", False, False)):
        bl = body.BodyLosses(models, DEV, "v0", grad=vg) if with_body else None
        trn = build_trainer(DEV, body=bl, vtex_grad=vg)
        batches = [dict(synthetic_batch(32, i, DEV), ld_attr=[("scott", "male"), ("miranda", "female")] * 16) for i in range(4)]
        for i in range(4):
            trn.train_step(batches[i])
        graphed = trn.enable_graph(batches[0])
        for i in range(3):
            trn.train_step(batches[i])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(20):
            trn.train_step(batches[i % 4])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 20
        ld = {k: round(float(v), 6) for k, v in trn.lpdm_losses.compute().items() if "vtex" in k}
        lines.append(f"train_gesture, batch 32, {'HIP graphs' if graphed else 'eager'}, {label}: {1 / dt:7.2f} it/s ({dt * 1e3:.2f} ms per step) {ld}")
        if bl is not None:
            bl.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
