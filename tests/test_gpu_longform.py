"""GPU: long-form inference - the join kernel (csrc/k_stitch.hip through amuse_amd/longform.py) against tests/stitch_ref.py's float64 restatement, and the path
built on it (PretrainedLPDM_v1.infer_long, the trainer's long-form jobs, the command line).

Bars.  Per blended joint the measure is the geodesic angle between the GPU's rotation and the float64 restatement's.  The bar is the project's rule for the body
model: max(4 x the float32 restatement's largest distance from the float64 one ON THE TEST'S OWN INPUTS, 2^-20 rad) - i.e. fp32 arithmetic in another order may be
four times worse than fp32 arithmetic in numpy's order, nothing more (the float32 restatement sits at 4.6e-7 .. 9.5e-7 rad on these cases, the kernel on an MI355X at 6.4e-7 .. 8.8e-7).  The
axis-angle VECTOR is compared too, on joints whose reference angle is below pi - 0.1 (beyond, the short representation's sign is a coin toss): a rotation error
of delta moves the rotation vector by at most delta x (theta / 2) / sin(theta / 2), the largest singular value of the exponential map's inverse Jacobian at angle
theta, so that is the bar's scale.  Translation: 4 ulp (fp32) of the larger input - (1 - w) a + w b is two roundings and an fma at most.  Frames outside the
overlaps are the input rows' bits.

Inputs: joint classes mixed in one tensor by joint index - independent random rotations up to 3.6 rad (beyond pi occurs), a == b, b = a + 1e-4 and + 1e-2 noise,
b the 2 pi - theta alias of a, both below 1e-6 rad.  Pairs with |q_a . q_b| < 1e-3 are redrawn: there the choice of hemisphere is a coin toss between any two
arithmetics (a choice of inputs, not an exclusion of results)."""
import functools
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import stitch_ref as sr

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"
CAP = 32      # sequences per launch (csrc/amuse_stitch_host.hpp kStitchMaxSeq; include/amuse_hip.h states it)

# (F, hop, windows, frames, with translation)
CASES = {
    "two_sequences": (12, 9, (3, 1), (30, 12), True),
    "capacity_plus_one": (4, 2, tuple(1 + s % 3 for s in range(CAP + 1)), tuple((s % 3) * 2 + 4 - (s % 2) * (s % 3 > 0) for s in range(CAP + 1)), True),
    "cut_short": (12, 9, (3, 2, 4), (25, 10, 28), True),          # L short of (W - 1) hop + F; L = (W - 1) hop + 1 twice
    "poses_only": (12, 9, (2,), (21,), False),
    "product_hop270": (300, 270, (2,), (570,), True),
    "product_hop150": (300, 150, (3,), (600,), True),             # the largest overlap: every frame past the first 150 has two windows
}


def _rand_aa(rng, shape, max_angle):
    ax = rng.standard_normal(shape + (3,))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    return ax * rng.uniform(0, max_angle, shape + (1,))


def _make(F, hop, windows, frames, seed):
    """float32 windows whose overlapping rows pair up as the joint classes ask (class = joint index mod 6)"""
    rng = np.random.default_rng(seed)
    nw = sum(windows)
    poses = _rand_aa(rng, (nw, F, 55), 3.6)
    O = F - hop
    cls = np.arange(55) % 6
    w0 = 0
    for W in windows:
        for k in range(1, W):
            a = poses[w0 + k - 1, hop:hop + O]                     # window k - 1's rows i + hop ...
            b = poses[w0 + k, :O]                                  # ... and window k's rows i: the same frames
            for _ in range(100):                                   # class 0: independent draws, no coin-toss hemispheres
                d = np.abs((sr.aa_to_quat(a.astype(np.float32)) * sr.aa_to_quat(b.astype(np.float32))).sum(-1))
                bad = (d < 1e-3) & (cls == 0)
                if not bad.any():
                    break
                b[bad] = _rand_aa(rng, (int(bad.sum()),), 3.6)
            assert not bad.any()
            b[:, cls == 1] = a[:, cls == 1]
            b[:, cls == 2] = a[:, cls == 2] + 1e-4 * rng.standard_normal(a[:, cls == 2].shape)
            b[:, cls == 3] = a[:, cls == 3] + 1e-2 * rng.standard_normal(a[:, cls == 3].shape)
            th = np.linalg.norm(a[:, cls == 4], axis=-1, keepdims=True)
            b[:, cls == 4] = -(a[:, cls == 4] / th) * (2 * np.pi - th)
            a[:, cls == 5] = 5e-7 * rng.uniform(-1, 1, a[:, cls == 5].shape)
            b[:, cls == 5] = 5e-7 * rng.uniform(-1, 1, a[:, cls == 5].shape)
            if O:
                a[0, 5], b[0, 11] = 0.0, 0.0                       # exact zeros: one side, then (joint 17 below) both
                a[0, 17], b[0, 17] = 0.0, 0.0
        w0 += W
    trans = rng.standard_normal((nw, F, 3)) * np.array([1.0, 0.1, 30.0])
    return poses.astype(np.float32), trans.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs, both restatements and the bar of a case, computed once and shared (read-only)"""
    F, hop, windows, frames, with_trans = CASES[name]
    assert all((W - 1) * hop < L <= (W - 1) * hop + F for W, L in zip(windows, frames)), name
    poses, trans = _make(F, hop, windows, frames, seed=sum(map(ord, name)))
    if not with_trans:
        trans = None
    blend = sr.blend_weights(F - hop)
    p64, t64, mask = sr.join(poses, trans, windows, frames, hop, blend)
    p32, _, _ = sr.join(poses, trans, windows, frames, hop, blend, np.float32)
    f32_dist = float(sr.geodesic(p32[mask], p64[mask]).max()) if mask.any() else 0.0
    out = dict(F=F, hop=hop, windows=windows, frames=frames, poses=poses, trans=trans, blend=blend, p64=p64, t64=t64, mask=mask, f32_dist=f32_dist,
               bar=max(4.0 * f32_dist, 2.0 ** -20))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _run(c, poses=None, trans=None):
    from amuse_amd import longform
    p = torch.tensor(c["poses"] if poses is None else poses, device=DEV)       # (torch.tensor copies: the shared case stays read-only)
    t = c["trans"] if trans is None else trans
    t = None if t is None else torch.tensor(t, device=DEV)
    po, to = longform.stitch(p, t, c["windows"], c["frames"], c["hop"], F=c["F"], blend=torch.tensor(c["blend"]))
    torch.cuda.synchronize()
    return po.cpu().numpy(), None if to is None else to.cpu().numpy()


def _rows(c):
    """(output frame, window, row) of every frame outside the overlaps"""
    out, w0, f0 = [], 0, 0
    for W, L in zip(c["windows"], c["frames"]):
        for f in range(L):
            k = min(f // c["hop"], W - 1)
            if not c["mask"][f0 + f]:
                out.append((f0 + f, w0 + k, f - k * c["hop"]))
        w0, f0 = w0 + W, f0 + L
    return np.array(out).T


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64_restatement(name):
    c = _case(name)
    po, to = _run(c)
    assert po.shape == c["p64"].shape and po.dtype == np.float32 and np.isfinite(po).all()
    mask = c["mask"]
    assert mask.any() and (~mask).any()
    # frames only one window produced: the input rows, bit for bit (angles beyond pi included: nothing is normalised there)
    fo, wi, ri = _rows(c)
    assert np.array_equal(po[fo].view(np.uint32), c["poses"][wi, ri].view(np.uint32))
    assert np.linalg.norm(po[fo], axis=-1).max() > np.pi
    # blended frames
    g = sr.geodesic(po[mask], c["p64"][mask])
    print(f"{name}: blended joints {g.size}, geodesic max {g.max():.3e} rad (float32 restatement {c['f32_dist']:.3e}, bar {c['bar']:.3e})")
    assert g.max() <= c["bar"], (float(g.max()), c["bar"])
    assert np.linalg.norm(po[mask], axis=-1).max() <= np.pi + 1e-6          # blended rows carry the short representation
    th = np.linalg.norm(c["p64"][mask], axis=-1)
    sel = th < np.pi - 0.1
    half = np.maximum(0.5 * th[sel], 1e-12)
    scale = np.where(th[sel] < 1e-6, 1.0, half / np.sin(half))
    dv = np.linalg.norm(po[mask][sel].astype(np.float64) - c["p64"][mask][sel], axis=-1)
    print(f"{name}: axis-angle vectors compared {int(sel.sum())} of {sel.size}, worst error / (bar x scale) {float((dv / (c['bar'] * scale)).max()):.3f}")
    assert sel.sum() > 0.5 * sel.size and (dv <= c["bar"] * scale).all()
    if c["trans"] is None:
        assert to is None
        return
    assert np.array_equal(to[fo].view(np.uint32), c["trans"][wi, ri].view(np.uint32))
    # 4 ulp of the larger input
    fb = np.nonzero(mask)[0]
    big = np.zeros((fb.size, 3), np.float32)
    w0 = f0 = 0
    n = 0
    for W, L in zip(c["windows"], c["frames"]):
        for f in range(L):
            if mask[f0 + f]:
                k = min(f // c["hop"], W - 1)
                i = f - k * c["hop"]
                big[n] = np.maximum(np.abs(c["trans"][w0 + k - 1, i + c["hop"]]), np.abs(c["trans"][w0 + k, i]))
                n += 1
        w0, f0 = w0 + W, f0 + L
    terr = np.abs(to[mask].astype(np.float64) - c["t64"][mask]) / np.spacing(big).astype(np.float64)
    print(f"{name}: translation worst error {terr.max():.2f} ulp of the larger input (bar 4)")
    assert terr.max() <= 4.0


def test_every_class_and_branch_is_reached():
    """the inputs do what the docstring says: every joint class sits in blended rows, angles beyond pi and below 1e-6 occur, aliases are the same rotation,
    both the slerp and its linear limit are taken, and the hemisphere flip happens"""
    c = _case("two_sequences")
    F, hop = c["F"], c["hop"]
    a, b = c["poses"][0, hop:], c["poses"][1, :F - hop]
    qa, qb = sr.aa_to_quat(a), sr.aa_to_quat(b)
    d = (qa * qb).sum(-1)
    om = np.arctan2(np.linalg.norm(np.where(d[..., None] < 0, -qb, qb) - np.abs(d)[..., None] * qa, axis=-1), np.abs(d))
    cls = np.arange(55) % 6
    assert (np.abs(d[:, cls == 0]) >= 1e-3).all() and (d < 0).any() and (d > 0).any()
    assert np.array_equal(a[:, cls == 1], b[:, cls == 1]) and (np.sin(om[:, cls == 1]) < 1e-4).all()            # the linear limit
    assert (np.sin(om[:, cls == 3]) >= 1e-4).any() and (np.sin(om[:, cls == 0]) >= 1e-4).all()                  # the slerp
    assert sr.geodesic(a[:, cls == 4], b[:, cls == 4]).max() < 1e-5 and (d[:, cls == 4] < 0).all()              # the alias: the same rotation, the other hemisphere
    assert (np.linalg.norm(a[:, cls == 5], axis=-1) < 1e-6).all() and not a[0, 17].any() and not b[0, 17].any()
    assert (np.linalg.norm(c["poses"], axis=-1) > np.pi).any()
    assert len(CASES["capacity_plus_one"][2]) == CAP + 1


def test_hop_equal_to_window_is_concatenation():
    from amuse_amd import longform
    rng = np.random.default_rng(9)
    poses, trans = _rand_aa(rng, (3, 300, 55), 3.6).astype(np.float32), rng.standard_normal((3, 300, 3)).astype(np.float32)
    po, to = longform.stitch(torch.from_numpy(poses).to(DEV), torch.from_numpy(trans).to(DEV), [2, 1], [600, 300], 300)
    assert np.array_equal(po.cpu().numpy().view(np.uint32), poses.reshape(900, 55, 3).view(np.uint32))
    assert np.array_equal(to.cpu().numpy().view(np.uint32), trans.reshape(900, 3).view(np.uint32))
    po, _ = longform.stitch(torch.from_numpy(poses).to(DEV), None, [2, 1], [301, 300], 300)          # one frame of the second window
    assert np.array_equal(po.cpu().numpy(), np.concatenate([poses[0], poses[1, :1], poses[2]]))


def test_repeat_calls_and_graph_replay():
    from amuse_amd import longform
    c = _case("cut_short")
    p, t, blend = (torch.tensor(c[k], device=DEV) for k in ("poses", "trans", "blend"))
    call = lambda: longform.stitch(p, t, c["windows"], c["frames"], c["hop"], F=c["F"], blend=blend)
    e1, e2 = call(), call()
    torch.cuda.synchronize()
    assert torch.equal(e1[0], e2[0]) and torch.equal(e1[1], e2[1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                # one linear branch: the entry point allocates nothing and copies nothing
        gp, gt = call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gp, e1[0]) and torch.equal(gt, e1[1])
    # the captured call follows overwritten inputs
    p2, t2 = _make(c["F"], c["hop"], c["windows"], c["frames"], seed=77)
    p.copy_(torch.from_numpy(p2))
    t.copy_(torch.from_numpy(t2))
    g.replay()
    torch.cuda.synchronize()
    e3 = call()
    torch.cuda.synchronize()
    assert torch.equal(gp, e3[0]) and torch.equal(gt, e3[1]) and not torch.equal(gp, e1[0])


# ------------------------------------------------------------------ the path built on the kernel
@pytest.fixture(scope="module")
def model():
    from amuse_amd import audio_weights as aw
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))     # random-init front-end, as tests/test_gpu_audio.py builds its engine
    m.precision = "fp32x"
    yield m
    m.audio_engine.close()
    m.engine.close()


def _wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    return (0.2 * torch.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 0.3 * t)) + 0.05 * torch.randn(n, generator=g) + 0.01)[None]


def test_infer_long_is_windows_plus_stitch(model):
    from amuse_amd import longform
    long_w, short_w = _wave(400000, 1), _wave(160000, 2)
    model._clip_counter = 7
    out = model.infer_long([long_w, short_w])
    assert model._clip_counter == 11 and len(out) == 2
    assert out[0]["poses"].shape == (750, 55, 3) and out[0]["trans"].shape == (750, 3) and out[1]["poses"].shape == (300, 55, 3)
    # the three windows, run explicitly at the same clip indices
    a = long_w - long_w.mean()
    chunks = [a[:, s:e] for s, e in longform.window_slices(400000, 270)]
    assert [c.shape[1] for c in chunks] == [160000, 160000, 112000]
    embs = model.process_seq_list(chunks, framerate=16000)
    con, emo, sty = (torch.cat([e[i] for e in embs]) for i in range(3))
    ob = model.diffusion_backward(3, con, emo, sty, clip_index0=7)
    for key in ("poses", "trans"):
        o, w = out[0][key], ob[key]
        assert torch.equal(o[:270], w[0, :270]) and torch.equal(o[300:540], w[1, 30:270]) and torch.equal(o[570:], w[2, 30:210])     # outside the overlaps
        assert not torch.equal(o[270:300], w[0, 270:]) and not torch.equal(o[270:300], w[1, :30])
    sp, st = longform.stitch(ob["poses"], ob["trans"], [3], [750], 270)
    assert torch.equal(sp, out[0]["poses"]) and torch.equal(st, out[0]["trans"])                                                     # the overlaps: the stitch of those rows
    assert not torch.equal(ob["poses"][0], ob["poses"][1])
    # a 10 s waveform: the single-clip path, bit for bit
    e1 = model.process_single_seq(short_w - short_w.mean(), framerate=16000)
    o1 = model.diffusion_backward(1, *e1, clip_index0=10)
    assert torch.equal(out[1]["poses"], o1["poses"][0]) and torch.equal(out[1]["trans"], o1["trans"][0])


def _tree(tmp_path, name="tree"):
    from conftest import make_reference_tree
    from scipy.io import wavfile
    root = make_reference_tree(tmp_path / name, n_infer_wavs=2)
    wavfile.write(root / "viz_dump/test/speech/scott_9_long.wav", 16000, (_wave(400000, 3)[0].numpy() * 20000).astype(np.int16))   # sorts after the two 10 s files
    return root


def test_trainer_long_form_jobs_and_default_bytes(model, tmp_path):
    """in process, on one model: with long_form on, the 25 s WAV becomes one NPZ of 750 frames and the 10 s WAVs give the bytes they give with it off"""
    from amuse_amd import main as cli
    from amuse_amd.trainer import trainer
    root = _tree(tmp_path)
    config, _ = cli.load_config(root, "infer_gesture", None)

    def run(long_form, stamp):
        config["TRAIN_PARAM"]["test"]["long_form"] = long_form
        model._clip_counter = 0
        random.seed(5)
        tr = trainer(config, torch.device(DEV), model=model, stamp=stamp)
        return tr.eval_prior_latdiff_forward_backward_v1(False, 0, True, False, modelversion="full", ammetric=True)
    off, on = run(False, "off"), run(True, "on")
    assert [p.name for p in off] == [p.name for p in on] and len(off) == 3
    assert off[0].read_bytes() == on[0].read_bytes() and off[1].read_bytes() == on[1].read_bytes()
    with np.load(off[2]) as z0, np.load(on[2]) as z1:
        assert z0["poses"].shape == (300, 55, 3) and z1["poses"].shape == (750, 55, 3) and z1["trans"].shape == (750, 3)
        assert np.isfinite(z1["poses"]).all() and np.abs(np.diff(z1["poses"][:, 12:], axis=0)).max() > 0


def test_cli_long_form_writes_750_frames(tmp_path):
    root = _tree(tmp_path)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "AMUSE_RUN_STAMP")}
    env.update(AMUSE_RUN_STAMP="20260101-000000")
    r = subprocess.run([sys.executable, "-m", "amuse_amd.main", "--fn", "infer_gesture", "--root", str(root), "--random-init", "--long-form"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    files = sorted((root / "viz_dump/test/gesture").rglob("*.npz"))
    shapes = sorted(np.load(p)["poses"].shape for p in files)
    assert shapes == [(300, 55, 3), (300, 55, 3), (750, 55, 3)], shapes
