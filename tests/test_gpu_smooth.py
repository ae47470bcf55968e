"""GPU: motion smoothing - the kernel (csrc/k_smooth.hip through amuse_amd/smooth.py) against tests/smooth_ref.py's float64 restatement on the seeded cases of
tests/smooth_cases.py, its bitwise invariances, and the paths built on it (trainer.run_jobs, the trainer's NPZ files, python -m amuse_amd.smooth).

Bars.  Per filtered joint the measure is the geodesic angle between the GPU's rotation and the float64 restatement's; the bar is the project's rule for the
stitch and the body model: max(4 x the float32 restatement's largest distance from the float64 one ON THE TEST'S OWN INPUTS, 2^-20 rad).  Translation: max(4 x
the float32 restatement's distance, 2^-20 x max|x|).  The cubic-angle known answer is held against the ANALYTIC rotations under the same rule (the float32
restatement's distance from them).  Measured on an MI355X: 8.2e-7 rad on the mixed case (float32 restatement 7.4e-7, bar 3.0e-6), 7.1e-7 rad from the analytic cubic
(6.1e-7, bar 2.4e-6), translation 1.4e-7 (1.5e-7, bar 9.7e-7).  Slots that are not filtered (m = 0, sequences shorter than the window) are the input's bits; so is everything else that is
claimed bitwise below."""
import ctypes as C
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import smooth_cases as cases
import smooth_ref as ref

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"
OPTS = {"window": 9, "order": 3}


def _run(c, poses=None, trans="case", frames=None):
    from amuse_amd import smooth
    p = torch.tensor(c["poses"] if poses is None else poses, device=DEV)       # (torch.tensor copies: the shared case stays read-only)
    t = c["trans"] if isinstance(trans, str) else trans
    t = None if t is None else torch.tensor(t, device=DEV)
    po, to = smooth.smooth(p, t, c["frames"] if frames is None else frames, order=c["order"], half_window=c["hw"])
    torch.cuda.synchronize()
    return po.cpu().numpy(), None if to is None else to.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_kernel_against_float64_restatement():
    c = cases.mixed()
    po, to = _run(c)
    assert po.shape == c["p64"].shape and po.dtype == np.float32 and np.isfinite(po).all() and np.isfinite(to).all()
    mj, mt = c["mask"][:, :55], c["mask"][:, 55]
    # m_j = 0 and sequences shorter than the window: the input's bits (angles beyond pi included)
    assert np.array_equal(_bits(po[~mj]), _bits(c["poses"][~mj])) and np.array_equal(_bits(to[~mt]), _bits(c["trans"][~mt]))
    assert np.linalg.norm(po[~mj], axis=-1).max() > np.pi and np.linalg.norm(po[mj], axis=-1).max() <= np.pi + 1e-6
    g = ref.geodesic(po[mj], c["p64"][mj])
    print(f"mixed: filtered joints {g.size}, geodesic max {g.max():.3e} rad (float32 restatement {c['f32_dist']:.3e}, bar {c['bar']:.3e})")
    terr = np.abs(to[mt].astype(np.float64) - c["t64"][mt])
    print(f"mixed: translation worst error {terr.max():.3e} (float32 restatement {c['t32_dist']:.3e}, bar {c['tbar']:.3e})")
    assert g.max() <= c["bar"], (float(g.max()), c["bar"])
    assert terr.max() <= c["tbar"], (float(terr.max()), c["tbar"])


def test_cubic_angle_known_answer():
    c = cases.cubic()
    po, to = _run(c)
    assert to is None
    g = ref.geodesic(po, c["exact"])
    print(f"cubic: geodesic max {g.max():.3e} rad from the analytic rotations (float32 restatement {c['f32_dist_exact']:.3e}, bar {c['bar_exact']:.3e})")
    assert g.max() <= c["bar_exact"], (float(g.max()), c["bar_exact"])
    assert ref.geodesic(po, c["p64"]).max() <= c["bar"]


def test_noisy_motion_comes_out_smoother_and_closer():
    c = cases.noisy()
    po, _ = _run(c)
    (j_in, j_out), (d_in, d_out) = cases.noisy_inequalities(c, po)
    print(f"noisy: mean geodesic second difference {j_in:.4f} -> {j_out:.4f}; distance from the clean motion {d_in:.4f} -> {d_out:.4f}")
    assert j_out < j_in and d_out < d_in
    assert ref.geodesic(po, c["p64"]).max() <= c["bar"]


def test_guard_rows_trans_absent_and_refusals():
    """the entry point itself, on caller-owned buffers: rows before and after both outputs stay untouched; trans / trans_out NULL together; in place refused"""
    from amuse_amd import _lib, smooth
    c = cases.mixed()
    lib, G, total, S = _lib.load(), 3, c["poses"].shape[0], len(c["frames"])
    p, t, bk = torch.tensor(c["poses"], device=DEV), torch.tensor(c["trans"], device=DEV), torch.tensor(smooth.banks(c["order"]), device=DEV)
    fill = float(np.float32(-123.25))
    pbig, tbig = torch.full((total + 2 * G, 55, 3), fill, device=DEV), torch.full((total + 2 * G, 3), fill, device=DEV)
    fr, hw = (C.c_int * S)(*c["frames"]), (C.c_ubyte * 56)(*c["hw"])
    vp = lambda x: C.c_void_p(x.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    assert lib.amuse_smooth_motion(vp(p), vp(t), S, fr, hw, vp(bk), vp(pbig[G:]), vp(tbig[G:]), st) == 0
    torch.cuda.synchronize()
    ref_p, ref_t = _run(c)
    assert np.array_equal(_bits(pbig[G:G + total].cpu().numpy()), _bits(ref_p)) and np.array_equal(_bits(tbig[G:G + total].cpu().numpy()), _bits(ref_t))
    for big in (pbig, tbig):
        assert bool((big[:G] == fill).all()) and bool((big[G + total:] == fill).all())
    # poses only: the same pose bits, the translation buffer is not touched
    pbig.fill_(fill)
    tbig.fill_(fill)
    assert lib.amuse_smooth_motion(vp(p), None, S, fr, hw, vp(bk), vp(pbig[G:]), None, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pbig[G:G + total].cpu().numpy()), _bits(ref_p)) and bool((tbig == fill).all()) and bool((pbig[:G] == fill).all())
    po, to = _run(c, trans=None)
    assert to is None and np.array_equal(_bits(po), _bits(ref_p))
    # refused before any launch
    assert lib.amuse_smooth_motion(vp(p), vp(t), S, fr, hw, vp(bk), vp(pbig[G:]), None, st) != 0
    assert lib.amuse_smooth_motion(vp(p), vp(t), S, fr, hw, vp(bk), vp(p), vp(tbig[G:]), st) != 0 and b"overlap" in lib.amuse_last_error()
    torch.cuda.synchronize()
    assert bool((pbig[:G] == fill).all())


def test_repeat_batch_position_and_graph_replay():
    from amuse_amd import smooth
    c = cases.mixed()
    a, b = _run(c), _run(c)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    # a sequence alone == its rows among the 33 (it sits in the second launch there, and first in its own call)
    offs = np.concatenate([[0], np.cumsum(c["frames"])])
    for s in (0, 14, 32):
        sl = slice(offs[s], offs[s + 1])
        po, to = _run(c, poses=c["poses"][sl], trans=c["trans"][sl], frames=[c["frames"][s]])
        assert np.array_equal(_bits(po), _bits(a[0][sl])) and np.array_equal(_bits(to), _bits(a[1][sl])), s
    # a captured call replayed on overwritten inputs == eager
    p, t = torch.tensor(c["poses"], device=DEV), torch.tensor(c["trans"], device=DEV)
    call = lambda: smooth.smooth(p, t, c["frames"], order=c["order"], half_window=c["hw"])
    call()                                   # (the bank of this order is on the device before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                # one linear branch: the entry point allocates nothing and copies nothing
        gp, gt = call()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gp.cpu().numpy()), _bits(a[0])) and np.array_equal(_bits(gt.cpu().numpy()), _bits(a[1]))
    perm = torch.arange(55, device=DEV).roll(6)        # joints moved by a whole period of the half-window pattern: other data, the same classes per m
    p.copy_(p[:, perm] * 0.9)
    t.mul_(1.5)
    g.replay()
    torch.cuda.synchronize()
    e = call()
    torch.cuda.synchronize()
    assert torch.equal(gp, e[0]) and torch.equal(gt, e[1]) and not np.array_equal(gp.cpu().numpy(), a[0])


@pytest.mark.parametrize("cut", [1, 7, cases.TILE - 1, cases.TILE + 1])
def test_tile_position_is_invisible(cut):
    """a sequence and the same sequence with its first `cut` frames cut off agree, bit for bit, on every frame that is interior in both: the cut moves every
    frame to another place in its tile (and, past a tile, to another tile)"""
    c = cases.mixed()
    s = 14
    L = c["frames"][s]
    assert L == 100 and L > 3 * cases.TILE
    f0 = int(np.sum(c["frames"][:s]))
    poses, trans = c["poses"][f0:f0 + L], c["trans"][f0:f0 + L]
    whole = _run(c, poses=poses, trans=trans, frames=[L])
    part = _run(c, poses=poses[cut:], trans=trans[cut:], frames=[L - cut])
    M = max(c["hw"])
    lo, hi = cut + M, L - M                      # frames whose window is centred in both sequences, for every half-window of the case
    assert hi - lo > cases.TILE
    assert np.array_equal(_bits(whole[0][lo:hi]), _bits(part[0][lo - cut:hi - cut])) and np.array_equal(_bits(whole[1][lo:hi]), _bits(part[1][lo - cut:hi - cut]))
    assert not np.array_equal(whole[0][cut:cut + 1], part[0][:1])          # the first frame of the cut sequence is an edge frame there: another window


# ------------------------------------------------------------------ the paths built on the kernel
@pytest.fixture(scope="module")
def model():
    from amuse_amd import audio_weights as aw
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))     # random-init front-end, as tests/test_gpu_longform.py builds its model
    m.precision = "fp32x"
    yield m
    m.audio_engine.close()
    m.engine.close()


def test_run_jobs_smooth_is_run_jobs_then_smooth(model):
    """a plain job (two clips) and a long-form job (two windows joined into 570 frames): bitwise"""
    from amuse_amd import smooth
    from amuse_amd.trainer import _job, run_jobs
    gen = torch.Generator().manual_seed(2)
    z = lambda n: torch.randn(n, 256, generator=gen)
    jobs = [_job("scott", "0_65_65", z(2), z(2), z(2), 2, "scott a"),
            _job("scott", "long", z(2), z(2), z(2), 2, "scott b", None, None, None, long_form={"frames": 570, "hop": 270})]
    model._clip_counter = 3
    raw = run_jobs(model, jobs)
    model._clip_counter = 3
    sm = run_jobs(model, jobs, smooth=dict(OPTS, hands_window=5))
    assert [tuple(r["feats"].shape) for r in raw] == [(2, 300, 168), (1, 570, 168)] == [tuple(r["feats"].shape) for r in sm]
    for r, q in zip(raw, sm):
        B, L = r["feats"].shape[:2]
        po, to = smooth.smooth(r["feats"][..., :165].reshape(B * L, 55, 3), r["feats"][..., 165:].reshape(B * L, 3), [L] * B, 9, 3, hands_window=5)
        assert torch.equal(q["feats"][..., :165].reshape(B * L, 55, 3), po) and torch.equal(q["feats"][..., 165:].reshape(B * L, 3), to)
        assert not torch.equal(q["feats"], r["feats"])
    # infer_long the same way
    wave = (0.2 * torch.sin(2 * np.pi * 220.0 * torch.arange(200000) / 16000.0))[None]
    model._clip_counter = 0
    a = model.infer_long([wave])
    model._clip_counter = 0
    b = model.infer_long([wave], smooth=OPTS)
    po, to = smooth.smooth(a[0]["poses"], a[0]["trans"], [a[0]["poses"].shape[0]])
    assert torch.equal(b[0]["poses"], po) and torch.equal(b[0]["trans"], to) and not torch.equal(po, a[0]["poses"])


def test_trainer_bytes_without_the_switch_and_the_npz_tool(model, tmp_path, monkeypatch):
    """in process, on one model: without TRAIN_PARAM.test.smooth the NPZ bytes are those of a run whose hook cannot run at all; with it, the files hold the
    smoothed motion - and python -m amuse_amd.smooth on the unsmoothed files gives the same rows for every joint outside the lower-body lock"""
    from conftest import make_reference_tree
    from amuse_amd import main as cli
    from amuse_amd import smooth
    from amuse_amd.npz_writer import LOWER_BODY_JOINTS
    from amuse_amd.trainer import trainer
    root = make_reference_tree(tmp_path / "tree", n_infer_wavs=2)
    config, _ = cli.load_config(root, "infer_gesture", None)

    def run(opts, stamp):
        config["TRAIN_PARAM"]["test"].pop("smooth", None)
        if opts is not None:
            config["TRAIN_PARAM"]["test"]["smooth"] = opts
        model._clip_counter = 0
        random.seed(5)
        tr = trainer(config, torch.device(DEV), model=model, stamp=stamp)
        return tr.eval_prior_latdiff_forward_backward_v1(False, 0, True, False, modelversion="full", ammetric=True)
    off = run(None, "off")
    with monkeypatch.context() as mp:            # the hook bypassed: a run in which calling the filter is an error
        def never(*a, **k):
            raise AssertionError("the smoothing hook ran without the switch")
        mp.setattr(smooth, "smooth_batch", never)
        mp.setattr(smooth, "smooth", never)
        bypass = run(None, "bypass")
    on = run(dict(OPTS), "on")
    assert [p.name for p in off] == [p.name for p in bypass] == [p.name for p in on] and len(off) == 2
    assert all(a.read_bytes() == b.read_bytes() for a, b in zip(off, bypass))
    assert all(a.read_bytes() != b.read_bytes() for a, b in zip(off, on))
    # the tool on the unsmoothed files
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "amuse_amd.smooth", *map(str, off), "-o", str(tmp_path / "sm"), "--window", "9", "--order", "3"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    free = [j for j in range(55) if j not in LOWER_BODY_JOINTS]
    for src, want in zip(off, on):
        got = tmp_path / "sm" / src.name.replace("_motion_smplx.npz", "_smoothed_motion_smplx.npz")
        with np.load(got) as zg, np.load(want) as zw, np.load(src) as zs:
            assert zg["poses"].shape == (300, 55, 3) and zg["poses"].dtype == np.float32
            assert np.array_equal(_bits(zg["poses"][:, free]), _bits(zw["poses"][:, free])) and not np.array_equal(zg["poses"][:, free], zs["poses"][:, free])
            assert (zg["poses"][:, LOWER_BODY_JOINTS] == zg["poses"][0, LOWER_BODY_JOINTS]).all() and not zg["trans"].any()       # the lock and the zero trans hold
            assert np.array_equal(zg["betas"], zs["betas"]) and str(zg["gender"]) == str(zs["gender"]) and float(zg["mocap_frame_rate"]) == float(zs["mocap_frame_rate"])


def test_cli_rejects_window_1():
    from amuse_amd import main as cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--fn", "infer_gesture", "--root", str(REPO), "--smooth", "--smooth-window", "1"])
    assert "--smooth" in str(e.value) and "3..31" in str(e.value)
