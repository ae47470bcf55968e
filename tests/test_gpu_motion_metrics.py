"""GPU: the motion metrics - amuse_motion_metrics (csrc/k_motion_metrics.hip) on every crafted case of tests/motion_metrics_cases.py against the float64
restatement (tests/motion_metrics_ref.py) on the identical fp32 inputs, the joint half end to end from pose rows, the latent half, and the trainer's wiring.

The kernel's bar: |got - want| <= 1e-9, absolute.  All arithmetic is double on both sides; a sum has at most 300 terms of magnitude <= ~50, so the expected
difference is ~1e-12 from summation order and fused multiply-adds alone.  The bar leaves three orders of margin over that and stays five orders below what any
fp32 accumulation of these sums produces.  The exact-zero, same-bits and NaN-row conditions are equalities."""
import json
import random
import types

import numpy as np
import pytest
import torch

import body_cases as bc
import motion_metrics_cases as mc
import motion_metrics_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-9


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV)      # (a copy: the cases are read-only)


def _rows(G, R, L=None):
    from amuse_amd import motion_metrics as mm
    r = mm.joint_rows(_dev(G), _dev(R), None if L is None else _dev(L, torch.int32))
    torch.cuda.synchronize()
    return r.cpu().numpy()


def _close(got, want, what):
    err = float(np.abs(got - want).max())
    print(f"{what}: max |got - want| = {err:.3e} (bar {BAR:.0e})")
    assert np.isfinite(got).all() and err <= BAR, (what, err)


@pytest.mark.parametrize("N,F", mc.SHAPES)
def test_crafted_cases_vs_restatement(N, F):
    L = mc.full_lengths(N, F)
    G, R = mc.random_pair(N, F)
    got = _rows(G, R)                                                                # lengths None: every clip has F frames
    _close(got, mr.rows(G, R, L), "random")
    assert np.array_equal(got, _rows(G, R, L))
    # G == R: every APE / AVE entry is exactly 0
    got = _rows(R, R)
    assert np.array_equal(got[:, :222], np.zeros((N, 222)))
    _close(got, mr.rows(R, R, L), "equal")
    assert np.array_equal(got[:, mr.SL["vel_gen"]], got[:, mr.SL["vel_ref"]]) and np.array_equal(got[:, mr.SL["acc_gen"]], got[:, mr.SL["acc_ref"]])
    # G = R + c: APE = |c| L, the velocities / accelerations of both are equal
    Gc, Rc = mc.constant_shift(N, F)
    got = _rows(Gc, Rc)
    _close(got, mr.rows(Gc, Rc, L), "constant shift")
    c = float(np.linalg.norm(mc.SHIFT.astype(np.float64)))
    assert np.abs(got[:, mr.SL["ape_joints"]] - c * F).max() <= BAR and np.abs(got[:, mr.SL["ape_root"]] - c * F).max() <= BAR
    assert np.abs(got[:, mr.SL["ape_traj"]] - float(np.hypot(float(mc.SHIFT[0]), float(mc.SHIFT[2]))) * F).max() <= BAR
    assert np.array_equal(got[:, mr.SL["ape_pose"]], np.zeros((N, 54)))
    assert np.array_equal(got[:, mr.SL["vel_gen"]], got[:, mr.SL["vel_ref"]]) and np.array_equal(got[:, mr.SL["acc_gen"]], got[:, mr.SL["acc_ref"]])
    # a static clip: variance, vel and acc are exactly 0
    Gs, Rs = mc.static_pair(N, F)
    got = _rows(Gs, Rs)
    assert np.array_equal(got[:, 111:], np.zeros((N, 442 - 111)))
    _close(got, mr.rows(Gs, Rs, L), "static")
    # mixed lengths {2, 3, F}, NaN at and beyond L_n: every result is finite
    Gm, Rm, Lm = mc.mixed_lengths(N, F)
    got = _rows(Gm, Rm, Lm)
    assert np.isfinite(got).all()
    _close(got, mr.rows(Gm, Rm, Lm), "mixed lengths")
    if F == 2:
        assert np.array_equal(got[:, mr.SL["acc_gen"]], np.zeros((N, 55)))           # L = 2: no second difference
    # a root offset of 1000 m on both sets: APE exact (the offset cancels in the fp32-exact differences), AVE within the bar
    Go_, Ro_, Go, Ro = mc.offset_pair(N, F)
    base, got = _rows(Go_, Ro_), _rows(Go, Ro)
    _close(base, mr.rows(Go_, Ro_, L), "grid")
    _close(got, mr.rows(Go, Ro, L), "1000 m offset")
    assert np.array_equal(got[:, :111], base[:, :111]) and np.array_equal(got[:, 222:], base[:, 222:])
    d = float(np.abs(got[:, 111:222] - base[:, 111:222]).max())
    print(f"1000 m offset: AVE moved by {d:.3e}")
    assert d <= BAR


@pytest.mark.parametrize("F", [2, 5, 67, 300])
def test_same_bits_alone_and_in_a_batch_and_nan_rows(F):
    G1, R1, L1, G5, R5, L5, k = mc.alone_and_in_batch(F)
    alone, batch = _rows(G1, R1, L1), _rows(G5, R5, L5)
    assert np.array_equal(alone[0].view(np.uint64), batch[k].view(np.uint64))        # same clip, same bits
    _close(batch, mr.rows(G5, R5, L5), "batch of 5")
    G, R, L, bad = mc.bad_lengths(F)
    got, want = _rows(G, R, L), mr.rows(G, R, L)
    good = [n for n in range(4) if n not in bad]
    assert np.isnan(got[list(bad)]).all() and np.isfinite(got[good]).all()           # exactly those rows are NaN
    _close(got[good], want[good], "beside the NaN rows")


def test_stream_capture_and_argument_refusals():
    """the call sits in a captured graph (no allocation, no copy, no synchronisation) and a replay follows the device inputs"""
    from amuse_amd import motion_metrics as mm
    G, R = mc.random_pair(3, 5)
    g, r, ln = _dev(G), _dev(R), _dev(mc.full_lengths(3, 5), torch.int32)
    eager = mm.joint_rows(g, r, ln).clone()
    out = []
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.append(mm.joint_rows(g, r, ln))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager)
    g.copy_(r)
    graph.replay()
    torch.cuda.synchronize()
    assert float(out[0][:, :222].abs().max()) == 0.0
    with pytest.raises(ValueError):
        mm.joint_rows(g, r[:, :4], ln)
    with pytest.raises(ValueError):
        mm.joint_rows(g.double(), r.double(), ln)


# ------------------------------------------------------------------ end to end: pose rows -> joints -> rows
def _bodies():
    from amuse_amd import body
    models = {g: bc.make_model(203, seed=40 + i) for i, g in enumerate(("male", "female"))}
    return models, body.BodyLosses({g: body.BodyModel.from_dict(m) for g, m in models.items()}, DEV)


def test_joint_half_end_to_end_from_pose_rows():
    """body_cases.make_model(V = 203), N = 3, F = 5, two subjects (a male and a female actor, each through its own model): MotionMetrics' joints + joint_rows from
    pose rows against the float64 torch twin's joints pushed through the restatement.  The only fp32 error is the body forward's.  Bars, computed here from the
    same inputs: per APE / velocity / acceleration entry L x the forward bar of tests/test_gpu_body.py for this case, 4 max(d32, dx) from
    body_cases.forward_distances (a frame's term moves by at most the joint's displacement); per AVE entry the same bar times 2 max |coordinate deviation| (a
    variance moves by 2 (x - mean) dx summed over L frames and divided by L - 1)."""
    from amuse_amd import body, motion_metrics as mm
    models, bl = _bodies()
    try:
        N, F = 3, 5
        attr = [("scott", "male"), ("miranda", "female"), ("scott", "male")]
        sets = bc.make_loss_sets(N, F, seed=11)
        (aa_r, tr_r, _), (aa_g, tr_g, _) = sets[0], sets[1]
        ev = mm.MotionMetrics(types.SimpleNamespace(diffusion_only=False), bl)
        sub = bl.subjects(attr)
        jg, jr = ev.joints(_dev(bc.motion_rows(aa_g, tr_g)), sub), ev.joints(_dev(bc.motion_rows(aa_r, tr_r)), sub)
        got = mm.joint_rows(jg, jr).cpu().numpy()
        rows_np = bl.subject_rows(attr)
        j64, fwd = {}, 0.0
        for tag, (aa, tr) in (("g", (aa_g, tr_g)), ("r", (aa_r, tr_r))):
            j64[tag] = np.zeros((N, F, 55, 3))
            for i, gname in enumerate(bl.genders):
                idx = np.nonzero(rows_np[i] >= 0)[0]
                betas = bl.betas[rows_np[i][idx]]
                j, _, d = bc.forward_distances(models[gname], betas, aa[idx], tr[idx])
                twin = body.torch_forward(bl.models[gname], bl.betas, torch.from_numpy(aa[idx]), torch.from_numpy(tr[idx]), subject=rows_np[i][idx])[0].numpy()
                assert np.abs(twin - j).max() < 1e-9                                 # the float64 torch twin == the numpy restatement
                j64[tag][idx] = twin
                fwd = max(fwd, 4 * max(d["d32"], d["dx"]))
        err_j = max(float(np.abs(jg.cpu().numpy() - j64["g"]).max()), float(np.abs(jr.cpu().numpy() - j64["r"]).max()))
        want = mr.rows(j64["g"], j64["r"], np.full(N, F))
        dev = max(float(np.abs(x - x.mean(1, keepdims=True)).max()) for x in (j64["g"], j64["r"], j64["g"] - j64["g"][:, :, :1], j64["r"] - j64["r"][:, :, :1]))
        bar_ape, bar_ave = F * fwd, F * fwd * 2 * dev
        err = np.abs(got - want)
        e_ape, e_ave, e_va = float(err[:, :111].max()), float(err[:, 111:222].max()), float(err[:, 222:].max())
        print(f"forward bar {fwd:.3e} (joints off by {err_j:.3e}); APE err {e_ape:.3e} (bar {bar_ape:.3e}); AVE err {e_ave:.3e} (bar {bar_ave:.3e}, max deviation "
              f"{dev:.3f} m); vel / acc err {e_va:.3e}")
        assert err_j <= fwd and e_ape <= bar_ape and e_va <= 4 * bar_ape and e_ave <= bar_ave    # (a second difference holds four joint positions' worth of error)
        assert float(want[:, :111].min()) > 0                                        # the sets differ: nothing here is trivially zero
    finally:
        bl.close()


# ------------------------------------------------------------------ the latent half, and the trainer
@pytest.fixture(scope="module")
def lpdm():
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device=DEV, seed=2024)
    m.precision = "fp32x"
    m.set_sampler("ddim", 4)
    yield m
    m.engine.close()


def _motions(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([0.3 * torch.randn(n, 300, 165, generator=g), 0.2 * torch.randn(n, 300, 3, generator=g)], -1)


def test_latent_half_with_random_prior_weights(lpdm):
    from amuse_amd import motion_metrics as mm
    _, bl = _bodies()
    try:
        gen, ref = _motions(4, 1), _motions(4, 2)
        ev = mm.MotionMetrics(lpdm, bl)
        out = ev.update(gen, ref, [("scott", "male"), ("miranda", "female")] * 2)
        eng = lpdm.engine
        for motion, key, held in ((gen, "mu_gen", ev.latent.arrays()[0]), (ref, "mu_ref", ev.latent.arrays()[1])):
            m = motion.to(DEV)
            mu = eng.vae_encode(eng.smplx_to_feats(m[..., :165].reshape(4, 300, 55, 3).contiguous(), m[..., 165:].contiguous()), None, "fp32x", eps=None)["mu"]
            assert torch.equal(out[key], mu) and np.array_equal(held, mu.cpu().numpy().astype(np.float64))     # the existing encode path's mu, bit for bit
        assert ev.joint.count == 1200 and ev.joint.count_seq == 4 and np.isfinite(ev.joint.rows).all()
        assert not torch.equal(out["mu_gen"], out["mu_ref"])
        both = mm.LatentMetrics()
        both.update(out["mu_gen"], out["mu_gen"])
        tr_ = float(np.trace(np.cov(both.arrays()[0], rowvar=False)))
        fid = both.fid()
        print(f"FID of a set against itself: {fid:.3e} (tr Sigma {tr_:.3e})")
        assert abs(fid) <= 1e-9 * tr_
        assert ev.latent.fid() > 1e-6 * tr_
        with pytest.raises(ValueError, match=r"300.*4"):
            ev.latent.compute()
        with pytest.raises(ValueError, match="diffusion_only"):
            mm.MotionMetrics(types.SimpleNamespace(diffusion_only=True), bl)
    finally:
        bl.close()


def _edit_config(tmp_path, task, metrics_only, switch):
    from conftest import make_reference_tree
    from amuse_amd import main as cli
    root = tmp_path / "tree"
    if not root.exists():
        make_reference_tree(root)
    config, _ = cli.load_config(root, "edit_gesture", None)
    tp = config["TRAIN_PARAM"]
    tp["test"]["emotion_control_list"]["use"] = False
    tp["motion_extractor"]["metrics_only"] = metrics_only
    if task == "emotion_control":
        tp["test"]["emotion_control"] = {"use": True, "overwrite": None, "actor": "[scott]", "take_element": "first"}
    else:
        tp["test"]["style_transfer"] = {"use": True, "overwrite": None, "actors": "[scott-miranda]", "emotion": "[fear]"}
    if switch:
        tp["test"]["motion_metrics"] = True
    return config


def _take(k, actor, gender, **extra):
    g = torch.Generator().manual_seed(100 + k)
    con, emo, sty = (torch.randn(1, 256, generator=g) for _ in range(3))
    return dict({"ld_z": torch.zeros(1, 128), "ld_z_con": con, "ld_z_emo": emo, "ld_z_sty": sty, "ld_attr": (actor, gender, "native", "x", "30"),
                 "ld_wav": np.zeros(10000, np.float32), "ld_motion": _motions(1, 50 + k)}, **extra)


def _run(lpdm, config, loader, models, stamp, tmp_path):
    from amuse_amd.trainer import trainer
    lpdm._clip_counter = 0
    lpdm.emotion_control, lpdm.style_transfer, lpdm.style_Xemo_transfer = (bool(config["TRAIN_PARAM"]["test"][k]["use"]) for k in
                                                                           ("emotion_control", "style_transfer", "style_Xemo_transfer"))
    random.seed(5)
    tr = trainer(config, torch.device(DEV), train_loader=loader(), model_path=tmp_path / "saved", model=lpdm, stamp=stamp, body_models=models)
    written = tr.eval_prior_latdiff_forward_backward_v1(False, 7, False, False, modelversion="full", ammetric=True)
    return tr, written


def test_trainer_writes_the_report_and_changes_nothing_else(lpdm, tmp_path):
    from amuse_amd import body
    models = {g: body.BodyModel.from_dict(bc.make_model(203, seed=40 + i)) for i, g in enumerate(("male", "female"))}
    # one edit task, two jobs (two actors with one take each: every take samples its own emotion only), metrics_only: nothing is rendered, the JSON is written
    loader = lambda: {"emotion_control_info": "[scott]_all", "emotion_control": {"scott": {"0_9_9": _take(0, "scott", "male")}, "miranda": {"0_9_9": _take(1, "miranda", "female")}}}
    tr_on, w_on = _run(lpdm, _edit_config(tmp_path, "emotion_control", True, True), loader, models, "on", tmp_path)
    assert w_on == [] and tr_on.motion_metrics_path is not None and tr_on.motion_metrics_path.name == "motion_metrics_on_E7.json"
    rep = json.loads(tr_on.motion_metrics_path.read_text())
    assert len(tr_on.metrics["emotion_control"]) == 2
    t = rep["tasks"]["emotion_control"]
    assert t["count_seq"] == 2 and t["count"] == 600 and rep["overall"]["count_seq"] == 2 and rep["precision"] == "fp32x"
    assert t["Diversity"] is None and "300" in t["Diversity_reason"] and "2" in t["Diversity_reason"] and t["FID"] is not None
    assert all(np.isfinite(t[k]) and t[k] > 0 for k in ("APE_root", "APE_mean_joints", "AVE_mean_pose", "vel_gen", "acc_ref"))
    # the switch off: the same run leaves self.metrics as it is and writes no report
    tr_off, w_off = _run(lpdm, _edit_config(tmp_path, "emotion_control", True, False), loader, models, "off", tmp_path)
    assert tr_off.motion_metrics_path is None and not list((tmp_path / "saved").rglob("motion_metrics_off*"))
    for a, b in zip(tr_on.metrics["emotion_control"], tr_off.metrics["emotion_control"]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])) if torch.is_tensor(a[k]) or isinstance(a[k], np.ndarray) else a[k] == b[k], k
    # without the SMPL-X models the switch alone evaluates nothing (main.py refuses that combination at start-up)
    tr_nm, _ = _run(lpdm, _edit_config(tmp_path, "emotion_control", True, True), loader, None, "nomodels", tmp_path)
    assert tr_nm.motion_metrics_path is None
    # rendering on (style_transfer: 8 jobs): the NPZ files carry the same names and bytes with the switch on and off
    f1, f2 = "0_103_103", "0_104_104"
    st = lambda: {"style_transfer_info": "[scott-miranda]_[fear]", "style_transfer": {
        "scott": {f1: _take(2, "scott", "male", ld_emo_label="fear"), f2: _take(3, "scott", "male", ld_emo_label="fear")},
        "miranda": {f1: _take(4, "miranda", "female", ld_emo_label="fear"), f2: _take(5, "miranda", "female", ld_emo_label="fear")}}}
    tr0, n0 = _run(lpdm, _edit_config(tmp_path, "style_transfer", False, False), st, models, "st_off", tmp_path)
    tr1, n1 = _run(lpdm, _edit_config(tmp_path, "style_transfer", False, True), st, models, "st_on", tmp_path)
    assert len(n0) == len(n1) == 8 and [p.name for p in n0] == [p.name for p in n1]
    assert all(a.read_bytes() == b.read_bytes() for a, b in zip(n0, n1))
    rep = json.loads(tr1.motion_metrics_path.read_text())
    assert rep["tasks"]["style_transfer"]["count_seq"] == 8 and tr0.motion_metrics_path is None

