"""CPU: the motion metrics without a GPU - the float64 restatement's known answers on the crafted cases (worked out by hand here), the Frechet distance of
amuse_amd/motion_metrics.py against scipy.linalg.sqrtm's form of the formula, the accumulators' sums and divisions, the Diversity refusal, the ABI entries, the
command line's refusal and the JSON writer."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import motion_metrics_cases as mc
import motion_metrics_ref as mr

REPO = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------ the restatement: known answers
def test_row_known_answers_by_hand():
    """a clip of three frames whose numbers can be followed on paper: every joint of G moves along x by 1 per frame from j, R stands still at 0 except joint 2"""
    F = 3
    G, R = np.zeros((F, 55, 3)), np.zeros((F, 55, 3))
    for f in range(F):
        G[f, :, 0] = np.arange(55) + f           # joint j at x = j + f, so local_G[f][j] = (j, 0, 0) for every f
        G[f, :, 2] = 2.0 * f * f                 # z = 0, 2, 8: second difference 4, for every joint alike (so it cancels in local)
    R[:, 2, 1] = [0.0, 3.0, 0.0]                 # R's joint 2 jumps to y = 3 in the middle frame
    row = mr.clip_row(G, R, 3)
    b = {k: row[s] for k, s in mr.SL.items()}
    # root: G = (f, 0, 2 f^2), R = 0 -> |.| = 0, sqrt(1 + 4), sqrt(4 + 64)
    assert b["ape_root"][0] == pytest.approx(np.sqrt(5) + np.sqrt(68), abs=1e-14) and b["ape_traj"][0] == pytest.approx(np.sqrt(5) + np.sqrt(68), abs=1e-14)
    # local_G[j] = (j, 0, 0) in all three frames; local_R = 0 except joint 2 at frame 1: (0, 3, 0)
    want_pose = 3.0 * np.arange(1, 55)
    want_pose[1] = 2.0 + 2.0 + np.sqrt(4.0 + 9.0)
    assert np.allclose(b["ape_pose"], want_pose, atol=1e-13)
    assert b["ape_joints"][7] == pytest.approx(7.0 + np.sqrt(64 + 4) + np.sqrt(81 + 64), abs=1e-13)
    # variances over 3 frames, / 2: x (j, j+1, j+2) -> 1; z (0, 2, 8): mean 10/3, sum sq dev = 100/9 + 16/9 + 196/9 = 104/3 -> 52/3; R's joint 2 y (0, 3, 0) -> 3
    assert b["ave_root"][0] == pytest.approx(np.hypot(1.0, 52.0 / 3.0), abs=1e-13) and b["ave_traj"][0] == pytest.approx(np.hypot(1.0, 52.0 / 3.0), abs=1e-13)
    assert b["ave_joints"][5] == pytest.approx(np.hypot(1.0, 52.0 / 3.0), abs=1e-13)
    assert b["ave_joints"][2] == pytest.approx(np.sqrt(1.0 + 9.0 + (52.0 / 3.0) ** 2), abs=1e-13)
    want_ave_pose = np.zeros(54)
    want_ave_pose[1] = 3.0                        # local_G is constant in time; local_R's joint 2 has variance 3 in y
    assert np.allclose(b["ave_pose"], want_ave_pose, atol=1e-13)
    # velocities: G steps (1, 0, 2) then (1, 0, 6); R's joint 2 steps 3 up and 3 down; accelerations: G (0, 0, 4), R's joint 2 |0 - 6 + 0|
    assert np.allclose(b["vel_gen"], np.sqrt(5) + np.sqrt(37), atol=1e-13) and np.allclose(b["acc_gen"], 4.0, atol=1e-13)
    want_vr, want_ar = np.zeros(55), np.zeros(55)
    want_vr[2], want_ar[2] = 6.0, 6.0
    assert np.array_equal(b["vel_ref"], want_vr) and np.array_equal(b["acc_ref"], want_ar)
    # L = 2 of the same clip: no second difference; one first difference
    b2 = {k: mr.clip_row(G, R, 2)[s] for k, s in mr.SL.items()}
    assert np.array_equal(b2["acc_gen"], np.zeros(55)) and np.allclose(b2["vel_gen"], np.sqrt(5), atol=1e-14) and b2["vel_ref"][2] == 3.0
    assert np.isnan(mr.clip_row(G, R, 1)).all() and np.isnan(mr.clip_row(G, R, 4)).all()
    assert sum(n for _, _, n in mr.BLOCKS) == mr.ROW and all(o == sum(m for _, _, m in mr.BLOCKS[:i]) for i, (_, o, _) in enumerate(mr.BLOCKS))


@pytest.mark.parametrize("N,F", mc.SHAPES)
def test_crafted_cases_on_the_restatement(N, F):
    L = mc.full_lengths(N, F)
    ape_ave = slice(0, 222)
    R = mc.random_pair(N, F)[1]
    assert np.array_equal(mr.rows(R, R, L)[:, ape_ave], np.zeros((N, 222)))                       # G == R
    G, R = mc.constant_shift(N, F)
    r = mr.rows(G, R, L)
    c = float(np.linalg.norm(mc.SHIFT.astype(np.float64)))
    assert np.abs(r[:, mr.SL["ape_joints"]] - c * F).max() <= 1e-12 * F and np.abs(r[:, mr.SL["ape_traj"]] - np.hypot(0.25, 0.125) * F).max() <= 1e-12 * F
    assert np.abs(r[:, mr.SL["ape_pose"]]).max() == 0.0
    assert np.array_equal(r[:, mr.SL["vel_gen"]], r[:, mr.SL["vel_ref"]]) and np.array_equal(r[:, mr.SL["acc_gen"]], r[:, mr.SL["acc_ref"]])
    G, R = mc.static_pair(N, F)
    r = mr.rows(G, R, L)
    assert np.array_equal(r[:, 111:], np.zeros((N, 442 - 111)))                                   # variance, vel and acc of a static clip: exactly 0
    G, R, Lm = mc.mixed_lengths(N, F)
    assert np.isfinite(mr.rows(G, R, Lm)).all() and (np.isnan(G).any() or F == 2)
    G, R, Go, Ro = mc.offset_pair(N, F)
    r0, r1 = mr.rows(G, R, L), mr.rows(Go, Ro, L)
    assert np.array_equal(r0[:, :111], r1[:, :111])                                               # APE: the offset cancels exactly in the differences
    assert np.abs(r0[:, 111:222] - r1[:, 111:222]).max() <= 1e-9                                  # AVE must not move
    # ... which a one-pass fp32 variance does not manage: E[x^2] - E[x]^2 at 1000 m in float32 is off by far more than the bar
    x = Go[0, :, 0, 0]
    one_pass = (np.mean(x * x, dtype=np.float32) - np.mean(x, dtype=np.float32) ** 2) * np.float32(F / (F - 1.0))
    assert abs(float(one_pass) - float(np.var(x.astype(np.float64), ddof=1))) > 1e-6
    G, R, Lb, bad = mc.bad_lengths(F)
    r = mr.rows(G, R, Lb)
    assert [n for n in range(4) if np.isnan(r[n]).any()] == list(bad) and np.isnan(r[list(bad)]).all()


# ------------------------------------------------------------------ Frechet distance
@pytest.mark.parametrize("n,rank", [(400, None), (60, None), (200, 17)])
def test_frechet_distance_vs_scipy_sqrtm(n, rank):
    """random SPD moments (n > 128), a rank-deficient pair from n < 128 samples, and a pair of rank 17: the eigh route of the product code against
    scipy.linalg.sqrtm's form of the same formula, and against the eigenvalues of C1 C2 taken directly"""
    from amuse_amd import motion_metrics as mm
    g, r = mc.latents(n, seed=n, rank=rank)
    m1, c1 = mm.moments(g)
    m2, c2 = mm.moments(r)
    assert np.array_equal(c1, np.cov(g, rowvar=False)) and np.linalg.matrix_rank(c1) == min(n - 1, rank or 128)
    got = mm.frechet_distance(m1, c1, m2, c2)
    scale = np.trace(c1) + np.trace(c2)
    # sqrtm of a singular product is accurate to about sqrt(eps) of its scale (it says so itself); on full-rank moments to ~1e-10
    bar = (1e-9 if (rank is None and n > 128) else 2e-6) * scale
    assert abs(got - mr.frechet_sqrtm(m1, c1, m2, c2)) <= bar, (got, mr.frechet_sqrtm(m1, c1, m2, c2))
    assert abs(got - mr.frechet_eig(m1, c1, m2, c2)) <= (1e-9 if (rank is None and n > 128) else 1e-7) * scale
    assert abs(mm.frechet_distance(m1, c1, m1, c1)) <= 1e-9 * np.trace(c1)                        # a set against itself
    assert got > 0


def test_frechet_distance_closed_form():
    """commuting (diagonal) covariances: |dmu|^2 + sum (sqrt a - sqrt b)^2"""
    from amuse_amd import motion_metrics as mm
    a, b = np.array([4.0, 9.0, 0.0, 1.0]), np.array([1.0, 16.0, 25.0, 0.0])
    want = 3.0 ** 2 + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert mm.frechet_distance(np.array([3.0, 0, 0, 0]), np.diag(a), np.zeros(4), np.diag(b)) == pytest.approx(want, abs=1e-12)


# ------------------------------------------------------------------ the accumulators
def test_joint_metrics_merge_and_divisions():
    from amuse_amd import motion_metrics as mm
    G, R, L = mc.mixed_lengths(5, 67)
    rows = mr.rows(G, R, L)
    whole = mm.JointMetrics()
    whole.update(rows, L)
    a, b = mm.JointMetrics(), mm.JointMetrics()
    a.update(rows[:2], L[:2])
    b.update(rows[2:], L[2:])
    a.merge(b)
    assert a.count == whole.count == int(L.sum()) and a.count_seq == whole.count_seq == 5
    assert np.allclose(a.rows, whole.rows, rtol=1e-15, atol=0)
    c1, c2 = a.compute(), whole.compute()
    assert all(np.allclose(c1[k], c2[k], rtol=1e-14, atol=0) for k in c2)
    # the divisions of val_metrics.py:63-92 written out by hand: APE over the frames counted, AVE over the clips counted
    s, count, count_seq = rows.sum(0), float(L.sum()), 5.0
    assert c2["APE_root"] == pytest.approx(s[0] / count, rel=1e-14) and c2["APE_traj"] == pytest.approx(s[1] / count, rel=1e-14)
    assert c2["APE_mean_pose"] == pytest.approx(s[2:56].mean() / count, rel=1e-14) and c2["APE_mean_joints"] == pytest.approx(s[56:111].mean() / count, rel=1e-14)
    assert c2["AVE_root"] == pytest.approx(s[111] / count_seq, rel=1e-14) and c2["AVE_traj"] == pytest.approx(s[112] / count_seq, rel=1e-14)
    assert c2["AVE_mean_pose"] == pytest.approx(s[113:167].mean() / count_seq, rel=1e-14)
    assert c2["AVE_mean_joints"] == pytest.approx(s[167:222].mean() / count_seq, rel=1e-14)
    assert c2["vel_gen"] == pytest.approx(s[222:277].mean() * 30.0 / (count - count_seq), rel=1e-14)
    assert c2["acc_ref"] == pytest.approx(s[387:442].mean() * 900.0 / (count - 2 * count_seq), rel=1e-14)
    ref = mr.joint_compute(rows, L)
    assert all(c2[k] == pytest.approx(v, rel=1e-13) for k, v in ref.items())
    assert c2["APE_joints_per_joint"].shape == (55,) and c2["AVE_pose_per_joint"].shape == (54,) and c2["vel_gen_per_joint"].shape == (55,)
    # state round trip; a NaN row (a clip whose length the kernel refused) is not accumulated silently
    again = mm.JointMetrics.from_state(whole.state())
    assert np.array_equal(again.rows, whole.rows) and again.count == whole.count
    with pytest.raises(ValueError, match="not finite"):
        whole.update(np.full((1, 442), np.nan), [300])


def test_latent_metrics_and_the_diversity_refusal():
    from amuse_amd import motion_metrics as mm
    g, r = mc.latents(40, seed=2)
    lm = mm.LatentMetrics()
    lm.update(g[:25], r[:25])
    lm.update(g[25:], r[25:])
    assert lm.n == 40
    with pytest.raises(ValueError, match=r"300.*40|40.*300"):
        lm.compute()                                    # the default draws 300 of 40
    with pytest.raises(ValueError, match="40"):
        lm.compute(diversity_times=40)                  # needs MORE than diversity_times, as the reference asserts
    out = lm.compute(diversity_times=39, seed=5)
    assert set(out) == {"FID", "Diversity", "gt_Diversity"}
    assert out["FID"] == pytest.approx(mr.frechet_eig(*mm.moments(g), *mm.moments(r)), rel=1e-6)
    rng = np.random.default_rng(5)
    a, b = rng.choice(40, 39, replace=False), rng.choice(40, 39, replace=False)
    assert out["Diversity"] == pytest.approx(np.linalg.norm(g[a] - g[b], axis=1).mean(), rel=1e-14)
    assert out == lm.compute(diversity_times=39, seed=5)                 # seeded: the same draw
    other = mm.LatentMetrics().merge(lm)
    assert np.array_equal(other.arrays()[0], g) and np.array_equal(other.arrays()[1], r)
    assert "R-precision" in mm.LatentMetrics.__doc__ or "R-precision" in mm.__doc__


# ------------------------------------------------------------------ ABI, command line, report
def test_abi_symbols_and_row_table():
    from amuse_amd import _lib, motion_metrics as mm
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", (REPO / "include/amuse_hip.h").read_text(), flags=re.S)
    for name in ("amuse_motion_metrics_row", "amuse_motion_metrics"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.amuse_motion_metrics_row() == mm.ROW == mr.ROW == 442
    assert [(k, mm.ROW_SLICES[k].start, n) for k, n in mm.ROW_BLOCKS] == list(mr.BLOCKS)          # the Python table == the restatement's == the header's
    raw = (REPO / "include/amuse_hip.h").read_text()
    for name, off, n in mr.BLOCKS:
        assert re.search(rf"\*\s+{off}\s+{n}\s+{name}\b", raw), name
    one = 0x1000                                            # (never dereferenced: every call below fails in its checks, before any HIP call)
    for args, word in (((None, one, one, 1, 2, one), "joints_gen"), ((one, None, one, 1, 2, one), "joints_ref"), ((one, one, None, 1, 2, one), "lengths_dev"),
                       ((one, one, one, 1, 2, None), "rows_out"), ((one, one, one, 0, 2, one), "N 0"), ((one, one, one, 1, 1, one), "F 1"),
                       ((one, one, one, 1 << 20, 1 << 12, one), "an int"), ((one, one, one, 5000000, 2, one), "an int")):
        assert lib.amuse_motion_metrics(*args, None) == -1 and word in lib.amuse_last_error().decode(), (args, lib.amuse_last_error())


def test_cli_motion_metrics_needs_smplx_models(tmp_path):
    from amuse_amd import main as amain
    with pytest.raises(SystemExit) as e:
        amain.main(["--fn", "edit_gesture", "--motion-metrics", "--root", str(tmp_path)])
    assert "--motion-metrics needs --smplx-models DIR" in str(e.value)
    empty = tmp_path / "no_models_here"
    empty.mkdir()
    with pytest.raises(SystemExit) as e:
        amain.main(["--fn", "edit_gesture", "--motion-metrics", "--smplx-models", str(empty), "--root", str(tmp_path)])
    assert str(empty) in str(e.value) and "SMPLX_MALE.npz" in str(e.value)
    with pytest.raises(SystemExit) as e:
        amain.main(["--fn", "train_gesture", "--motion-metrics", "--smplx-models", str(empty)])
    assert "--motion-metrics belongs to" in str(e.value)


def test_report_writer_on_a_fake_two_task_state(tmp_path):
    from amuse_amd import motion_metrics as mm
    states = {}
    for i, (name, n) in enumerate((("style_transfer", 3), ("emotion_control", 5))):
        G, R = mc.random_pair(n, 5, seed=20 + i)
        jm, lm = mm.JointMetrics(), mm.LatentMetrics()
        jm.update(mr.rows(G, R, mc.full_lengths(n, 5)), mc.full_lengths(n, 5))
        lm.update(*mc.latents(n, seed=30 + i))
        states[name] = {"joint": jm.state(), "latent": lm.state()}
    p = mm.write_report(tmp_path / "viz" / "motion_metrics_stamp_E7.json", states, "fp32x", diversity_times=6)
    rep = json.loads(p.read_text())
    assert rep["precision"] == "fp32x" and set(rep["tasks"]) == {"style_transfer", "emotion_control"}
    t = rep["tasks"]["style_transfer"]
    assert t["count_seq"] == 3 and t["count"] == 15 and t["Diversity"] is None and "6" in t["Diversity_reason"] and "3" in t["Diversity_reason"]
    assert t["FID"] is not None and len(t["APE_joints_per_joint"]) == 55
    o = rep["overall"]
    assert o["count_seq"] == 8 and o["count"] == 40 and o["Diversity"] is not None and o["gt_Diversity"] is not None and o["latent_clips"] == 8
    G, R = (np.concatenate([mc.random_pair(3, 5, seed=20)[k], mc.random_pair(5, 5, seed=21)[k]]) for k in (0, 1))
    want = mr.joint_compute(mr.rows(G, R, mc.full_lengths(8, 5)), mc.full_lengths(8, 5))
    assert all(o[k] == pytest.approx(v, rel=1e-13) for k, v in want.items())
    # a task with nothing evaluated: counts of zero, nulls with reasons, still valid JSON
    empty = {"joint": mm.JointMetrics().state(), "latent": mm.LatentMetrics().state()}
    rep2 = json.loads(mm.write_report(tmp_path / "e.json", {"none": empty}, "bf16").read_text())
    assert rep2["tasks"]["none"]["count_seq"] == 0 and rep2["tasks"]["none"]["FID"] is None and "FID_reason" in rep2["tasks"]["none"]
