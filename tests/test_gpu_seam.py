"""GPU: the long-form candidates - the seam-cost, best-path and gather kernels (csrc/k_seam.hip through amuse_amd/seam.py) against tests/seam_ref.py's float64
restatement, and the path built on them (PretrainedLPDM_v1.infer_long(candidates=K), the trainer's long-form jobs).

Bars.  The cost is a weighted sum of squared geodesic angles; the kernel computes each angle in fp32 and everything after it in double.  With delta = max(4 x the
float32 restatement's largest |theta - theta64| ON THE CASE'S OWN INPUTS, 2^-20 rad) - the project's rule for these kernels: fp32 arithmetic in another order may
be four times worse than fp32 arithmetic in numpy's order, nothing more (the float32 restatement sits at 3.1e-7 .. 6.5e-7 rad on these cases) - the bar of a
pair is sum_i u_i sum_j w_j (2 theta64 delta + delta^2), plus the translation term with every fp32 difference allowed 4 ulp of the larger input
(seam_ref.cost_bar).  Nothing is excluded: theta = 2 atan2(|r.xyz|, |r.w|) has no coin-toss inputs.  The path is held to the restatement's dynamic programme
exactly, choices and totals bit for bit; the gather to the input rows' bits.

Inputs: tests/seam_cases.py."""
import itertools
import random

import numpy as np
import pytest
import torch

import seam_cases as sc
import seam_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _cost(c, poses=None, trans=None, windows=None, frames=None, K=None, **kw):
    from amuse_amd import seam
    poses = c["poses"] if poses is None else poses
    trans = c["trans"] if trans is None and c["trans"] is not None else trans
    p = torch.tensor(poses, device=DEV)                                        # (torch.tensor copies: the shared case stays read-only)
    t = None if c["trans"] is None else torch.tensor(trans, device=DEV)
    return seam.cost(p, t, c["windows"] if windows is None else windows, c["frames"] if frames is None else frames, c["K"] if K is None else K, c["hop"], F=c["F"],
                     row_weight=torch.tensor(c["row_weight"]), joint_weight=torch.tensor(c["joint_weight"]), trans_weight=c["trans_weight"], **kw)


def _check_bar(name, m, cost64, bar):
    assert m.shape == cost64.shape and m.dtype == np.float64 and np.isfinite(m).all()
    ratio = np.abs(m - cost64) / bar
    print(f"{name}: {m.size} pairs, cost {cost64.min():.4g} .. {cost64.max():.4g}, worst |error| / bar {ratio.max():.3f} (largest error {np.abs(m - cost64).max():.3e})")
    assert (ratio <= 1.0).all(), float(ratio.max())


@pytest.mark.parametrize("name", list(sc.CASES))
def test_cost_against_float64_restatement(name):
    c = sc.case(name)
    m = _cost(c).cpu().numpy()
    print(f"{name}: float32 restatement's largest angle distance {c['f32_dist']:.3e} rad, delta {c['delta']:.3e}")
    _check_bar(name, m, c["cost64"], c["bar"])


def _bytes_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_a_pairs_cost_has_the_same_bits_wherever_it_is_computed():
    c = sc.case("cut_short")
    K, windows, frames = c["K"], c["windows"], c["frames"]
    full = _cost(c).cpu().numpy()
    assert _bytes_equal(_cost(c).cpu().numpy(), full)                           # a repeat
    # candidate subsets re-packed as K = 2
    nw = sum(windows)
    for sub in ((0, 3), (4, 1), (2, 2)):
        rows = [g * K + s for g in range(nw) for s in sub]
        got = _cost(c, poses=c["poses"][rows], trans=c["trans"][rows], K=2).cpu().numpy()
        assert _bytes_equal(got, full[:, list(sub)][:, :, list(sub)]), sub
    # the sequences one per call: another launch, another sequence slot, another place in the batch
    g0 = s0 = 0
    for W, L in zip(windows, frames):
        got = _cost(c, poses=c["poses"][g0 * K:(g0 + W) * K], trans=c["trans"][g0 * K:(g0 + W) * K], windows=(W,), frames=(L,)).cpu().numpy()
        assert _bytes_equal(got, full[s0:s0 + W - 1])
        g0, s0 = g0 + W, s0 + W - 1


def test_cost_graph_replay_follows_overwritten_inputs():
    from amuse_amd import seam
    c = sc.case("cut_short")
    p, t = torch.tensor(c["poses"], device=DEV), torch.tensor(c["trans"], device=DEV)
    u, w = torch.tensor(c["row_weight"], device=DEV), torch.tensor(c["joint_weight"], device=DEV)
    pl = seam.plan(c["windows"], c["K"], c["hop"], c["F"])
    ws = torch.empty(pl["workspace_bytes"], device=DEV, dtype=torch.uint8)
    out = torch.zeros(pl["seams"], c["K"], c["K"], device=DEV, dtype=torch.float64)
    call = lambda **kw: seam.cost(p, t, c["windows"], c["frames"], c["K"], c["hop"], F=c["F"], row_weight=u, joint_weight=w, trans_weight=c["trans_weight"], **kw)
    e1 = call().clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                # one linear branch: the entry point allocates nothing and copies nothing
        call(workspace=ws, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, e1)
    p2, t2 = sc.make(c["F"], c["hop"], c["windows"], c["frames"], c["K"], seed=77)
    p.copy_(torch.from_numpy(p2))
    t.copy_(torch.from_numpy(t2))
    g.replay()
    torch.cuda.synchronize()
    e2 = call()
    torch.cuda.synchronize()
    assert torch.equal(out, e2) and not torch.equal(out, e1)


def _check_path(m, windows, K, what):
    from amuse_amd import seam
    choice, total = seam.path(torch.tensor(m, device=DEV, dtype=torch.float64).reshape(-1, K, K), windows, K)
    rc, rt = ref.best_path(m, windows, K)
    assert np.array_equal(choice.cpu().numpy(), rc), what
    assert total.cpu().numpy().tobytes() == rt.tobytes(), what
    return rc, rt


def test_path_is_the_restatements_dynamic_programme_exactly():
    for k, (windows, K, m) in enumerate(sc.int_matrices()):                      # ties; W = 1; K = 1; several sequences
        _check_path(m, windows, K, f"integer matrix {k}")
    for name in ("cut_short", "capacity_plus_one", "one_candidate", "k64"):      # the GPU's own cost matrices: 33 sequences, K = 1, K = 64
        c = sc.case(name)
        rc, rt = _check_path(_cost(c).cpu().numpy(), c["windows"], c["K"], name)
        assert np.isfinite(rt).all() and len(rc) == sum(c["windows"])
    rng = np.random.default_rng(8)
    _check_path(rng.uniform(0, 5, (4, 64, 64)), (5,), 64, "random K = 64")
    _check_path(rng.integers(0, 2, (6, 64, 64)).astype(np.float64), (3, 5), 64, "ties at K = 64")
    _check_path(rng.uniform(0, 5, (1999, 3, 3)), (2000,), 3, "more windows than one round of back-pointers holds")
    _check_path(rng.integers(0, 2, (2100, 2, 2)).astype(np.float64), (962, 1, 1140), 2, "961 windows + 1: the round boundary, with ties")
    m = rng.uniform(0, 5, (5, 4, 4))                                             # NaN / inf entries never win
    m[0, 1, :], m[1, :, 2], m[2, 0, 0], m[3, 3, 3], m[4, 2, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    rc, rt = _check_path(m, (6,), 4, "non-finite entries")
    assert np.isfinite(rt).all()
    rc, rt = _check_path(np.full((3, 4, 4), np.nan), (4,), 4, "nothing finite")
    assert rc.tolist() == [0, 4, 8, 12] and np.isinf(rt[0])
    m = rng.uniform(0, 5, (3, 4, 4))
    m[1] = np.inf                                                                # one impassable seam: +inf total, candidate 0 from there on
    rc, rt = _check_path(m, (4,), 4, "an impassable seam")
    assert np.isinf(rt[0]) and rc[2:].tolist() == [8, 12]
    rc, rt = _check_path(np.zeros((0, 5, 5)), (1, 1, 1), 5, "single windows only")
    assert rc.tolist() == [0, 5, 10] and rt.tolist() == [0.0, 0.0, 0.0]


def test_select_is_a_bitwise_gather_and_refuses_overlap():
    from amuse_amd import _lib, seam
    c = sc.case("two_sequences")
    p, t = torch.tensor(c["poses"], device=DEV), torch.tensor(c["trans"], device=DEV)
    choice = torch.tensor([1, 2, 5, 7], device=DEV, dtype=torch.int32)
    po, to = seam.select(p, t, choice)
    torch.cuda.synchronize()
    rp, rt = ref.select(c["poses"], c["trans"], [1, 2, 5, 7])
    assert np.array_equal(po.cpu().numpy().view(np.uint32), rp.view(np.uint32)) and np.array_equal(to.cpu().numpy().view(np.uint32), rt.view(np.uint32))
    po2, to2 = seam.select(p, None, choice)
    assert to2 is None and torch.equal(po2, po)
    # a choice outside the input is never read: its output row is NaN, the others are copies
    po3, to3 = seam.select(p, t, torch.tensor([3, 8, -1], device=DEV, dtype=torch.int32))
    assert torch.equal(po3[0], p[3]) and torch.equal(to3[0], t[3]) and bool(torch.isnan(po3[1:]).all()) and bool(torch.isnan(to3[1:]).all())
    with pytest.raises(_lib.AmuseHipError, match="overlaps"):
        seam.select(p, None, choice[:2], poses_out=p[2:4])                       # in place
    big = torch.zeros(12, c["F"], 55, 3, device=DEV)
    with pytest.raises(_lib.AmuseHipError, match="overlaps"):
        seam.select(big[:8], None, choice[:2], poses_out=big[7:9])               # the output's first row is the input's last
    po4, _ = seam.select(big[:8], None, choice[:2], poses_out=big[8:10])         # right behind the input: accepted
    assert po4.data_ptr() == big[8].data_ptr()


def test_best_windows_chains_the_three_calls():
    from amuse_amd import seam
    c = sc.case("cut_short")
    K, windows = c["K"], c["windows"]
    p, t = torch.tensor(c["poses"], device=DEV), torch.tensor(c["trans"], device=DEV)
    po, to, info = seam.best_windows(p, t, windows, c["frames"], K, c["hop"], F=c["F"], row_weight=torch.tensor(c["row_weight"]),
                                     joint_weight=torch.tensor(c["joint_weight"]), trans_weight=c["trans_weight"])
    m = info["cost"].cpu().numpy()
    rc, rt = ref.best_path(m, windows, K)
    assert np.array_equal(info["choice"].cpu().numpy(), rc) and info["total"].cpu().numpy().tobytes() == rt.tobytes()
    assert torch.equal(po, p[torch.from_numpy(rc).long().to(DEV)]) and torch.equal(to, t[torch.from_numpy(rc).long().to(DEV)])
    rep = seam.report(info, windows, K)
    s0 = g0 = 0
    for s, W in enumerate(windows):
        first = ref.path_total(m, K, s0, [0] * W)
        assert np.float64(rep[s]["total_first"]).tobytes() == np.float64(first).tobytes() and rep[s]["total"] == rt[s] <= first
        assert rep[s]["choice"] == [int(r) - (g0 + k) * K for k, r in enumerate(rc[g0:g0 + W])]
        s0, g0 = s0 + W - 1, g0 + W


# ------------------------------------------------------------------ the path built on the kernels
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


def _wave(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    return (0.2 * torch.sin(2 * np.pi * 220.0 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 0.3 * t)) + 0.05 * torch.randn(n, generator=g) + 0.01)[None]


def test_infer_long_with_candidates_is_sample_choose_stitch(model):
    from amuse_amd import longform, seam
    K, wave = 4, _wave(400000, 1)
    model._clip_counter = 7
    out = model.infer_long([wave], candidates=K)
    assert model._clip_counter == 7 + 3 * K and len(out) == 1 and out[0]["poses"].shape == (750, 55, 3) and out[0]["trans"].shape == (750, 3)
    rep = out[0]["seam"]
    # the twelve clips, run explicitly at the same clip indices: row g K + c is candidate c of window g, the window's embeddings repeated
    a = wave - wave.mean()
    chunks = [a[:, s:e] for s, e in longform.window_slices(400000, 270)]
    embs = model.process_seq_list(chunks, framerate=16000)
    con, emo, sty = (torch.cat([e[i] for e in embs]).repeat_interleave(K, dim=0) for i in range(3))
    ob = model.diffusion_backward(3 * K, con, emo, sty, clip_index0=7)
    assert model._clip_counter == 7 + 3 * K
    # the condition of everything below: the candidates of a window are distinct motions, so the cost matrix is not constant
    for g in range(3):
        for c1, c2 in itertools.combinations(range(K), 2):
            assert not torch.equal(ob["poses"][g * K + c1], ob["poses"][g * K + c2])
    m = seam.cost(ob["poses"], ob["trans"], [3], [750], K, 270).cpu().numpy()     # the product's default weights, as infer_long uses them
    assert all(len(set(m[s].ravel().tolist())) == K * K for s in range(2)), m
    # the output is the stitch of the selected rows
    rows = [g * K + c for g, c in enumerate(rep["choice"])]
    sp, st = longform.stitch(ob["poses"][rows], ob["trans"][rows], [3], [750], 270)
    assert torch.equal(sp, out[0]["poses"]) and torch.equal(st, out[0]["trans"])
    # the selected path is the best of all 64, summed on the host in the dynamic programme's order from the GPU's matrix
    totals = {p: ref.path_total(m, K, 0, p) for p in itertools.product(range(K), repeat=3)}
    chosen = totals[tuple(rep["choice"])]
    print(f"infer_long(candidates=4): choice {rep['choice']}, total {rep['total']:.6g}, all-first {rep['total_first']:.6g}, worst path {max(totals.values()):.6g}")
    assert np.float64(rep["total"]).tobytes() == np.float64(chosen).tobytes() and all(chosen <= v for v in totals.values())
    assert np.float64(rep["total_first"]).tobytes() == np.float64(totals[(0, 0, 0)]).tobytes() and rep["total"] <= rep["total_first"]
    # and that matrix passes the kernel test's bar against the restatement on these poses
    poses = ob["poses"].cpu().numpy()
    u, w, tw = (np.asarray(x) for x in seam.default_weights(30))
    th64, th32 = ref.thetas(poses, (3,), (750,), K, 270), ref.thetas(poses, (3,), (750,), K, 270, np.float32)
    f32_dist = max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(th32, th64))
    delta = max(4.0 * f32_dist, 2.0 ** -20)
    print(f"infer_long poses: float32 restatement's largest angle distance {f32_dist:.3e} rad, delta {delta:.3e}")
    _check_bar("infer_long poses", m, ref.cost(poses, None, (3,), (750,), K, 270, u, w, 0.0), ref.cost_bar(th64, delta, u, w, K=K))


def test_infer_long_one_candidate_is_infer_long(model):
    wave = _wave(400000, 1)
    model._clip_counter = 7
    a = model.infer_long([wave], candidates=1)
    assert model._clip_counter == 10 and "seam" not in a[0]
    model._clip_counter = 7
    b = model.infer_long([wave])
    assert model._clip_counter == 10 and torch.equal(a[0]["poses"], b[0]["poses"]) and torch.equal(a[0]["trans"], b[0]["trans"])
    with pytest.raises(ValueError, match="outside 1..64"):
        model.infer_long([wave], candidates=65)


def test_trainer_candidates_jobs_and_default_bytes(model, tmp_path, capsys):
    """in process, on one model: long_form_candidates 1 gives the bytes an absent key gives; with 4 the 25 s WAV is still one 750-frame NPZ and the 10 s WAVs -
    one window, not expanded - keep their bytes"""
    from conftest import make_reference_tree
    from scipy.io import wavfile
    from amuse_amd import main as cli
    from amuse_amd.trainer import trainer
    root = make_reference_tree(tmp_path / "tree", n_infer_wavs=2)
    wavfile.write(root / "viz_dump/test/speech/scott_9_long.wav", 16000, (_wave(400000, 3)[0].numpy() * 20000).astype(np.int16))   # sorts after the two 10 s files
    config, _ = cli.load_config(root, "infer_gesture", None)
    config["TRAIN_PARAM"]["test"].update(long_form=True, hop_frames=270)

    def run(cands, stamp):
        config["TRAIN_PARAM"]["test"].pop("long_form_candidates", None)
        if cands is not None:
            config["TRAIN_PARAM"]["test"]["long_form_candidates"] = cands
        model._clip_counter = 0
        random.seed(5)
        tr = trainer(config, torch.device(DEV), model=model, stamp=stamp)
        files = tr.eval_prior_latdiff_forward_backward_v1(False, 0, True, False, modelversion="full", ammetric=True)
        return files, model._clip_counter
    (absent, n0), (one, n1) = run(None, "absent"), run(1, "one")
    assert "long-form candidates" not in capsys.readouterr().out
    (four, n4) = run(4, "four")
    lines = [l for l in capsys.readouterr().out.splitlines() if "long-form candidates" in l]
    assert len(lines) == 1 and "scott_9_long" in lines[0] and "K = 4" in lines[0] and "->" in lines[0], lines
    assert (n0, n1, n4) == (5, 5, 14)
    assert [p.name for p in absent] == [p.name for p in one] == [p.name for p in four] and len(absent) == 3
    assert all(a.read_bytes() == b.read_bytes() for a, b in zip(absent, one))
    assert absent[0].read_bytes() == four[0].read_bytes() and absent[1].read_bytes() == four[1].read_bytes()
    with np.load(four[2]) as z:
        assert z["poses"].shape == (750, 55, 3) and z["trans"].shape == (750, 3) and np.isfinite(z["poses"]).all()
        assert np.abs(np.diff(z["poses"][:, 12:], axis=0)).max() > 0
