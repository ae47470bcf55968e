"""CPU: the host half of the SMPL-X body model - the loader, the float64 torch twin, LatentPriorLosses with body= and the CLI's model directory.
The reference values are tests/body_ref.py's numpy RESTATEMENT of the published algorithm (`smplx` is not installed: no pin)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import body_cases as bc
import body_ref as br
from amuse_amd import body, npz_writer

MODEL = bc.make_model(V=37, n_betas=300, seed=11)


def test_loader_round_trip_and_missing_keys(tmp_path):
    m = body.BodyModel.from_dict(MODEL)
    m.to_npz(tmp_path / "SMPLX_NEUTRAL.npz")
    with np.load(tmp_path / "SMPLX_NEUTRAL.npz") as z:
        assert z["posedirs"].shape == (37, 3, 486) and z["kintree_table"].shape == (2, 55) and int(z["kintree_table"][0, 0]) == 2 ** 32 - 1   # the file's layout
        full = {k: z[k] for k in z.files}
    back = body.BodyModel.from_npz(tmp_path / "SMPLX_NEUTRAL.npz")
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "parents"):
        assert np.array_equal(getattr(back, k), getattr(m, k)), k
    assert body.BodyModel.from_npz(tmp_path / "SMPLX_NEUTRAL.npz", num_betas=10).shapedirs.shape == (37, 3, 10)   # the file's first columns
    for k in body.NPZ_KEYS:
        np.savez(tmp_path / "broken.npz", **{q: v for q, v in full.items() if q != k})
        with pytest.raises(KeyError, match=f"lacks the key '{k}'"):
            body.BodyModel.from_npz(tmp_path / "broken.npz")
    bad = dict(MODEL, parents=MODEL["parents"].copy())
    bad["parents"][7] = 7
    with pytest.raises(ValueError, match="parents"):
        body.BodyModel.from_dict(bad)
    assert not body.models_present(tmp_path)
    for f in body.SMPLX_FILES.values():
        m.to_npz(tmp_path / f)
    assert body.models_present(tmp_path) and set(body.load_models(tmp_path)) == {"male", "female", "neutral"}


def test_torch_twin_vs_restatement():
    m = body.BodyModel.from_dict(MODEL)
    betas = bc.make_betas(3)
    aa, tr, d6 = bc.make_motion(3, 5)
    j64, v64 = br.forward(MODEL, betas, aa, tr)
    j, v = body.torch_forward(m, betas, torch.from_numpy(aa), torch.from_numpy(tr), kind="aa", frames_per_pass=2)
    assert j.dtype == torch.float64 and np.abs(j.numpy() - j64).max() < 1e-12 and np.abs(v.numpy() - v64).max() < 1e-12
    sub = np.array([2, 0, 1])
    j6, v6 = body.torch_forward(m, betas, torch.from_numpy(d6), torch.from_numpy(tr), subject=sub, kind="6d")
    j6r, v6r = br.forward(MODEL, betas[sub], d6, tr, "6d")
    assert np.abs(j6.numpy() - j6r).max() < 1e-12 and np.abs(v6.numpy() - v6r).max() < 1e-12
    sets = bc.make_loss_sets(3, 5)
    s64, _ = bc.loss_distances(MODEL, betas, sets, "6d", names=())
    rows = [torch.from_numpy(bc.feats_rows(s[2], s[1])) for s in sets]
    got = body.torch_loss_sums(m, betas, *rows, subject=np.arange(3), kind="6d", frames_per_pass=2).numpy()
    assert max(abs(got[i] - s64[i]) / s64[i] for i in range(2)) < 1e-12
    assert float(body.torch_loss_sums(m, betas, rows[0], rows[1], None, subject=np.arange(3), kind="6d")[1]) == 0.0
    rows_aa = [torch.from_numpy(bc.motion_rows(s[0], s[1])) for s in sets]
    s64aa, _ = bc.loss_distances(MODEL, betas, sets, "aa", names=())
    got = body.torch_loss_sums(m, betas, *rows_aa, subject=np.arange(3), kind="aa").numpy()
    assert max(abs(got[i] - s64aa[i]) / s64aa[i] for i in range(2)) < 1e-12


def _models():
    return {g: bc.make_model(V=37, seed=20 + i) for i, g in enumerate(("male", "female", "neutral"))}


ATTR = [("scott", "male"), ("miranda", "female"), ("wayne", "male"), ("sophie", "female")]


def _rs_set(seed=0):
    sets = bc.make_loss_sets(4, 3, seed=seed)
    g = torch.Generator().manual_seed(seed)
    rs = {"m_ref": torch.from_numpy(bc.feats_rows(sets[0][2], sets[0][1])), "m_rst": torch.from_numpy(bc.feats_rows(sets[1][2], sets[1][1])).requires_grad_(True),
          "gen_m_rst": torch.from_numpy(bc.feats_rows(sets[2][2], sets[2][1])), "noise": torch.randn(4, 1, 128, generator=g),
          "noise_pred": torch.randn(4, 1, 128, generator=g), "attr": ATTR}
    return sets, rs


@pytest.mark.parametrize("version", ["v0", "v1"])
def test_latent_prior_losses_with_body(version):
    """against latent_losses.py's arithmetic written out in float64: per gender (v0) or through the neutral model (v1) the three motions are posed with the actor's
    betas, SmoothL1 (mean over B F V 3) of (reconstruction, batch) and (generation, batch), weight LAMBDA_REC, inside `total`, no gradient"""
    from amuse_amd.train_gesture import LatentPriorLosses
    models = _models()
    bl = body.BodyLosses({g: body.BodyModel.from_dict(m) for g, m in models.items()}, "cpu", version=version)
    cfg = {"LAMBDA_KL": 0.0, "LAMBDA_REC": 0.7, "vtex_displacement": True}
    with pytest.raises(NotImplementedError):
        LatentPriorLosses(cfg)                                                # without body: as before
    L, L0 = LatentPriorLosses(cfg, "cpu", body=bl), LatentPriorLosses(dict(cfg, vtex_displacement=False))
    assert L.losses == ["inst_loss", "recons_feature", "recons_joints", "kl_motion", "gen_feature", "gen_joints", "rec_vtex_displacement", "gen_vtex_displacement", "total"]
    sets, rs = _rs_set()
    total, total0 = L.update(rs), L0.update(rs)
    # the restatement, clip by clip
    V = 37
    rec = gen = 0.0
    for n, (actor, gender) in enumerate(ATTR):
        mdl = models[gender if version == "v0" else "neutral"]
        b = npz_writer.fetchbetas(actor)[None].astype(np.float32)
        v = [br.forward(mdl, b, s[2][n:n + 1], s[1][n:n + 1], "6d")[1] for s in sets]
        rec, gen = rec + br.smooth_l1_sum(v[1], v[0]), gen + br.smooth_l1_sum(v[2], v[0])
    rec, gen = rec / (4 * 3 * V * 3), gen / (4 * 3 * V * 3)
    out = L.compute()
    assert abs(float(out["rec_vtex_displacement"]) - rec) < 2e-7 * rec and abs(float(out["gen_vtex_displacement"]) - gen) < 2e-7 * gen   # float32 scalars of float64 sums
    assert rec > 0 and gen > 0 and abs(rec - gen) > 1e-6
    assert abs(float(total) - (float(total0) + 0.7 * (np.float32(rec) + np.float32(gen)))) < 1e-6 * float(total)
    for k in L0.losses[:-1]:
        assert float(out[k]) == float(L0.compute()[k]), k                      # the other terms: untouched
    # no gradient flows through the vertex terms
    g, = torch.autograd.grad(total, rs["m_rst"], retain_graph=True)
    g0, = torch.autograd.grad(total0, rs["m_rst"])
    assert torch.equal(g, g0)
    # accumulated in place (a captured step holds on to these tensors), averaged by compute()
    ptr = L.sums["rec_vtex_displacement"].data_ptr()
    L.update(rs)
    assert L.sums["rec_vtex_displacement"].data_ptr() == ptr and abs(float(L.compute()["rec_vtex_displacement"]) - rec) < 2e-7 * rec
    # without a generation (a CPU run has no in-loop sampler) the generation term is 0
    L.reset()
    L.update(dict(rs, gen_m_rst=None))
    assert float(L.compute()["gen_vtex_displacement"]) == 0.0 and float(L.compute()["rec_vtex_displacement"]) > 0
    # the split as device data: one row per model, -1 where the clip is the other model's
    rows = bl.subject_rows(ATTR)
    assert rows.shape == ((2, 4) if version == "v0" else (1, 4))
    if version == "v0":
        assert (rows[0] >= 0).tolist() == [True, False, True, False] and ((rows[0] >= 0) ^ (rows[1] >= 0)).all()
    with pytest.raises(NotImplementedError, match="Actor not found"):
        bl.subject_rows([("nobody", "male")])


def test_feature_rows_vs_the_references_axis_angle_round_trip():
    """The stated deviation: the trainer poses the 6D rows directly; the reference converts them matrix -> axis-angle -> matrix first (float32).  Identity up to
    fp32 rounding: the vertices of the two agree to a few float32 ulps of a metre."""
    from oracle import amuse_oracle as orc
    _, tr, d6 = bc.make_motion(2, 4)
    betas = bc.make_betas(2)
    aa = orc.matrix_to_axis_angle(orc.rotation_6d_to_matrix(torch.from_numpy(d6))).numpy().astype(np.float32)
    v6 = br.forward(MODEL, betas, d6, tr, "6d")[1]
    va = br.forward(MODEL, betas, aa, tr, "aa")[1]
    assert np.abs(v6 - va).max() < 4e-6, np.abs(v6 - va).max()


def test_cli_smplx_models_directory(tmp_path):
    """`main.py --fn train_gesture` on an override with vtex_displacement: True - without the model files the SystemExit names the directory looked in; with them
    (default <root>/body_models/codebase/models/smplx or --smplx-models DIR) it trains with the terms on and the checkpoint names carry a real vtexR."""
    from conftest import make_reference_tree
    from amuse_amd import main as cli
    root = make_reference_tree(tmp_path / "tree")
    (root / "scripts/overrides/train_gesture.yaml").write_text(
        "TRAIN_PARAM:\n  latent_diffusion:\n    batch_size: 2\n    n_epochs: 1\n    model_save_freq: 1\n    vtex_displacement: True\n  diffusion:\n"
        "    lmdb_cache: BEAT-cache/2023-10-28_30F_fing_smplx_MOSH_identity_v1_feat_based_300\n")
    default = root / "body_models" / "codebase" / "models" / "smplx"
    run = ["--fn", "train_gesture", "--root", str(root), "--device", "cpu", "--synthetic", "--iters-per-epoch", "1"]
    with pytest.raises(SystemExit, match="vtex_displacement") as e:
        cli.main(run)
    assert str(default) in str(e.value)
    other = tmp_path / "models"
    with pytest.raises(SystemExit, match="vtex_displacement") as e:
        cli.main(run + ["--smplx-models", str(other)])
    assert str(other) in str(e.value)
    other.mkdir()
    for i, f in enumerate(body.SMPLX_FILES.values()):
        body.BodyModel.from_dict(bc.make_model(V=37, seed=30 + i)).to_npz(other / f)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(run + ["--smplx-models", str(other)]) == 0
    assert "vertex-displacement losses ON" in buf.getvalue() and "WARNING: vtex_displacement" not in buf.getvalue()
    names = [p.name for p in (root / "saved-models").glob("latdiff_model_wOpt_*_e1.pt")]
    assert len(names) == 1 and "_vtexR" in names[0] and "_vtexR0.0000" not in names[0], names
    # a dataset version the terms do not know is refused by name, not by an argparse usage error
    ov = (root / "scripts/overrides/train_gesture.yaml").read_text()
    (root / "scripts/overrides/train_gesture.yaml").write_text(ov + "  wav_dtw_mfcc:\n    ablation_version: v7\n")
    with pytest.raises(SystemExit, match="ablation_version"):
        cli.main(run + ["--smplx-models", str(other)])
    (root / "scripts/overrides/train_gesture.yaml").write_text(ov)
    # --skip-vtex-loss: as before
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(run + ["--skip-vtex-loss"]) == 0
    assert "WARNING: vtex_displacement" in buf.getvalue()
