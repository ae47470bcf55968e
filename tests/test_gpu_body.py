"""GPU: the SMPL-X body model in HIP (include/amuse_hip.h amuse_body_*, csrc/k_body.hip) through the C ABI's binding (amuse_amd/body.py BodyEngine, a ctypes
wrapper that adds nothing) against the float64 numpy RESTATEMENT of the published algorithm (tests/body_ref.py; `smplx` is not installed - this is no pin).

Bars, computed on the CPU in the same test from the same inputs (tests/body_cases.py forward_distances / loss_distances):
  forward, AMUSE_PREC_F32X   4 x max(d32, dx): d32 = the restatement in float32, dx = float32 with the split-fp16 pose-blend product; the factor covers summation order
  forward, AMUSE_PREC_F16    4 x d16 (the one-product form)
  loss sums                  relative, 4 x the float32 restatement's relative distance, floored at 2^-20 (16 fp32 ulps for the in-lane accumulation)"""
import numpy as np
import pytest
import torch

import body_cases as bc
import body_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -20


def _engine(model, betas, precision="fp32x"):
    from amuse_amd.body import BodyEngine, BodyModel
    eng = BodyEngine(DEV, BodyModel.from_dict(model), precision)
    eng.set_subjects(betas)
    return eng


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def small():
    model, betas = bc.make_model(203), bc.make_betas(3)
    eng = _engine(model, betas)
    yield model, betas, eng
    eng.close()


@pytest.fixture(scope="module")
def loss_case(small):
    """N = 3, F = 17 (across a 16-frame tile), both SmoothL1 branches; float64 sums and the float32 restatement's relative distance, computed once"""
    model, betas, _ = small
    sets = bc.make_loss_sets(3, 17)
    s64, d = bc.loss_distances(model, betas, sets, "aa", names=("r32",))
    return sets, s64, max(4 * d["r32"], FLOOR)


@pytest.mark.parametrize("V", [203, 208])
@pytest.mark.parametrize("F", [5, 17])
def test_forward_vs_restatement(small, F, V):
    model, betas, eng = small if V == 203 else (bc.make_model(V, seed=5), bc.make_betas(3), None)
    own = eng is None
    if own:
        eng = _engine(model, betas)
    aa, tr, d6 = bc.make_motion(3, F, seed=10 + F)
    j64, v64, d = bc.forward_distances(model, betas, aa, tr)
    sub = _dev(np.arange(3), torch.int32)
    j_aa, v_aa = eng.forward(_dev(aa), _dev(tr), sub, "aa")
    for prec, bar in (("fp32x", 4 * max(d["d32"], d["dx"])), ("fp16", 4 * d["d16"])):
        j, v = eng.forward(_dev(aa), _dev(tr), sub, "aa", precision=prec)
        ev, ej = float(np.abs(v.cpu().numpy() - v64).max()), float(np.abs(j.cpu().numpy() - j64).max())
        print(f"V {V} F {F} {prec}: vertices {ev:.3e} joints {ej:.3e} bar {bar:.3e}  (d32 {d['d32']:.3e} dx {d['dx']:.3e} dx without pre-scale {d['dx_noscale']:.3e} d16 {d['d16']:.3e})")
        assert ev <= bar and ej <= bar, (prec, ev, ej, bar)
    # 6D input of the same rotations: within the same bar of the restatement, joints-only and vertices-only calls give the bits of the joint call
    bar = 4 * max(d["d32"], d["dx"])
    rows = _dev(bc.feats_rows(d6, tr))
    j6, v6 = eng.forward(rows, None, sub, "6d")
    assert float(np.abs(v6.cpu().numpy() - v64).max()) <= bar and float(np.abs(j6.cpu().numpy() - j64).max()) <= bar
    e6 = float((v6 - v_aa).abs().max()), float((j6 - j_aa).abs().max())                   # ... and the two GPU results within the forward bar of EACH OTHER
    print(f"V {V} F {F}: 6D vs axis-angle input, vertices {e6[0]:.3e} joints {e6[1]:.3e} bar {bar:.3e}")
    assert max(e6) <= bar, (e6, bar)
    assert torch.equal(eng.joints(rows, None, sub, "6d"), j6) and torch.equal(eng.vertices(rows, None, sub, "6d"), v6)
    if own:
        eng.close()


def test_loss_sums(small, loss_case):
    model, betas, eng = small
    sets, s64, bar = loss_case
    sub = _dev(np.arange(3), torch.int32)
    rows = [_dev(bc.motion_rows(s[0], s[1])) for s in sets]
    got = eng.vertex_loss(*rows, subject=sub, kind="aa").cpu().numpy()
    rel = [abs(got[i] - s64[i]) / s64[i] for i in range(2)]
    print(f"fused sums {got} float64 {s64} relative {rel} bar {bar:.3e}")
    assert max(rel) <= bar
    # both SmoothL1 branches are reached (clip 0 of the first candidate is 1.5 m off)
    v = [eng.vertices(_dev(s[0]), _dev(s[1]), sub, "aa").double() for s in sets]
    assert bool(((v[1] - v[0]).abs() > 1).any()) and bool(((v[1] - v[0]).abs() < 1).any())
    # the same sums formed on the host from vertices_out of the same context
    host = [float(torch.nn.functional.smooth_l1_loss(v[i], v[0], reduction="sum")) for i in (1, 2)]
    assert max(abs(got[i] - host[i]) / host[i] for i in range(2)) <= bar, (got, host)
    # 6D rows of the same motions
    rows6 = [_dev(bc.feats_rows(s[2], s[1])) for s in sets]
    got6 = eng.vertex_loss(*rows6, subject=sub, kind="6d").cpu().numpy()
    assert max(abs(got6[i] - s64[i]) / s64[i] for i in range(2)) <= bar, (got6, s64)
    # b = NULL
    out = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    eng.vertex_loss(rows[0], rows[1], None, sub, "aa", out=out)
    assert float(out[1]) == 0.0 and abs(float(out[0]) - s64[0]) / s64[0] <= bar   # (the two-set instantiation: another build of the same arithmetic)
    # the one-product form against ITS emulation's distance
    _, d = bc.loss_distances(model, betas, sets, "aa", names=("r16",))
    got16 = eng.vertex_loss(*rows, subject=sub, kind="aa", precision="fp16").cpu().numpy()
    assert max(abs(got16[i] - s64[i]) / s64[i] for i in range(2)) <= max(4 * d["r16"], FLOOR), (got16, s64, d)


def test_real_vertex_count_loss():
    """V = 10,475 (SMPL-X's), N = 2, F = 300, loss mode only: the indexing at the product's size without 3.6 GB of vertices.  The 300 frames of a clip repeat a
    period of 20 distinct frames, so the float64 restatement poses 40 frames, not 600 (its sums times 15); the GPU poses all 600 - a frame, tile or chunk index gone
    wrong reads another phase of the period (20 against tiles of 16) and moves the sums."""
    model, betas = bc.make_model(10475, seed=7), bc.make_betas(2, seed=8)
    period = bc.make_loss_sets(2, 20, seed=9)
    s64, d = bc.loss_distances(model, betas, period, "aa", frames_per_pass=20, names=("r32",))
    s64 = [15 * x for x in s64]
    bar = max(4 * d["r32"], FLOOR)
    eng = _engine(model, betas)
    rows = [_dev(np.tile(bc.motion_rows(s[0], s[1]), (1, 15, 1))) for s in period]
    assert rows[0].shape == (2, 300, 168)
    got = eng.vertex_loss(*rows, subject=_dev(np.arange(2), torch.int32), kind="aa").cpu().numpy()
    eng.close()
    rel = [abs(got[i] - s64[i]) / s64[i] for i in range(2)]
    print(f"V 10475: fused sums {got} float64 {s64} relative {rel} bar {bar:.3e}")
    assert max(rel) <= bar


def test_bitwise_properties(small):
    model, betas, eng = small
    aa, tr, d6 = bc.make_motion(3, 17, seed=21)
    sub = _dev(np.arange(3), torch.int32)
    j, v = eng.forward(_dev(aa), _dev(tr), sub, "aa")
    j2, v2 = eng.forward(_dev(aa), _dev(tr), sub, "aa")
    assert torch.equal(j, j2) and torch.equal(v, v2)                                     # the same call twice
    j1, v1 = eng.forward(_dev(aa[1:2]), _dev(tr[1:2]), sub[1:2].contiguous(), "aa")       # a clip alone == its rows in the batch
    assert torch.equal(j1[0], j[1]) and torch.equal(v1[0], v[1])
    perm = [2, 0, 1]                                                                      # permuting subject_dev permutes the results
    same = np.repeat(aa[:1], 3, 0), np.repeat(tr[:1], 3, 0)
    ja, va = eng.forward(_dev(same[0]), _dev(same[1]), sub, "aa")
    jb, vb = eng.forward(_dev(same[0]), _dev(same[1]), _dev(np.array(perm), torch.int32), "aa")
    assert torch.equal(jb, ja[perm]) and torch.equal(vb, va[perm]) and not torch.equal(va[0], va[1])
    sets = bc.make_loss_sets(3, 17)
    rows = [_dev(bc.motion_rows(s[0], s[1])) for s in sets]
    assert torch.equal(eng.vertex_loss(*rows, subject=sub, kind="aa"), eng.vertex_loss(*rows, subject=sub, kind="aa"))


def test_graph_replay_follows_device_inputs(small):
    """a captured single-stream graph of the loss call == the eager call, and a replay after the device inputs were overwritten follows them"""
    model, betas, eng = small
    sets, other = bc.make_loss_sets(3, 17), bc.make_loss_sets(3, 17, seed=33)
    rows = [_dev(bc.motion_rows(s[0], s[1])) for s in sets]
    rows2 = [_dev(bc.motion_rows(s[0], s[1])) for s in other]
    sub, sub2 = _dev(np.arange(3), torch.int32), _dev(np.array([1, 2, 0]), torch.int32)
    eager = eng.vertex_loss(*rows, subject=sub, kind="aa").clone()
    eager2 = eng.vertex_loss(*rows2, subject=sub2, kind="aa").clone()
    buf = [r.clone() for r in rows]
    sbuf, out = sub.clone(), torch.zeros(2, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.vertex_loss(*buf, subject=sbuf, kind="aa", out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    for b, r in zip(buf, rows2):
        b.copy_(r)
    sbuf.copy_(sub2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2) and not torch.equal(eager, eager2)


def test_argument_checks(small):
    from amuse_amd import _lib
    model, betas, eng = small
    lib = _lib.load()
    x = torch.zeros(1, 2, 168, device=DEV)
    sub = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    assert lib.amuse_body_vertex_loss(eng.ctx, x.data_ptr(), x.data_ptr(), None, 0, sub.data_ptr(), 1, 2, _lib.PREC_F32, out.data_ptr(), None) == -1   # AMUSE_EINVAL
    assert lib.amuse_body_vertex_loss(eng.ctx, x.data_ptr(), x.data_ptr(), None, 0, sub.data_ptr(), 1, 2, _lib.PREC_BF16, out.data_ptr(), None) == -1
    assert lib.amuse_body_vertex_loss(eng.ctx, x.data_ptr(), x.data_ptr(), None, 5, sub.data_ptr(), 1, 2, _lib.PREC_F32X, out.data_ptr(), None) == -1
    bad = dict(model, parents=model["parents"].copy())
    bad["parents"][5] = 9
    from amuse_amd.body import BodyModel
    with pytest.raises(ValueError, match="parents"):
        BodyModel.from_dict(bad)


def test_trainer_iteration_with_body():
    """One iteration of the GPU trainer with body= (batch 2, a male and a female actor, synthetic models): rec_ / gen_vtex_displacement against the CPU twin of the
    same step (the float64 torch twin on the very motions the step handed over) within the loss bar's floor - never wider than max(4 r32, 2^-20) - and the other
    loss terms bitwise what they are without body.  Then the step captured as HIP graphs: a replay on a batch with the genders swapped follows it."""
    from amuse_amd import body
    from amuse_amd.train_gesture import build_trainer, synthetic_batch
    models = {g: body.BodyModel.from_dict(bc.make_model(203, seed=40 + i)) for i, g in enumerate(("male", "female"))}
    attr = [("scott", "male"), ("miranda", "female")]
    batch = dict(synthetic_batch(2, 3, DEV), ld_attr=attr)
    g = torch.Generator().manual_seed(0)
    draws = dict(noise=torch.randn(2, 1, 128, generator=g).to(DEV), timesteps=torch.randint(0, 1000, (2,), generator=g).to(DEV),
                 eps_enc=torch.randn(1, 2, 128, generator=g).to(DEV), eps_inf=torch.randn(1, 2, 128, generator=g).to(DEV))
    got, seen = {}, {}
    for with_body in (True, False):
        bl = body.BodyLosses(models, DEV, "v0") if with_body else None
        torch.manual_seed(7)                      # (whatever the step draws from torch's generator is the same in both runs)
        tr = build_trainer(DEV, seed=2, dropout=0.0, body=bl)
        if with_body:
            inner = bl.terms
            def spy(m_ref, m_rst, gen, attr_, subjects, inner=inner):
                seen.update(ref=m_ref.detach().cpu(), rst=m_rst.detach().cpu(), gen=gen.detach().cpu())
                return inner(m_ref, m_rst, gen, attr_, subjects)
            bl.terms = spy
        for m in tr.model.values():
            m.train()
        loss = tr.forward_losses(batch, **draws)
        torch.cuda.synchronize()
        got[with_body] = ({k: v.clone() for k, v in tr.lpdm_losses.sums.items()}, loss.detach().clone())
        if with_body:
            bl.terms = inner
            keep = (tr, bl)
    (sb, lb), (s0, l0) = got[True], got[False]
    for k in s0:
        if k != "total":
            assert torch.equal(sb[k], s0[k]), k
    rec, gen = body.BodyLosses(models, "cpu", "v0").terms(seen["ref"], seen["rst"], seen["gen"], attr)
    for name, want in (("rec_vtex_displacement", rec), ("gen_vtex_displacement", gen)):
        rel = abs(float(sb[name]) - float(want)) / float(want)
        print(f"{name}: GPU {float(sb[name]):.9g} CPU twin {float(want):.9g} relative {rel:.3e} bar {FLOOR:.3e}")
        assert float(want) > 0 and rel <= FLOOR
    assert abs(float(lb) - (float(l0) + float(sb["rec_vtex_displacement"]) + float(sb["gen_vtex_displacement"]))) <= 1e-6 * abs(float(lb))   # LAMBDA_REC 1, inside total
    # captured: replays follow the batch's actors (the split is device data)
    tr, bl = keep
    for i in range(3):
        tr.train_step(batch)
    assert tr.enable_graph(batch)
    tr.lpdm_losses.reset()
    tr.train_step(batch)
    torch.cuda.synchronize()
    a = float(tr.lpdm_losses.sums["rec_vtex_displacement"])
    assert a > 0 and np.isfinite(a)
    swapped = dict(batch, ld_attr=[("miranda", "female"), ("scott", "male")])
    tr.train_step(swapped)
    torch.cuda.synchronize()
    assert tr._graph["static"]["ld_subjects"].cpu().tolist() == bl.subject_rows(swapped["ld_attr"]).tolist()
    assert np.isfinite(float(tr.lpdm_losses.sums["total"])) and float(tr.lpdm_losses.sums["rec_vtex_displacement"]) > a
    # the terms themselves, captured with the split as a device buffer: a replay after the buffer was overwritten with the swapped genders gives the swapped batch's
    # values (the float64 twin's, and the eager call's bits), not the captured batch's
    dev3 = [seen[k].to(DEV) for k in ("ref", "rst", "gen")]
    sbuf = bl.subjects(attr)
    eager = [torch.stack(bl.terms(*dev3, None, bl.subjects(x))).clone() for x in (attr, swapped["ld_attr"])]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = torch.stack(bl.terms(*dev3, None, sbuf))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0])
    sbuf.copy_(bl.subjects(swapped["ld_attr"]))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1]) and not torch.equal(eager[0], eager[1])
    want = body.BodyLosses(models, "cpu", "v0").terms(seen["ref"], seen["rst"], seen["gen"], swapped["ld_attr"])
    for i in range(2):
        rel = abs(float(out[i]) - float(want[i])) / float(want[i])
        print(f"replay on the swapped genders, term {i}: {float(out[i]):.9g} float64 twin {float(want[i]):.9g} relative {rel:.3e} bar {FLOOR:.3e}")
        assert rel <= FLOOR
    bl.close()


def test_poser_matches_a_hand_driven_engine(tmp_path):
    """body.Poser on motion_file.read records against BodyEngine driven by hand as beat_align.score_pairs drove it before there was a Poser - bit for bit: two
    files of two genders and lengths, stored betas one short of and one past the model's 300, the first file again after the other subject was set."""
    from amuse_amd import body, motion_file
    models = {g: body.BodyModel.from_dict(bc.make_model(V=203, n_betas=300, seed=s)) for g, s in (("male", 0), ("female", 7))}
    files = []
    for k, (g, F, nb) in enumerate((("male", 2, 299), ("female", 3, 301))):
        aa, tr, _ = bc.make_motion(1, F, seed=40 + k)
        files.append(tmp_path / f"{g}_motion_smplx.npz")
        np.savez(files[-1], poses=aa[0].reshape(F, 165), trans=tr[0].astype(np.float64), gender=np.array(g, dtype="<U7"),
                 betas=np.random.default_rng(50 + k).standard_normal(nb) * 0.5, mocap_frame_rate=np.array(30.0))

    def by_hand(path, engines):
        with np.load(path, allow_pickle=False) as z:
            g = str(z["gender"])
            poses, trans, betas = np.asarray(z["poses"], np.float32), np.asarray(z["trans"], np.float32), np.asarray(z["betas"], np.float32)
        F, n = int(poses.shape[0]), models[g].n_betas
        if g not in engines:
            engines[g] = body.BodyEngine(DEV, models[g])
        engines[g].set_subjects(np.pad(betas.reshape(-1)[:n], (0, max(0, n - betas.size)))[None])
        return engines[g].joints(torch.from_numpy(poses.reshape(1, F, 55, 3)).to(DEV).contiguous(), torch.from_numpy(trans.reshape(1, F, 3)).to(DEV).contiguous(),
                                 torch.zeros(1, dtype=torch.int32, device=DEV), "aa").clone()

    order = [files[0], files[1], files[0]]
    hand = {}
    want = [by_hand(p, hand) for p in order]
    for e in hand.values():
        e.close()
    poser = body.Poser(models, DEV)
    got = []
    for p in order:
        eng, rot, tr = poser.pose(motion_file.read(p))
        assert tuple(rot.shape) == (1, rot.shape[1], 55, 3) and tuple(tr.shape) == (1, rot.shape[1], 3) and rot.is_cuda and eng.n_subjects == 1
        got.append(eng.joints(rot, tr).clone())
    torch.cuda.synchronize()
    assert [tuple(j.shape) for j in got] == [(1, 2, 55, 3), (1, 3, 55, 3), (1, 2, 55, 3)]
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(got[0], got[2]) and bool(torch.isfinite(got[1]).all())
    engines = list(poser.engines.values())
    assert len(engines) == 2
    poser.close()
    assert poser.engines == {} and all(e.ctx is None for e in engines)
