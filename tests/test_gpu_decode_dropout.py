"""GPU: train-mode decode (amuse_set_decode_dropout) - the six dropouts of every MotionPrior.decode block live inside the staged HIP decode kernels.

The mask contract is restated in tests/test_decode_dropout_cpu.py (decode_restated: the oracle's decoder arithmetic with the six sites, masks from
philox4x32_10), which the CPU suite holds to the reference's own module (tests/golden/decode_dropout.npz).  Here the kernels are held to that fixture
and to the restatement.  Bars that are measured rather than fixed follow one rule: twice the distance that is there without dropout - the same kernel's
p = 0 error in the same run, or the restatement's own distance to the reference module - because the masks select and scale (1 / (1 - p) = 1.11 per
site) values whose fp32 summation order is the only difference left; never above the 2e-5 the eval decode is given."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_decode_dropout_cpu as R  # noqa: E402  (the restatement; its tests need no GPU)

pytestmark = pytest.mark.gpu

P = 0.1
SEED = 0x0BAD_5EED_1234_5678
STAGED, FUSED = 1, 2


def _weights():
    from amuse_amd import weights as wts
    from oracle import amuse_oracle as orc
    wd, wp = wts.make_denoiser_weights(0), wts.make_prior_weights(0)
    return wd, wp, orc.to_torch(wp)


def _engine(wd, wp):
    from amuse_amd import scheduler as sch
    from amuse_amd.engine import HipEngine
    eng = HipEngine(wd, wp, "cuda:0")
    eng.set_schedule(sch.ddim_table())
    return eng


def _epoch_set(eng, k):
    from amuse_amd import _lib
    _lib.check(eng.lib.amuse_train_epoch_set(int(k), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _z(B, seed):
    return torch.randn(B, 128, generator=torch.Generator().manual_seed(seed))


def _feats(eng, z, lengths=None, prec="fp32"):
    return eng.vae_decode(z, lengths, prec, return_feats=True)["feats"].cpu()


def _restatement_distance_to_reference(Wp):
    """the CPU restatement against the reference module's fixture (what tests/test_decode_dropout_cpu.py asserts below 2e-5), full case"""
    cases, m = R.fixture_cases()
    name, lengths, expect = cases[0]
    return R.fixture_distance(R.decode_restated(Wp, m["z"], lengths, R.Masks(m["seed"], m["clips"], m["epoch"], m["p"])).numpy(), expect)


# ---- 1. eval unchanged ---------------------------------------------------------------------------------------------------------------
def test_p0_after_dropout_is_bitwise_the_eval_decode():
    wd, wp, _ = _weights()
    z = _z(70, 3)                           # 70 clips: AUTO takes the fused per-clip kernel in the 16-bit modes
    fresh, eng = _engine(wd, wp), _engine(wd, wp)
    for prec in ("fp32", "bf16", "fp16"):
        for path in ("auto", "staged", "fused"):
            fresh.set_decode_path(path), eng.set_decode_path(path)
            ref = fresh.vae_decode(z, None, prec, return_feats=True)
            eng.set_decode_dropout(P, SEED, 5)
            assert not torch.equal(eng.vae_decode(z, None, prec, return_feats=True)["feats"], ref["feats"]), (prec, path)
            eng.set_decode_dropout(0.0, SEED, 5)
            out = eng.vae_decode(z, None, prec, return_feats=True)
            for k in ("feats", "poses", "trans"):
                assert torch.equal(out[k], ref[k]), (prec, path, k)
    fresh.close(), eng.close()


# ---- 2. fp32 against the reference's own module --------------------------------------------------------------------------------------
def test_fp32_matches_the_reference_module_fixture():
    """Measured on one MI355X: kernel p = 0 against vae_decode.npz 2.4e-6, restatement against the fixture 2.1e-6 (that box's CPU; 1.9e-6 on the build machine)
    -> bar 4.8e-6; the dropout decode against decode_dropout.npz: full 2.5e-6, ragged 2.6e-6."""
    wd, wp, Wp = _weights()
    eng = _engine(wd, wp)
    g0 = np.load(R.GOLDEN / "vae_decode.npz")
    e0 = float(np.abs(_feats(eng, torch.from_numpy(g0["z"])).numpy() - g0["feats"]).max())
    r0 = _restatement_distance_to_reference(Wp)
    bar = min(2.0 * max(e0, r0), 2e-5)
    print(f"fp32 staged decode, p = 0, against vae_decode.npz: {e0:.3e}; CPU restatement against decode_dropout.npz: {r0:.3e}; bar {bar:.3e}")
    assert e0 < 2e-5 and r0 < 2e-5
    cases, m = R.fixture_cases()
    _epoch_set(eng, m["epoch"])
    worst = {}
    try:
        for name, lengths, expect in cases:
            feats = torch.empty(3, 300, 333)
            # the stored clip indices are not consecutive: clips 0, 1 as one call (base 7), clip 2 on its own (base 4096) - a clip's result does not depend on its batch
            for sl, base in ((slice(0, 2), m["clips"][0]), (slice(2, 3), m["clips"][2])):
                eng.set_decode_dropout(m["p"], m["seed"], base)
                feats[sl] = _feats(eng, m["z"][sl], None if lengths is None else lengths[sl])
            worst[name] = R.fixture_distance(feats.numpy(), expect)
            print(f"fp32 dropout decode against the reference module ({name}): {worst[name]:.3e}")
            if lengths is not None:
                for b, n in enumerate(lengths):
                    assert bool((feats[b, n:] == 0).all())
    finally:
        _epoch_set(eng, 0)
    for name, d in worst.items():
        assert d <= bar, (name, d, bar)
    eng.close()


# ---- 3. fp32 against the restatement on fresh inputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ragged", [(1, False), (17, True), (70, False)])
def test_fp32_matches_the_restatement(B, ragged):
    """B = 1, 17, 70: tile, workgroup and chunk boundaries.  Bar: twice the larger of the same kernel's p = 0 distance to the oracle on the same latents and the
    restatement's distance to the reference module (1.9e-6), at most 2e-5."""
    from oracle import amuse_oracle as orc
    wd, wp, Wp = _weights()
    z = _z(B, 100 + B)
    lengths = None
    if ragged:
        lengths = [int(v) for v in np.random.default_rng(B).integers(1, 301, size=B)]
        lengths[0], lengths[1], lengths[2] = 300, 1, 33
    eng = _engine(wd, wp)
    e0 = float((_feats(eng, z, lengths) - orc.vae_decode(Wp, z, lengths)).abs().max())
    bar = min(2.0 * max(e0, 1.9e-6), 2e-5)
    c0, epoch = 1000 + B, 2
    _epoch_set(eng, epoch)
    try:
        eng.set_decode_dropout(P, SEED, c0)
        got = _feats(eng, z, lengths)
    finally:
        _epoch_set(eng, 0)
    ref = R.decode_restated(Wp, z, lengths, R.Masks(SEED, c0 + np.arange(B), epoch, P))
    d = float((got - ref).abs().max())
    print(f"B = {B}{' ragged' if ragged else ''}: p = 0 kernel vs oracle {e0:.3e}, dropout kernel vs restatement {d:.3e}, bar {bar:.3e}")
    assert d <= bar, (d, bar)
    assert float((got - orc.vae_decode(Wp, z, lengths)).abs().max()) > 0.1        # (the masks matter)
    eng.close()


# ---- 4. bf16 / fp16 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_decode_follows_its_own_masks(prec):
    """The distance to the restatement with the right masks (in the oracle's 16-bit emulation) is at most 0.25 of the distance with the clip indices shifted by one
    (the ratio of test_gpu_sample_dropout.py::test_16bit_step_follows_its_own_masks) and at most twice the same staged kernel's p = 0 distance to the emulating
    oracle in the same run."""
    from oracle import amuse_oracle as orc
    wd, wp, Wp = _weights()
    B = 6
    z = _z(B, 41)
    eng = _engine(wd, wp)
    eng.set_decode_path("staged")
    e0 = float((_feats(eng, z, None, prec) - orc.vae_decode(Wp, z, None, emulate_bf16=prec == "bf16", fp16=prec == "fp16")).abs().max())
    _epoch_set(eng, 0)
    eng.set_decode_dropout(P, SEED, 20)
    got = _feats(eng, z, None, prec)
    right = R.decode_restated(Wp, z, None, R.Masks(SEED, 20 + np.arange(B), 0, P), emulate=prec)
    wrong = R.decode_restated(Wp, z, None, R.Masks(SEED, 21 + np.arange(B), 0, P), emulate=prec)
    e_right, e_wrong = float((got - right).abs().max()), float((got - wrong).abs().max())
    print(f"{prec}: p = 0 kernel vs emulating oracle {e0:.3e}; dropout kernel vs right masks {e_right:.3e}, vs shifted masks {e_wrong:.3e}")
    assert e_right <= 0.25 * e_wrong, (e_right, e_wrong)
    assert e_right <= 2.0 * e0, (e_right, e0)
    eng.close()


# ---- 5. keying -----------------------------------------------------------------------------------------------------------------------
def test_masks_are_keyed_by_seed_clip_base_and_epoch():
    wd, wp, _ = _weights()
    B = 50                                  # (above 48 clips the 16-bit attention launches one workgroup per (clip, head); a single clip launches five)
    z = _z(B, 51)
    eng = _engine(wd, wp)
    _epoch_set(eng, 0)
    for prec in ("fp32", "bf16", "fp16"):
        eng.set_decode_dropout(P, SEED, 9)
        a = _feats(eng, z, None, prec)
        assert torch.equal(_feats(eng, z, None, prec), a), prec
        eng.set_decode_dropout(P, SEED + 1, 9)
        assert not torch.equal(_feats(eng, z, None, prec), a), prec
        eng.set_decode_dropout(P, SEED, 10)
        b = _feats(eng, z, None, prec)
        assert not torch.equal(b, a) and torch.equal(b[1:], _feats_at(eng, z[1:], prec, 11)), prec      # (the same global clips from another call)
        eng.set_decode_dropout(P, SEED, 9)
        _epoch_set(eng, 4)
        assert not torch.equal(_feats(eng, z, None, prec), a), prec
        _epoch_set(eng, 0)
        assert torch.equal(_feats(eng, z, None, prec), a), prec
        # clip c alone (B = 1, clip base c) is row c of the batch, bitwise
        for c in (0, 17, B - 1):
            eng.set_decode_dropout(P, SEED, 9 + c)
            assert torch.equal(_feats(eng, z[c:c + 1], None, prec)[0], a[c]), (prec, c)
    eng.close()


def _feats_at(eng, z, prec, base):
    eng.set_decode_dropout(P, SEED, base)
    return _feats(eng, z, None, prec)


# ---- 6. diffusion_backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_diffusion_backward_is_sample_then_decode(prec):
    wd, wp, _ = _weights()
    B, c0 = 5, 77
    g = torch.Generator().manual_seed(61)
    con, emo, sty, x = (torch.randn(B, n, generator=g) for n in (256, 256, 256, 128))
    eng = _engine(wd, wp)
    _epoch_set(eng, 1)
    try:
        eng.set_sample_dropout(P, SEED + 7)
        eng.set_decode_dropout(P, SEED, 123456)          # (the setter's base must NOT be used inside diffusion_backward)
        out = eng.diffusion_backward(con, emo, sty, prec, clip_index0=c0, x_init=x)
        lat = eng.sample(con, emo, sty, prec, clip_index0=c0, x_init=x)
        assert torch.equal(out["latents"], lat)
        eng.set_decode_dropout(P, SEED, c0)
        dec = eng.vae_decode(lat, None, prec)
        assert torch.equal(out["poses"], dec["poses"]) and torch.equal(out["trans"], dec["trans"])
        eng.set_decode_dropout(P, SEED, c0 + 1)
        assert not torch.equal(eng.vae_decode(lat, None, prec)["poses"], out["poses"])
        # the decode switch alone: the sampler stays in eval mode
        eng.set_sample_dropout(0.0, 0)
        eng.set_decode_dropout(0.0, 0, 0)
        lat_eval = eng.sample(con, emo, sty, prec, clip_index0=c0, x_init=x)
        eng.set_decode_dropout(P, SEED, 0)
        assert torch.equal(eng.sample(con, emo, sty, prec, clip_index0=c0, x_init=x), lat_eval)
    finally:
        _epoch_set(eng, 0)
    eng.close()


# ---- 7. rejects and the plan ---------------------------------------------------------------------------------------------------------
def test_refusals_and_the_reported_plan():
    from amuse_amd import _lib
    from amuse_amd import scheduler as sch
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    wd, wp, _ = _weights()
    eng = _engine(wd, wp)
    p = lambda t: C.c_void_p(t.data_ptr())
    z = _z(4, 71).cuda()
    g = torch.Generator().manual_seed(72)
    con, emo, sty, x = (torch.randn(4, n, generator=g).cuda() for n in (256, 256, 256, 128))
    eng.set_decode_dropout(P, SEED, 0)
    poses = torch.full((4, 300, 55, 3), 7.0, device="cuda:0")
    trans = torch.full((4, 300, 3), 7.0, device="cuda:0")
    lat = torch.full((4, 128), 7.0, device="cuda:0")
    rc = eng.lib.amuse_vae_decode(eng.ctx, p(z), None, 4, 2, 0, None, p(poses), p(trans), eng._stream())                 # 2 = AMUSE_PREC_F32X
    rc2 = eng.lib.amuse_diffusion_backward(eng.ctx, p(con), p(emo), p(sty), 4, 2, 0, 0, 0, p(x), None, p(lat), p(poses), p(trans), eng._stream())
    torch.cuda.synchronize()
    assert rc == -4 and rc2 == -4                                                                                         # AMUSE_ESTATE
    assert bool((poses == 7.0).all()) and bool((trans == 7.0).all()) and bool((lat == 7.0).all())                          # nothing launched, not even the sampler
    with pytest.raises(_lib.AmuseHipError):
        eng.vae_decode(z, None, "fp32x")
    # the sampler, the encode and the teacher-forced step do not care
    eng.sample(con, emo, sty, "fp32x", x_init=x)
    eng.set_decode_dropout(0.0, 0, 0)
    assert bool(torch.isfinite(eng.vae_decode(z, None, "fp32x")["poses"]).all())
    # the plan: a 256-clip bf16 decode takes the fused kernel, the dropout decode the staged family whatever the pin says
    zz = _z(256, 73).cuda()
    plan = C.c_int(0)
    for pin in ("auto", "fused"):
        eng.set_decode_path(pin)
        eng.set_decode_dropout(P, SEED, 0)
        eng.vae_decode(zz, None, "bf16")
        _lib.check(eng.lib.amuse_debug_last_plan(eng.ctx, None, C.byref(plan), None, None))
        assert plan.value == STAGED, pin
        eng.set_decode_dropout(0.0, SEED, 0)
        eng.vae_decode(zz, None, "bf16")
        _lib.check(eng.lib.amuse_debug_last_plan(eng.ctx, None, C.byref(plan), None, None))
        assert plan.value == FUSED, pin
    eng.close()
    # a context without a prior
    ev = HipEngine(wts.make_denoiser_weights(0, "trans_enc", True), None, "cuda:0", arch="trans_enc", diffusion_only=True)
    ev.set_schedule(sch.ddim_table())
    ev.set_decode_dropout(P, SEED, 0)
    rc = ev.lib.amuse_vae_decode(ev.ctx, p(z), None, 4, 0, 0, None, p(poses), p(trans), ev._stream())
    assert rc == -4
    ev.close()


# ---- 8. graph replay -----------------------------------------------------------------------------------------------------------------
def test_captured_decode_draws_fresh_masks_through_the_epoch():
    from amuse_amd import _lib
    wd, wp, _ = _weights()
    z = _z(32, 81).cuda()
    eng = _engine(wd, wp)
    eng.set_decode_dropout(P, SEED, 3)
    _epoch_set(eng, 0)
    dec = lambda: eng.vae_decode(z, None, "bf16", return_feats=True)["feats"]
    dec()                                   # eager first: workspaces and the epoch word exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(eng.lib.amuse_train_epoch_advance(1, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        out = dec()
    _epoch_set(eng, 0)
    replays = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    assert not torch.equal(replays[0], replays[1])
    for k in range(2):
        _epoch_set(eng, k + 1)              # (the advance is captured in front of the decode)
        assert torch.equal(dec(), replays[k]), k
    _epoch_set(eng, 0)
    del g
    eng.close()


# ---- 9. the trainer ------------------------------------------------------------------------------------------------------------------
def test_trainer_with_the_train_mode_hip_decode():
    from amuse_amd.train_gesture import HipInnerSampler, build_trainer, synthetic_batch
    torch.manual_seed(0)
    tr = build_trainer("cuda:0", inner="train-hip-decode")
    s = tr.inner_sampler
    assert isinstance(s, HipInnerSampler) and s.dropout == pytest.approx(0.1) and s.hip_decode and not s.decode_on_trainer_stream
    assert not getattr(s, "serial", False) and s.mode == "train-hip-decode"
    batch = synthetic_batch(32, 3, "cuda:0")
    for _ in range(3):
        loss = float(tr.train_step(batch))
        ld = {k: float(v) for k, v in tr.lpdm_losses.compute().items()}
        assert np.isfinite(loss) and np.isfinite(ld["gen_feature"]) and ld["gen_feature"] > 0
    seen = []
    dec = s.decode
    s.decode = lambda lat: (seen.append(dec(lat)), seen[-1])[1]
    assert tr.enable_graph(batch)
    s.decode = dec
    assert len(seen) == 1
    outs = []
    for _ in range(2):
        assert np.isfinite(float(tr.train_step(batch)))
        torch.cuda.synchronize()
        outs.append(seen[0].clone())
    assert bool(torch.isfinite(outs[0]).all()) and not torch.equal(outs[0], outs[1])
