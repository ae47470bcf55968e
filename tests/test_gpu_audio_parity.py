"""GPU: the parity mode of the audio front-end (amuse_audio_set_precision AMUSE_PREC_F32X: split-fp16 operands, fp32 everything else) through the
C ABI against oracle/audio_oracle.py in fp32.  Parity stays UNPINNED for this path in the project's sense (timm / torchaudio absent: the yardstick is
the restated oracle, cross-checked against transformers.ASTModel on the CPU side) - what is new is the size of the bar: 1e-5, derived in
tests/test_audio_split_emulation_cpu.py (emulated 2.5e-6), where the bf16 front-end measures 5e-3.  Weights make_ast_weights(0, *), the signals of
tests/test_gpu_audio.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _waves(n, B=2, seed=0):   # tests/test_gpu_audio.py
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32) / 16000.0
    base = 0.2 * torch.sin(2 * np.pi * 220.0 * t) + 0.1 * torch.sin(2 * np.pi * 1900.0 * t)
    return torch.stack([base * (0.5 + 0.5 * i) + 0.05 * torch.randn(n, generator=g) for i in range(B)])


@pytest.fixture(scope="module")
def env():
    from amuse_amd import audio_weights as aw
    from amuse_amd.audio import AudioEngine
    from oracle import audio_oracle as ao
    W = {n: aw.make_ast_weights(0, n) for n in aw.ENCODERS}
    eng = AudioEngine(W["con"], W["emo"], W["sty"], "cuda:0")
    yield {"eng": eng, "Wnp": W, "W": {n: ao.to_torch(W[n]) for n in W}, "ao": ao}
    eng.close()


@pytest.fixture
def fp32x(env):
    """the module's engine in the parity mode for one test, back in bf16 afterwards"""
    env["eng"].set_precision("fp32x")
    yield env["eng"]
    env["eng"].set_precision("bf16")


# ------------------------------------------------------------------------------------------------ (a) encoder parity
@pytest.mark.parametrize("n_samples", [60000, 159744])
@pytest.mark.parametrize("which", ["con", "emo", "sty"])
def test_encoder_parity_with_the_fp32_oracle(env, which, n_samples):
    """encode(which, oracle fbank, tap_block = l) in fp32x: the residual stream after blocks 0, 5 and 11 within 1e-5 relative L2 of the fp32 oracle's, the
    feature within 1e-5 x max|feature|.  And the switch switches: the bf16 mode of the SAME context is at least 100 x further away (emulation: ~2,000 x)."""
    ao, eng, W = env["ao"], env["eng"], env["W"][which]
    fb = torch.stack([ao.prepare_fbank(x) for x in _waves(n_samples, 2, seed=5)])
    taps = {}
    with torch.no_grad():
        ref = ao.ast_forward(W, fb, True, emulate_bf16=False, taps=taps)
    eng.set_precision("fp32x")
    try:
        assert eng.precision == "fp32x"
        rel = {}
        for l in (0, 5, 11):
            feat, hid = eng.encode(which, fb, tap_block=l)
            r = taps[f"block{l}"]
            rel[l] = float((hid.cpu() - r).norm() / r.norm())
        ferr = float((feat.cpu() - ref).abs().max() / ref.abs().max())
    finally:
        eng.set_precision("bf16")
    feat_b, hid_b = eng.encode(which, fb, tap_block=11)
    rel_b = float((hid_b.cpu() - taps["block11"]).norm() / taps["block11"].norm())
    ferr_b = float((feat_b.cpu() - ref).abs().max() / ref.abs().max())
    print(f"[audio parity] {which} n={n_samples}: fp32x rel-L2 after blocks 0/5/11 {rel[0]:.2e} {rel[5]:.2e} {rel[11]:.2e}, feature {ferr:.2e}; "
          f"bf16 block 11 {rel_b:.2e}, feature {ferr_b:.2e}")
    assert all(v <= 1e-5 for v in rel.values()), rel
    assert ferr <= 1e-5, ferr
    assert rel_b >= 100 * rel[11] and ferr_b >= 100 * ferr, (rel_b, rel[11], ferr_b, ferr)


# ------------------------------------------------------------------------------------------------ (b) switch semantics
def test_switch_semantics(env):
    from amuse_amd import _lib
    from amuse_amd.audio import AudioEngine
    eng = env["eng"]
    w = _waves(48000, 3, seed=9)
    fb = eng.fbank(w)
    # bf16 outputs after an fp32x round trip are bitwise those of a context that never left the mode
    fresh = AudioEngine(env["Wnp"]["con"], env["Wnp"]["emo"], env["Wnp"]["sty"], "cuda:0")
    try:
        assert fresh.precision == "bf16"
        want = [t.clone() for t in fresh.features(w)] + [t.clone() for t in fresh.encode("emo", fb, tap_block=7)]
    finally:
        fresh.close()
    eng.set_precision("fp32x")
    x3 = eng.features(w)
    eng.set_precision("bf16")
    got = list(eng.features(w)) + list(eng.encode("emo", fb, tap_block=7))
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert not any(torch.equal(a, b) for a, b in zip(x3, got[:3]))          # the modes differ
    eng.set_precision("fp32x")
    try:
        # features is encode, encoder by encoder; two calls give the same bits
        for name, t in zip(("con", "emo", "sty"), x3):
            assert torch.equal(eng.encode(name, fb), t), name
        again = eng.features(w)
        assert all(torch.equal(a, b) for a, b in zip(again, x3)) and all(bool(torch.isfinite(t).all()) for t in x3)
        # a clip alone is its row of a 35-clip batch, which crosses the 32-clip chunk (both sides of it)
        w35 = torch.cat([w, _waves(48000, 32, seed=11)])
        b35 = eng.features(w35)
        assert all(torch.equal(a[:3], b) for a, b in zip(b35, x3))
        for k in (1, 31, 32, 34):
            one = eng.features(w35[k:k + 1])
            assert all(torch.equal(a[0], b[k]) for a, b in zip(one, b35)), k
        # bad values are refused and the mode does not change
        for bad in (_lib.PREC_F32, _lib.PREC_F16, -1, 4):
            assert eng.lib.amuse_audio_set_precision(eng.ctx, bad) == -1 and eng.precision == "fp32x"
        with pytest.raises(ValueError):
            eng.set_precision("fp16")
        assert eng.precision == "fp32x" and eng.lib.amuse_audio_precision(eng.ctx) == _lib.PREC_F32X
    finally:
        eng.set_precision("bf16")
    assert eng.precision == "bf16"


# ------------------------------------------------------------------------------------------------ (c) ragged input
def test_ragged_input_equals_call_by_call(env, fp32x):
    from amuse_amd import weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    eng = fp32x
    ragged = [_waves(160000, 1, seed=41), _waves(50000, 2, seed=42), _waves(200000, 1, seed=43), _waves(163840 + 240, 1, seed=44)[0]]
    con, emo, sty = eng.features_ragged(ragged)
    for k, wv in enumerate(ragged):
        c1, e1, s1 = eng.process_single_seq(wv)
        assert torch.equal(c1[0], con[k]) and torch.equal(e1[0], emo[k]) and torch.equal(s1[0], sty[k]), k
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device="cuda:0")
    m.audio_engine = eng
    try:
        many = m.process_seq_list(ragged, framerate=16000)
        assert len(many) == 4
        for k, (c_k, e_k, s_k) in enumerate(many):
            assert c_k.shape == (1, 256) and torch.equal(c_k[0], con[k]) and torch.equal(e_k[0], emo[k]) and torch.equal(s_k[0], sty[k]), k
    finally:
        m.audio_engine = None   # the fixture owns the engine


# ------------------------------------------------------------------------------------------------ (d) from the waveform
def test_every_joint_within_1e_4_from_the_waveform(env):
    """The north star's sentence from the WAVEFORM: GPU fbank + 3 x AST in fp32x, then one diffusion_backward in fp32x (DDIM-50, explicit x_T) on the
    well-conditioned second weight draw, against prepare_fbank -> ast_forward (fp32) -> amuse_oracle.diffusion_backward.  Every joint's L2 < 1e-4, latents
    within 1e-4.  With the audio in bf16 the same call leaves fewer than half of the joints inside the bar (emulation: 0.2 %)."""
    from amuse_amd import scheduler as sch, weights as wts
    from amuse_amd.engine import HipEngine
    from oracle import amuse_oracle as orc
    ao, aeng = env["ao"], env["eng"]
    waves = [_waves(159744, 1, seed=61)[0], _waves(90000, 2, seed=62)[1]]
    with torch.no_grad():
        fb = torch.stack([ao.prepare_fbank(x) for x in waves])
        cond = [ao.ast_forward(env["W"][n], fb, True) for n in ("con", "emo", "sty")]
    wd, wp = wts.make_denoiser_weights(1), wts.make_wellcond_prior_weights(1)
    x_T = torch.randn(2, 128, generator=torch.Generator().manual_seed(77))
    ref = orc.diffusion_backward(orc.to_torch(wd), orc.to_torch(wp), orc.DDIM(), cond[0], cond[1], cond[2], x_T)
    eng = HipEngine(wd, wp, "cuda:0")
    try:
        eng.set_schedule(sch.ddim_table())
        res = {}
        for mode in ("fp32x", "bf16"):
            aeng.set_precision(mode)
            got = aeng.features_ragged(waves)
            cerr = max(float((g.cpu() - c).abs().max() / c.abs().max()) for g, c in zip(got, cond))
            out = eng.diffusion_backward(got[0], got[1], got[2], "fp32x", x_init=x_T)
            lat = float((out["latents"].cpu() - ref["latents"]).abs().max())
            dj = torch.linalg.vector_norm(out["poses"].cpu() - ref["poses"], dim=-1)
            assert dj.shape == (2, 300, 55)
            res[mode] = (cerr, lat, float(dj.max()), float(dj.median()), float((dj < 1e-4).float().mean()))
            print(f"[audio parity] waveform -> pose, audio {mode}: condition max/max {cerr:.2e}, latent {lat:.2e}, pose L2 max {res[mode][2]:.2e} "
                  f"median {res[mode][3]:.2e}, joints within 1e-4: {100 * res[mode][4]:.1f} %")
    finally:
        aeng.set_precision("bf16")
        eng.close()
    assert res["fp32x"][2] < 1e-4 and res["fp32x"][1] < 1e-4, res
    assert res["bf16"][4] < 0.5, res


# ------------------------------------------------------------------------------------------------ (f) host mirror
def test_host_mirror_and_cli(env, tmp_path):
    from conftest import make_reference_tree

    from amuse_amd import main as cli, weights as wts
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    from amuse_amd.npz_writer import pack_feats, smplx_npz_fields
    from amuse_amd.trainer import load_wav
    eng = env["eng"]
    m = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), device="cuda:0")
    m.set_audio_encoders(env["Wnp"]["con"], env["Wnp"]["emo"], env["Wnp"]["sty"], precision="fp32x")
    assert m.audio_engine.precision == "fp32x"
    wave = _waves(160000 + 5000, 1, seed=21)
    got = m.process_single_seq(wave)
    eng.set_precision("fp32x")
    try:
        want = eng.features(wave[0][None])
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        # the CLI: --audio-precision fp32x on the reference-shaped tree of test_cli_infer_and_edit_from_a_reference_tree
        root = make_reference_tree(tmp_path / "amuse", n_infer_wavs=2)
        wx = cli.main(["--fn", "infer_gesture", "--root", str(root), "--random-init", "--audio-precision", "fp32x"])
        px = [np.load(p)["poses"] for p in wx]       # read before the second run: two runs inside one second share the stamped directory and the seeded tags
        wb = cli.main(["--fn", "infer_gesture", "--root", str(root), "--random-init"])
        assert len(wx) == len(wb) == 2
        pb = [np.load(p)["poses"] for p in wb]
        assert all(np.isfinite(p).all() and p.shape == (300, 55, 3) for p in px)
        assert not any(np.array_equal(a, b) for a, b in zip(px, pb))
        # ... and they are the engine-level result: this engine's fp32x embeddings of the same WAVs through the same sampler (clips 0, 1 of seed 2024)
        wavs = sorted((root / "viz_dump/test/speech").glob("*.wav"))
        loaded = [load_wav(p) for p in wavs]
        con, emo, sty = eng.features_ragged([a - a.mean() for a in loaded])                  # (the trainer removes the mean, trainer.py:519-521)
        _, ldm_cfg = cli.load_config(root, "infer_gesture", None)
        m2 = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), ldm_cfg, "cuda:0", seed=2024)
        m2.precision = "fp32x"
        m2.set_sampler("ddim", None)
        out = m2.diffusion_backward(2, con, emo, sty, clip_index0=0)
        # what the trainer writes of a clip: poses ++ trans packed into (300, 168), then the NPZ writer's fields (it freezes the lower body to frame 0)
        feats = pack_feats(out["poses"], out["trans"]).cpu().numpy()
        for k in range(2):
            assert np.array_equal(smplx_npz_fields(feats[k])["poses"], px[k]), k
    finally:
        eng.set_precision("bf16")
        m.audio_engine.close()
