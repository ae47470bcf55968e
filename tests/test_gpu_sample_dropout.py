"""GPU: train-mode sampling (amuse_set_sample_dropout) - the Denoiser's encoder dropouts live inside the persistent sampler kernels.

The mask contract of include/amuse_hip.h is restated here on its own: element e of dropout site s of encoder layer l uses draw e % 4 of
Philox4x32-10(key = seed, counter = (clip, step, ((4 l + s) << 16) | e / 4, 2 + epoch)), keep <=> draw >> 8 >= p 2^24, kept values times 1 / (1 - p).
Sites: 0 = softmax probabilities (e = (h S + q) S + k), 1 = dropout1 (e = tok 128 + f), 2 = the FFN's inner dropout (e = tok 512 + f),
3 = dropout2 (e = tok 128 + f).  The restatement below applies those masks to the encoder-block arithmetic of the oracle."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 0.1
SEED = 0x1234_5678_9ABC_DEF0


def _weights():
    from amuse_amd import weights as wts
    from oracle import amuse_oracle as orc
    wd, wp = wts.make_denoiser_weights(0), wts.make_prior_weights(0)
    return wd, wp, orc.to_torch(wd)


def _engine(wd, wp, table=None):
    from amuse_amd import scheduler as sch
    from amuse_amd.engine import HipEngine
    eng = HipEngine(wd, wp, "cuda:0")
    eng.set_schedule(table or sch.ddim_table())
    return eng


def _inputs(B, ncond, seed=5):
    g = torch.Generator().manual_seed(seed)
    con, emo, sty, x = (torch.randn(B, n, generator=g) for n in (256, 256, 256, 128))
    return con, (emo if ncond >= 2 else None), (sty if ncond >= 3 else None), x


def _epoch_set(eng, k):
    from amuse_amd import _lib
    _lib.check(eng.lib.amuse_train_epoch_set(int(k), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _thr_scale(p):
    p32 = np.float32(p)
    return int(p32 * np.float32(16777216.0)), float(np.float32(1.0) / (np.float32(1.0) - p32))


def _site_masks(seed, clips, step, epoch, S, p):
    """{(l, s): bool keep array}: s 0 -> (B, 4, S, S), s 1 / 3 -> (B, S, 128), s 2 -> (B, S, 512)."""
    from oracle import amuse_oracle as orc
    thr, _ = _thr_scale(p)
    clips = np.asarray(clips, dtype=np.uint64)
    sizes = {0: 4 * S * S, 1: S * 128, 2: S * 512, 3: S * 128}
    out = {}
    for l in range(9):
        for s, n in sizes.items():
            e = np.arange(n, dtype=np.uint64)
            ctr = np.zeros((len(clips), n, 4), dtype=np.uint64)
            ctr[..., 0] = clips[:, None]
            ctr[..., 1] = np.uint64(step)
            ctr[..., 2] = (np.uint64((4 * l + s) << 16) | (e // np.uint64(4)))[None]
            ctr[..., 3] = np.uint64(2 + epoch)
            # (each group of 4 draws is computed 4 times here: simple beats fast in a restatement)
            r = orc.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
            draw = np.take_along_axis(r, (e % np.uint64(4)).astype(np.int64)[None, :, None].repeat(len(clips), 0), axis=-1)[..., 0]
            keep = (draw >> np.uint64(8)) >= np.uint64(thr)
            shape = {0: (len(clips), 4, S, S), 1: (len(clips), S, 128), 2: (len(clips), S, 512), 3: (len(clips), S, 128)}[s]
            out[(l, s)] = torch.from_numpy(keep.reshape(shape))
    return out


def _drop(x, keep, scale):
    return torch.where(keep, x * scale, torch.zeros_like(x))


def _enc_block(ops, x, W, p, masks, l, scale):
    """oracle enc_block (TransformerEncoderLayer.forward_post) with the four dropout sites."""
    from oracle import amuse_oracle as orc
    B, S, D = x.shape
    pa = p + ".self_attn"
    qkv = ops.lin(x, W[pa + ".in_proj_weight"], W[pa + ".in_proj_bias"])
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    q = q * math.sqrt(1.0 / 32)
    sh = lambda t: t.reshape(B, S, 4, 32).permute(0, 2, 1, 3)
    q, k, v = sh(q), sh(k), sh(v)
    att = torch.softmax(ops.mm(q, k.transpose(-1, -2)), dim=-1)
    if masks is not None:
        att = _drop(att, masks[(l, 0)], scale)
    o = ops.mm(att, v).permute(0, 2, 1, 3).reshape(B, S, D)
    y = ops.lin(o, W[pa + ".out_proj.weight"], W[pa + ".out_proj.bias"])
    if masks is not None:
        y = _drop(y, masks[(l, 1)], scale)
    x = orc.layer_norm(x + y, W[p + ".norm1.weight"], W[p + ".norm1.bias"])
    h = ops.act(ops.lin(x, W[p + ".linear1.weight"], W[p + ".linear1.bias"]))
    if masks is not None:
        h = _drop(h, masks[(l, 2)], scale)
    y = ops.lin(h, W[p + ".linear2.weight"], W[p + ".linear2.bias"])
    if masks is not None:
        y = _drop(y, masks[(l, 3)], scale)
    return orc.layer_norm(x + y, W[p + ".norm2.weight"], W[p + ".norm2.bias"])


def _forward(W, x, t, con, emo, sty, masks, p=P, taps=None, emulate=None):
    """Denoiser.forward with the masks (None = eval); emulate = None | "bf16" | "fp16" (the oracle's 16-bit models)."""
    from oracle import amuse_oracle as orc
    ops = orc.Ops(emulate is not None, poly_gelu=emulate is not None, fp16=emulate == "fp16")
    _, scale = _thr_scale(p)
    xs = orc.denoiser_tokens(W, x, t, con, emo, sty)
    if taps is not None:
        taps.append(xs)
    layer = iter(range(9))
    block = lambda h, name: _enc_block(ops, h, W, name, masks, next(layer), scale)
    names = [f"encoder.input_blocks.{i}" for i in range(4)] + ["encoder.middle_block"] + [f"encoder.output_blocks.{i}" for i in range(4)]
    xs_skip = []
    for i in range(4):
        x_ = block(xs if i == 0 else x_, names[i])
        xs_skip.append(x_)
        if taps is not None:
            taps.append(x_)
    x_ = block(x_, names[4])
    if taps is not None:
        taps.append(x_)
    for i in range(4):
        x_ = ops.lin(torch.cat([x_, xs_skip.pop()], dim=-1), W[f"encoder.linear_blocks.{i}.weight"], W[f"encoder.linear_blocks.{i}.bias"])
        x_ = block(x_, names[5 + i])
        if taps is not None:
            taps.append(x_)
    out = orc.layer_norm(x_, W["encoder.norm.weight"], W["encoder.norm.bias"])
    if taps is not None:
        taps.append(out)
    return out[:, 0]


def _S(emo, sty):
    return 3 + (emo is not None) + (sty is not None)


# ---- 1. eval unchanged ---------------------------------------------------------------------------------------------------------------
def test_p0_is_bitwise_the_eval_kernel():
    wd, wp, _ = _weights()
    con, emo, sty, x = _inputs(40, 3)
    fresh, eng = _engine(wd, wp), _engine(wd, wp)
    for prec in ("fp32", "bf16"):
        ref = fresh.sample(con, emo, sty, prec, seed=3)
        eng.set_sample_dropout(0.0, SEED)
        assert torch.equal(eng.sample(con, emo, sty, prec, seed=3), ref), prec
        eng.set_sample_dropout(P, SEED)
        assert not torch.equal(eng.sample(con, emo, sty, prec, seed=3), ref), prec
        eng.set_sample_dropout(0.0, SEED)
        assert torch.equal(eng.sample(con, emo, sty, prec, seed=3), ref), prec
    fresh.close(), eng.close()


# ---- 2. exact masks, one step (fp32) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncond", [3, 2, 1])
def test_one_step_matches_the_restated_masks(ncond):
    from oracle import amuse_oracle as orc
    wd, wp, W = _weights()
    con, emo, sty, x = _inputs(7, ncond)
    S, t = _S(emo, sty), 501
    # the restatement's non-mask arithmetic is the oracle's
    assert float((_forward(W, x, t, con, emo, sty, None) - orc.denoiser_forward(W, x, t, con, emo, sty)).abs().max()) < 1e-6
    eng = _engine(wd, wp)
    _epoch_set(eng, 0)
    eng.set_sample_dropout(P, SEED)
    eps, tap = eng.denoise_step(x, t, con, emo, sty, "fp32", taps=True)
    taps = []
    ref = _forward(W, x, t, con, emo, sty, _site_masks(SEED, np.arange(7), 0, 0, S, P), taps=taps)
    tp = tap.cpu()
    for k in range(11):
        assert float((tp[k, :S] - taps[k][0]).abs().max()) < 1e-5, k
    assert float((eps.cpu() - ref).abs().max()) < 1e-5
    assert float((eps.cpu() - orc.denoiser_forward(W, x, t, con, emo, sty)).abs().max()) > 1e-2   # (the masks matter)
    eng.close()


# ---- 3. exact masks, whole DDIM-50 loop (fp32) ---------------------------------------------------------------------------------------
def test_ddim50_trajectory_matches_the_restated_loop():
    from oracle import amuse_oracle as orc
    wd, wp, W = _weights()
    con, emo, sty, x = _inputs(3, 3, seed=9)
    eng = _engine(wd, wp)
    _epoch_set(eng, 0)
    eng.set_sample_dropout(P, SEED)
    c0 = 11
    _, traj = eng.sample(con, emo, sty, "fp32", clip_index0=c0, x_init=x, return_traj=True)
    traj = traj.cpu()
    sched = orc.DDIM()
    xr = x * sched.init_noise_sigma
    worst = 0.0
    for i, t in enumerate(sched.timesteps):
        eps = _forward(W, xr, int(t), con, emo, sty, _site_masks(SEED, c0 + np.arange(3), i, 0, 5, P))
        xr = sched.step(eps, int(t), xr, None)
        worst = max(worst, float((traj[i] - xr).abs().max()))
    assert worst < 3e-5, worst
    eng.close()


# ---- 4. bf16 / fp16 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_step_follows_its_own_masks(prec):
    wd, wp, W = _weights()
    B = 24
    con, emo, sty, x = _inputs(B, 3, seed=13)
    eng = _engine(wd, wp)
    _epoch_set(eng, 0)
    eng.set_sample_dropout(P, SEED)
    eps = eng.denoise_step(x, 261, con, emo, sty, prec).cpu()
    right = _forward(W, x, 261, con, emo, sty, _site_masks(SEED, np.arange(B), 0, 0, 5, P), emulate=prec)
    wrong = _forward(W, x, 261, con, emo, sty, _site_masks(SEED, np.arange(B) + 1, 0, 0, 5, P), emulate=prec)
    e_right, e_wrong = float((eps - right).abs().max()), float((eps - wrong).abs().max())
    assert e_right < 8e-2, e_right
    assert e_right <= 0.25 * e_wrong, (e_right, e_wrong)
    eng.close()


# ---- 5. keying -------------------------------------------------------------------------------------------------------------------------
def test_masks_are_keyed_by_seed_clip_and_epoch():
    wd, wp, _ = _weights()
    B = 12
    con, emo, sty, x = _inputs(B, 3, seed=17)
    eng = _engine(wd, wp)
    run = lambda c0=0, prec="fp32": eng.sample(con, emo, sty, prec, clip_index0=c0, x_init=x)
    _epoch_set(eng, 0)
    eng.set_sample_dropout(P, SEED)
    a = run()
    assert torch.equal(run(), a)
    eng.set_sample_dropout(P, SEED + 1)
    assert not torch.equal(run(), a)
    eng.set_sample_dropout(P, SEED)
    assert not torch.equal(run(c0=5), a)
    _epoch_set(eng, 3)
    assert not torch.equal(run(), a)
    _epoch_set(eng, 0)
    assert torch.equal(run(), a)
    # per-clip results do not depend on how the clips are split into calls or tiles (up to the rounding of the attention sums)
    lo = eng.sample(con[:5], emo[:5], sty[:5], "fp32", clip_index0=0, x_init=x[:5])
    hi = eng.sample(con[5:], emo[5:], sty[5:], "fp32", clip_index0=5, x_init=x[5:])
    assert float((torch.cat([lo, hi]) - a).abs().max()) < 1e-4
    eng.set_clips_per_group(1)
    assert float((run() - a).abs().max()) < 1e-4
    eng.set_clips_per_group(0)
    eng.close()


# ---- 6. graph replay -------------------------------------------------------------------------------------------------------------------
def test_graph_replays_draw_fresh_masks_through_the_epoch():
    from amuse_amd import _lib
    wd, wp, _ = _weights()
    B = 32
    con, emo, sty, x = (t.cuda() for t in _inputs(B, 3, seed=19))
    eng = _engine(wd, wp)
    eng.set_sample_dropout(P, SEED)
    _epoch_set(eng, 0)
    eng.sample(con, emo, sty, "bf16", x_init=x)         # eager first: workspaces and the epoch word exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.sample(con, emo, sty, "bf16", x_init=x)
        _lib.check(eng.lib.amuse_train_epoch_advance(1, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    _epoch_set(eng, 0)
    replays = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    assert not torch.equal(replays[0], replays[1]) and not torch.equal(replays[1], replays[2])
    for k in range(3):
        _epoch_set(eng, k)
        assert torch.equal(eng.sample(con, emo, sty, "bf16", x_init=x), replays[k]), k
    _epoch_set(eng, 0)
    del g
    eng.close()


# ---- 7. rejects ------------------------------------------------------------------------------------------------------------------------
def test_contexts_without_a_dropout_kernel_refuse():
    from amuse_amd import _lib
    from amuse_amd import scheduler as sch
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    wd, wp, _ = _weights()
    con, emo, sty, x = _inputs(4, 3)
    eng = _engine(wd, wp)
    eng.set_sample_dropout(P, SEED)
    lat = torch.full((4, 128), 7.0, device="cuda:0")
    xd, cd, ed, sd = x.cuda(), con.cuda(), emo.cuda(), sty.cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.amuse_sample(eng.ctx, p(cd), p(ed), p(sd), 4, 2, 0, 0, p(xd), None, p(lat), None, eng._stream())
    torch.cuda.synchronize()
    assert rc == -4 and bool((lat == 7.0).all())                  # AMUSE_ESTATE, nothing written
    with pytest.raises(_lib.AmuseHipError):
        eng.denoise_step(x, 500, con, emo, sty, "fp32x")
    eng.close()
    for arch, pose in (("trans_dec", False), ("trans_enc", True)):
        ev = HipEngine(wts.make_denoiser_weights(0, arch, pose), None if pose else wts.make_prior_weights(0), "cuda:0", arch=arch, diffusion_only=pose)
        ev.set_schedule(sch.ddim_table())
        ss = ev.state_shape
        ev.set_sample_dropout(P, SEED)
        out = torch.full((4, *ss), 7.0, device="cuda:0")
        xv = torch.randn(4, *ss, device="cuda:0")
        rc = ev.lib.amuse_sample(ev.ctx, p(cd), p(ed), p(sd), 4, 0, 0, 0, p(xv), None, p(out), None, ev._stream())
        eps = torch.full((4, *ss), 7.0, device="cuda:0")
        rc2 = ev.lib.amuse_denoise_step(ev.ctx, p(xv), 500, p(cd), p(ed), p(sd), 4, 0, p(eps), None, ev._stream())
        torch.cuda.synchronize()
        assert rc == -4 and rc2 == -4 and bool((out == 7.0).all()) and bool((eps == 7.0).all()), arch
        ev.close()


# ---- 8. the trainer --------------------------------------------------------------------------------------------------------------------
def test_trainer_with_the_train_mode_hip_sampler():
    from amuse_amd.train_gesture import HipInnerSampler, build_trainer, synthetic_batch
    torch.manual_seed(0)
    tr = build_trainer("cuda:0", inner="train-hip")
    s = tr.inner_sampler
    assert isinstance(s, HipInnerSampler) and s.dropout == pytest.approx(0.1) and not getattr(s, "serial", False) and s.mode == "train-hip"
    batch = synthetic_batch(32, 3, "cuda:0")
    for _ in range(3):
        loss = float(tr.train_step(batch))
        ld = {k: float(v) for k, v in tr.lpdm_losses.compute().items()}
        assert np.isfinite(loss) and np.isfinite(ld["gen_feature"]) and ld["gen_feature"] > 0
    # eager calls draw fresh masks through the clip counter: the same conditions, two different samples
    c, e, st = batch["ld_audio_con"], batch["ld_audio_emo"], batch["ld_audio_sty"]
    with torch.no_grad():
        assert not torch.equal(s.sample_latents(c, e, st, 32), s.sample_latents(c, e, st, 32))
    # capturable: the sampler is not serial; replays see the epoch word advance
    seen = []
    dec = s.decode
    s.decode = lambda lat: (seen.append(lat), dec(lat))[1]
    assert tr.enable_graph(batch)
    s.decode = dec
    assert len(seen) == 1
    outs = []
    for _ in range(2):
        assert np.isfinite(float(tr.train_step(batch)))
        torch.cuda.synchronize()
        outs.append(seen[0].clone())
    assert not torch.equal(outs[0], outs[1])
