"""GPU tests at the shapes of BASELINE.json's configs that the per-kernel parity tests do not reach:

  config 2  - one clip, 1000-step DDPM, bf16: the 8-wave kernel's OWN trajectory is checked state by state
              (teacher-forced eps_hat against the bf16-emulating oracle; the in-loop update against the scheduler
              restatement applied to that eps_hat)
  config 5  - edit_gesture emotion_control: 16 waveforms -> audio front-end -> 8 x 8 content / emotion swaps = 64 jobs
              as ONE diffusion_backward launch (scripts/trainer.py:839-901, infer_ldm.py:387-410)
  bf16 mode - the throughput mode is gated against the fp32 parity mode at <= 2 x the measured drift
              (profiles/r01_bf16_vs_fp32_drift.json), so a regression of the bf16 kernels fails a test
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _err(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max())


@pytest.fixture(scope="module")
def env():
    from amuse_amd import weights as wts
    from amuse_amd.engine import HipEngine
    from oracle import amuse_oracle as orc
    wd, wp = wts.make_denoiser_weights(0), wts.make_prior_weights(0)
    eng = HipEngine(wd, wp, "cuda:0")
    yield {"eng": eng, "wd": wd, "wp": wp, "Wd": orc.to_torch(wd), "Wp": orc.to_torch(wp), "orc": orc}
    eng.close()


def test_config2_bf16_single_clip_ddpm1000_own_trajectory(env):
    """BASELINE config 2 through k_sample8 (B = 1, T = 1000, bf16): every 100th state of the kernel's own trajectory."""
    from amuse_amd import scheduler as sch
    orc, eng, Wd = env["orc"], env["eng"], env["Wd"]
    gen = torch.Generator().manual_seed(2024)
    c, e, s, x = (torch.randn(1, n, generator=gen) for n in (256, 256, 256, 128))
    nz = torch.randn(1000, 1, 128, generator=gen)
    tab = sch.ddpm_table()
    eng.set_schedule(tab)
    lat, traj = eng.sample(c, e, s, "bf16", x_init=x, step_noise=nz, return_traj=True)
    traj = traj.cpu()
    assert torch.equal(lat.cpu(), traj[-1]) and bool(torch.isfinite(traj).all())
    osched = orc.DDPM()
    worst_eps, worst_upd = 0.0, 0.0
    for i in range(0, 1000, 100):
        xi = x if i == 0 else traj[i - 1]
        t = int(tab.timesteps[i])
        eps = eng.denoise_step(xi, t, c, e, s, "bf16").cpu()            # teacher-forced on the kernel's own state
        ref = orc.denoiser_forward(Wd, xi, t, c, e, s, emulate_bf16=True)
        worst_eps = max(worst_eps, _err(eps, ref))
        # the step the loop took from this state == scheduler restatement applied to the teacher-forced eps_hat
        nxt = osched.step(eps, t, xi, nz[i])
        scale = max(1.0, float(nxt.abs().max()))
        worst_upd = max(worst_upd, _err(traj[i], nxt) / scale)
    assert worst_eps < 5e-2, worst_eps      # whole-network bf16 tolerance (|eps_hat| ~ 3); measured 1-2e-2
    assert worst_upd < 2e-5, worst_upd      # the in-loop eps_hat IS the teacher-forced one; update in fp32
    # and the same job through the one-call entry point is deterministic
    a = eng.diffusion_backward(c, e, s, "bf16", seed=2024)
    b = eng.diffusion_backward(c, e, s, "bf16", seed=2024)
    assert torch.equal(a["poses"], b["poses"]) and bool(torch.isfinite(a["poses"]).all())


def test_bf16_mode_gated_against_fp32_mode(env):
    """Same inputs + noise through both modes, 64 clips (tests/tools/gpu_drift.py is the measuring twin).  Bounds are
    <= 2 x the measured values: DDIM-50 latents rms 0.039 / max 0.23 on rms 0.53; DDPM-1000 latents rms 0.17 on rms 32,
    pose geodesic median 0.39 deg / p99 3.6 deg."""
    from amuse_amd import scheduler as sch
    orc, eng = env["orc"], env["eng"]
    g = torch.Generator().manual_seed(2024)
    B = 64
    c, e, s, x = (torch.randn(B, n, generator=g) for n in (256, 256, 256, 128))
    def geodesic_deg(lat_ref, lat_bf16):
        pa = eng.vae_decode(lat_ref, None, "fp32")["poses"].cpu()
        pb = eng.vae_decode(lat_bf16, None, "bf16")["poses"].cpu()
        Ra, Rb = orc.axis_angle_to_matrix(pa.double()), orc.axis_angle_to_matrix(pb.double())
        return torch.acos(((Ra.transpose(-1, -2) @ Rb).diagonal(dim1=-2, dim2=-1).sum(-1) - 1).div(2).clamp(-1, 1)) * 180 / np.pi

    eng.set_schedule(sch.ddim_table())
    a = eng.sample(c, e, s, "fp32", x_init=x).cpu()
    b = eng.sample(c, e, s, "bf16", x_init=x).cpu()
    assert float((a - b).pow(2).mean().sqrt()) < 0.08 and float((a - b).abs().max()) < 0.46
    # the fast parity mode sits with the fp32 mode, not with bf16: same 64 clips, DDIM-50 latents
    ax = eng.sample(c, e, s, "fp32x", x_init=x).cpu()
    assert float((a - ax).abs().max()) < 1e-3, float((a - ax).abs().max())
    # DDIM-50 is the sampler the reference ships (infer_ldm.py:116-125): its bf16 POSES are gated too - latents of rms 0.53
    # (no ancestral noise to wash the rounding out) put the decoder's 6D outputs near ill-conditioned Gram-Schmidt pivots, so
    # the same latent drift costs more degrees than under DDPM-1000: measured median 3.6 deg, p99 30.6 deg; bound <= 2 x
    ang = geodesic_deg(a, b)
    assert float(ang.median()) < 7.2, float(ang.median())
    assert float(ang.flatten().kthvalue(int(ang.numel() * 0.99)).values) < 61.0
    tab = sch.ddpm_table()
    eng.set_schedule(tab)
    nz = torch.randn(tab.n_steps, B, 128, generator=g)
    a = eng.sample(c, e, s, "fp32", x_init=x, step_noise=nz).cpu()
    b = eng.sample(c, e, s, "bf16", x_init=x, step_noise=nz).cpu()
    assert float((a - b).pow(2).mean().sqrt()) < 0.35
    ang = geodesic_deg(a, b)
    assert float(ang.median()) < 1.0, float(ang.median())
    assert float(ang.flatten().kthvalue(int(ang.numel() * 0.99)).values) < 8.0


def test_config5_edit_gesture_emotion_control_batch64(env):
    """16 waveforms -> amuse_audio_features -> 8 x 8 emotion swap -> ONE B = 64 diffusion_backward through the product's
    edit driver (amuse_amd/trainer.py emotion_control_jobs + run_jobs); DDIM-50 fp32 latents against the oracle for 8 of
    the 64 jobs; bf16 DDPM-1000 finite and deterministic."""
    from amuse_amd import audio_weights as aw
    from amuse_amd.infer_ldm import PretrainedLPDM_v1
    from amuse_amd.trainer import emotion_control_jobs, run_jobs
    orc, Wd = env["orc"], env["Wd"]
    m = PretrainedLPDM_v1.from_state_dicts(env["wd"], env["wp"], device="cuda:0", seed=2024)
    m.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS))
    m.emotion_control = True
    gen = torch.Generator().manual_seed(0)
    takes = [f"0_{k}_{k}" for k in (9, 65, 73, 81, 87, 95, 103, 111)]       # one take per emotion (ldm_evals.py:79-87)
    waves = 0.1 * torch.randn(16, 160000, generator=gen)
    con, emo, sty = m.audio_engine.features(waves)                          # 16 clips through fbank + 3 x AST
    assert bool(torch.isfinite(con).all() and torch.isfinite(emo).all() and torch.isfinite(sty).all())
    # the dataset dict process_loader receives (infer_ldm.py:387-410), latents precomputed: content / style of
    # waveform k, emotion of waveform 8 + k
    data = {"emotion_control_info": "[scott]_all", "emotion_control": {"scott": {
        tk: {"ld_z": torch.zeros(1, 128), "ld_z_con": con[k:k + 1], "ld_z_emo": emo[8 + k:9 + k], "ld_z_sty": sty[k:k + 1],
             "ld_attr": ("scott", "male", "native", "x", "30"), "ld_wav": np.zeros(10000, np.float32),
             "ld_motion": None} for k, tk in enumerate(takes)}}}
    loaded = m.process_loader(data)
    jobs = emotion_control_jobs(loaded["emotion_control"])
    assert len(jobs) == 64 and sum(j["bsz"] for j in jobs) == 64             # 8 original emotions x 8 swapped (trainer.py:919)
    m.precision, c0 = "fp32", m._clip_counter
    m.set_sampler("ddim")
    res = run_jobs(m, jobs, return_latents=True)
    assert len(res) == 64 and res[0]["feats"].shape == (1, 300, 168)
    lat = torch.cat([r["latents"] for r in res]).cpu()
    x0 = m.engine.counter_normal(m.seed, c0, 64, 0, 0).cpu()
    for j in range(0, 64, 9):                                                # jobs 0, 9, ..., 63: 8 distinct (take, emotion) pairs
        job = jobs[j]
        ref = orc.sample_latents(Wd, orc.DDIM(), job["z_con"].cpu(), job["z_emo"].cpu(), job["z_sty"].cpu(), x0[j:j + 1])
        assert _err(lat[j:j + 1], ref) < 1e-4, j
    # the same 64 jobs in the fast parity mode (fp32x): same clip indices, same bar against the oracle, and the SMPL-X
    # features of the whole task within the fp32 run's conversion noise
    m.precision, m._clip_counter = "fp32x", c0
    resx = run_jobs(m, jobs, return_latents=True)
    latx = torch.cat([r["latents"] for r in resx]).cpu()
    for j in range(0, 64, 9):
        job = jobs[j]
        ref = orc.sample_latents(Wd, orc.DDIM(), job["z_con"].cpu(), job["z_emo"].cpu(), job["z_sty"].cpu(), x0[j:j + 1])
        assert _err(latx[j:j + 1], ref) < 1e-4, j
    assert _err(latx, lat) < 1e-4
    m.precision = "fp32"
    # swapping changes the motion; the un-swapped job keeps the take's own emotion
    assert jobs[0]["z_emo_key"] == "ld_z_emo" and torch.equal(jobs[0]["z_emo"], emo[8:9])
    assert not torch.equal(res[0]["feats"], res[1]["feats"])
    # throughput mode at this shape: DDPM-1000 bf16
    m.precision = "bf16"
    m.set_sampler("ddpm")
    m._clip_counter = 1000
    a = run_jobs(m, jobs)
    m._clip_counter = 1000
    b = run_jobs(m, jobs)
    fa, fb = torch.cat([r["feats"] for r in a]), torch.cat([r["feats"] for r in b])
    assert fa.shape == (64, 300, 168) and bool(torch.isfinite(fa).all()) and torch.equal(fa, fb)
    m.audio_engine.close()


_SHARD_WORKER = r'''
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from amuse_amd import weights as wts, scheduler as sch
from amuse_amd.engine import HipEngine
from amuse_amd.shard import sample_sharded
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)     # one GPU on the test box: both ranks share cuda:0
eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0), "cuda:0")
eng.set_schedule(sch.ddpm_table(40))
g = torch.Generator().manual_seed(3)
B = 300                                                            # three clips per tile at the job level
con, emo, sty = (torch.randn(B, 256, generator=g) for _ in range(3))
def sample_fn(bsz, c, e, s, clip_index0=0):
    o = eng.diffusion_backward(c, e, s, "bf16", seed=11, clip_index0=clip_index0)
    return {"latents": o["latents"], "poses": o["poses"][:, :2]}
full = sample_sharded(sample_fn, con, emo, sty, rank, world, gather=True, set_clips_per_group=eng.set_clips_per_group,
                      set_decode_path=eng.set_decode_path)
if rank == 0:
    single = sample_sharded(sample_fn, con, emo, sty, 0, 1, set_clips_per_group=eng.set_clips_per_group,
                            set_decode_path=eng.set_decode_path)
    assert full["latents"].shape == (B, 128)
    assert torch.equal(full["latents"], single["latents"].cpu()) and torch.equal(full["poses"], single["poses"].cpu())
    # the job-level tiling did not leak into the context: an unrelated small call is back on the per-launch rule
    a = eng.sample(con[:5], emo[:5], sty[:5], "bf16", seed=11)
    eng.set_clips_per_group(1)
    assert torch.equal(a, eng.sample(con[:5], emo[:5], sty[:5], "bf16", seed=11))
    print("SHARD_GPU_OK")
dist.barrier()
dist.destroy_process_group()
'''


def test_two_process_sharded_job_through_the_hip_engine(tmp_path):
    """The N > 1 path bench.py --gpus N runs (one process per rank, HipEngine per rank, amuse_amd/shard.py), as two
    processes on this box's one GPU with gloo for the gather: bitwise the single-process job."""
    import os, subprocess, sys
    from conftest import REPO
    script = tmp_path / "worker.py"
    script.write_text(_SHARD_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641")
    procs = [subprocess.Popen([sys.executable, str(script), str(REPO)], env=dict(env, RANK=str(r), WORLD_SIZE="2"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "SHARD_GPU_OK" in outs[0]


def test_bench_line_with_two_ranks_sharing_the_gpu():
    """`python bench.py --gpus 2` as typed (the parent starts its own ranks, amuse_amd/launch.py), with AMUSE_BENCH_SHARE_GPU=1 so that
    both ranks run on this box's one GPU (gloo for the two scalar reductions): the N > 1 logic of bench.py end to end - `value` =
    BASELINE config 3's job (--clips IN TOTAL, sharded over the ranks: "scaling": "strong"), the weak-scaling companion, clip ranges,
    one JSON line from rank 0.  (Timings of ranks that share a GPU mean nothing and are not looked at.)"""
    import json, os, subprocess, sys
    from conftest import REPO
    env = dict(os.environ, AMUSE_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--T", "20", "--clips", "64",
                        "--full", "--no-extras"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_seen"] == 2 and d["scaling"] == "strong"
    assert d["config"]["clips_total"] == 64 and d["config"]["clips_rank0"] == 32       # config.clips_total == --clips at every N
    assert d["config"]["clip_range_per_rank"] == [[0, 32], [32, 64]]
    assert abs(d["value"] - 64 * 300 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    w = d["weak_scaling"]
    assert w["clips_total"] == 128 and w["clips_per_gpu"] == 64 and w["clip_range_per_rank"] == [[0, 64], [64, 128]] and w["frames_per_s"] > 0
    assert d["roofline"]["frac"] > 0 and d["roofline"]["kernel_ms"] > 0 and d["roofline"]["bound"] == "chain+l2_stream"


def test_bench_edit_batch_with_two_ranks_sharing_the_gpu():
    """BASELINE config 5's shape through `bench.py --gpus 2` (AMUSE_BENCH_SHARE_GPU=1: both ranks on this box's GPU, gloo for the exchange): each rank embeds 8 of
    the 16 WAVs, the embeddings are all-gathered, each rank samples 32 of the 64 jobs."""
    import json, os, subprocess, sys
    from conftest import REPO
    env = dict(os.environ, AMUSE_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--T", "20", "--clips", "64",
                        "--no-extras", "--edit-batch"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    eb = d["edit_batch"]
    assert "error" not in eb, eb
    assert eb["n_gpus"] == 2 and eb["wavs_per_rank"] == [[0, 8], [8, 16]] and eb["jobs_per_rank"] == [[0, 32], [32, 64]]
    assert eb["frames_per_s"] > 0 and "all_gather" in eb["exchange"]


def test_rccl_world_of_one_all_reduces_the_flat_gradient():
    """init_process_group("nccl") (= RCCL on ROCm) at world size 1 on the GPU and an all-reduce of the 6,835,661-element flat fp32
    gradient train_gesture exchanges (amuse_amd/train_gesture.py) - the collective library is loaded and run by something in this
    tree even on a one-GPU box.  Own process: a process group cannot be re-initialised inside the test session."""
    import os, subprocess, sys
    from conftest import REPO
    code = (
        "import os, torch, torch.distributed as dist\n"
        "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29655', RANK='0', WORLD_SIZE='1')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', device_id=torch.device('cuda', 0))\n"
        "g = torch.arange(6835661, device='cuda', dtype=torch.float32) * 1e-6\n"
        "ref = g.clone()\n"
        "dist.barrier(); dist.all_reduce(g, op=dist.ReduceOp.SUM); torch.cuda.synchronize()\n"
        "assert torch.equal(g, ref), 'world of one: SUM must be the identity'\n"
        "t = torch.tensor([1.5], device='cuda', dtype=torch.float64); dist.all_reduce(t, op=dist.ReduceOp.MAX)\n"
        "assert float(t.item()) == 1.5\n"
        "print('RCCL_OK', dist.get_backend(), torch.cuda.nccl.version())\n"
        "dist.destroy_process_group()\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True,
                       timeout=600, cwd=str(REPO))
    assert r.returncode == 0 and "RCCL_OK nccl" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_entry_points_are_stream_capturable():
    """A caller may capture the library's calls into a HIP graph (no allocation, host synchronisation or default-stream work once a context is warm; the audio
    front-end's three-stream fork / join is event-ordered): capture diffusion_backward and amuse_audio_features, replay, compare bitwise with the eager call.
    (Measured gain of replaying: 0-4 %, profiles/r05_graph_capture_probe.txt - the launch sequences are device-bound; the point here is that capture WORKS.)"""
    from amuse_amd import audio_weights as aw, scheduler as sch, weights as wts
    from amuse_amd.audio import AudioEngine
    from amuse_amd.engine import HipEngine
    eng = HipEngine(wts.make_denoiser_weights(0), wts.make_prior_weights(0))
    eng.set_schedule(sch.ddim_table())
    aeng = AudioEngine(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS), device="cuda:0")
    g = torch.Generator().manual_seed(0)
    c, e, s_ = (torch.randn(2, 256, generator=g).cuda() for _ in range(3))
    w = (0.1 * torch.randn(1, 160000, generator=g)).cuda()
    for fn, key in ((lambda: eng.diffusion_backward(c, e, s_, "fp32x", seed=5), "poses"), (lambda: {"f": torch.cat(aeng.features(w))}, "f")):
        ref = fn()[key].clone()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            fn()
        torch.cuda.current_stream().wait_stream(st)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            out = fn()
        out[key].zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[key], ref)
    aeng.close()
    eng.close()
