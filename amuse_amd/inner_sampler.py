"""The no-gradient half of a train_gesture iteration: ldm.diffusion_backward (DDIM-50, ldm.py:117-153) + prior.decode of its result on the trainer's CURRENT
weights, in the four modes of `--inner-sampler` / AMUSE_TRAIN_INNER.  MODES is their one description - how each is built, whether it needs a GPU, and the sentence
the argparse help, build_trainer's errors, the start-up print and the bench line's config.inner_sampler all quote; InnerSampler is what GestureTrainer asks of one."""
from __future__ import annotations

import time
from typing import Dict, NamedTuple, Optional

import torch
import torch.nn as nn

from . import scheduler as sch
from .nn_modules import numpy_state

SEQ_LEN = 300


class InnerSampler:
    """(con, emo, sty, bsz) -> noise2feats (B, 300, 333).  The class attributes are what GestureTrainer reads; a sampler overrides those it changes."""
    mode = ""                               # its key in MODES
    serial = False                          # runs on the trainer's own modules: on the trainer's stream, and not capturable in a HIP graph
    decode_on_trainer_stream = False        # sample_latents() on the side stream, decode() on the trainer's stream after the join
    graph_safe = False                      # set by the capture of the step: initial latents from torch's generator instead of the host-side clip counter
    refresh, dropout, hip_decode = 1, 0.0, False      # weights re-packed every n-th call (a captured step needs 1); HipInnerSampler's two switches

    def __init__(self):
        self.calls, self.clip_counter, self.sync_ms = 0, 0, []     # calls made, clips drawn so far (all ranks), ms of each weight re-pack


class HipInnerSampler(InnerSampler):
    """The sampler and the decode on the HIP kernels.  refresh = n: amuse_update_weights every n-th call (1 = every iteration, the reference's semantics).
    dropout = p > 0: the reference's train-mode semantics on the same kernel - the Denoiser's encoder dropouts live in all steps (amuse_set_sample_dropout: masks
    keyed by the global clip index and the library's dropout epoch, so eager calls draw fresh masks through the clip counter and replays of a captured step
    through the epoch), and the decode is prior.decode on the trainer's own modules in train mode (the library's dropout-live layer kernels), on the trainer's
    stream after the join (decode_on_trainer_stream).  hip_decode (with dropout > 0): the decode stays in the library too - amuse_set_decode_dropout turns on the
    dropout instantiations of the staged decode kernels, masks keyed like the sampler's (seed + 2, the sample's clip base, the dropout epoch) - and on the
    sampler's side stream, off the trainer's critical stream."""

    def __init__(self, trainer_models: Dict[str, nn.Module], device, precision: str = "bf16", refresh: int = 1, seed: int = 2024,
                 ldm_cfg: Optional[dict] = None, flat: Optional[tuple] = None, rank: int = 0, world: int = 1, dropout: float = 0.0, hip_decode: bool = False):
        from .engine import HipEngine
        super().__init__()
        self.models, self.precision, self.refresh, self.seed = trainer_models, precision, max(1, refresh), seed
        self.flat = flat                        # (prior, denoiser) flat fp32 images that ARE the parameters (GestureTrainer.flat_param)
        self.engine = HipEngine(numpy_state(trainer_models["ldm"].denoiser), numpy_state(trainer_models["prior"]), device)
        self.engine.set_schedule(sch.from_ldm_cfg(ldm_cfg, "ddim") if ldm_cfg and "scheduler" in ldm_cfg else sch.ddim_table())
        self.rank, self.world = rank, world
        # the in-loop decode shares the GPU with the networks' forward pass (side stream): the per-clip kernel keeps it on `bsz` CUs (0.51 ms on 32 of 256) where the staged
        # launches AUTO would take below 64 clips spread over all of them (0.42 ms of 19 chip-wide launches in the forward pass's way)
        self.engine.set_decode_path("fused")
        self.what = {"bf16": 2, "fp32x": 8, "fp16": 16}.get(precision, 1)   # AMUSE_UPD_* mask of the streams this sampler runs
        self.on_device = True      # re-pack on the GPU straight from the trainer's flat parameter buffer (False: the host path of amuse_update_weights; tests)
        self.dropout = float(dropout)
        self.hip_decode = bool(hip_decode) and self.dropout > 0
        self.decode_on_trainer_stream = self.dropout > 0 and not self.hip_decode
        self.mode = "train-hip-decode" if self.hip_decode else "train-hip" if self.dropout > 0 else "eval"
        self._clip0 = 0            # clip base of the last sample: the decode's masks follow the sampler's clips
        if self.dropout > 0:
            self.engine.set_sample_dropout(self.dropout, seed=seed + 1)

    def __call__(self, con, emo, sty, bsz):
        return self.decode(self.sample_latents(con, emo, sty, bsz))

    def decode(self, lat):
        if self.hip_decode:       # train mode inside the library's decode kernels (a host-side switch: safe inside a captured step)
            self.engine.set_decode_dropout(self.dropout, seed=self.seed + 2, clip_index0=self._clip0)
        elif self.dropout > 0:    # train mode: the trainer's MotionPrior.decode, dropout live through the layer kernels
            return self.models["prior"].decode(lat[None], [SEQ_LEN] * lat.shape[0])
        return self.engine.vae_decode(lat, None, self.precision, return_feats=True)["feats"]

    def sample_latents(self, con, emo, sty, bsz):
        if self.calls % self.refresh == 0 and self.calls > 0:
            t0 = time.perf_counter()
            if self.on_device:
                # the weights never leave the GPU: the parameters ARE the flat images (or one torch.cat per network), then a gather kernel per packed image
                if self.flat is not None:
                    pri, den = self.flat
                else:
                    from .engine import flatten_on_device
                    from . import weights as wts
                    den = flatten_on_device(self.models["ldm"].denoiser.state_dict(), wts.denoiser_param_spec())
                    pri = flatten_on_device(self.models["prior"].state_dict(), wts.prior_param_spec())
                self.engine.update_weights_device(den, pri, what=self.what)
            else:
                self.engine.update_weights(numpy_state(self.models["ldm"].denoiser), numpy_state(self.models["prior"]), what=self.what)
            self.sync_ms.append((time.perf_counter() - t0) * 1e3)
        self.calls += 1
        if self.graph_safe:
            # inside a captured training step (GestureTrainer.enable_graph) the host-side clip counter would be frozen: the initial latents come from torch's
            # generator on the device, whose state the graph advances per replay
            # (with dropout live the clip index still keys the masks: rank r takes clips [r bsz, (r + 1) bsz), the epoch word advances per replay)
            self._clip0 = self.rank * bsz if self.dropout > 0 else 0
            return self.engine.sample(con, emo, sty, self.precision, seed=self.seed, x_init=torch.randn(bsz, 128, device=self.engine.device), clip_index0=self._clip0)
        # initial latents are keyed by a global clip index: rank r draws clips [counter + r * bsz, counter + (r + 1) * bsz)
        self._clip0 = self.clip_counter + self.rank * bsz
        lat = self.engine.sample(con, emo, sty, self.precision, seed=self.seed, clip_index0=self._clip0)
        self.clip_counter += bsz * self.world
        return lat


class TrainModeInnerSampler(InnerSampler):
    """OPT-IN: the reference's own form of the no-gradient half.  The reference calls `ldm.diffusion_backward` (DDIM-50, ldm.py:117-153) and `prior.decode` inside
    its training loop while both networks are in train() mode (trainer.py:357-358,413-415): every dropout of the Denoiser's nine encoder layers - attention weights,
    both residual branches, the FFN activation - and of the prior's decoder is LIVE in all 50 denoising steps and in the decode.  HipInnerSampler's default runs the
    persistent eval-mode kernel instead: ~10 x faster and, being deterministic, the better estimate of what the networks generate - a stated difference.  Here: the
    trainer's own modules as they are (train mode -> dropout through the library's counter-based masks, train_ops / k_train.hip; eval mode -> none), 50 x
    Denoiser.forward + the scheduler row update of amuse_amd/scheduler.py (the arithmetic the sampler kernels apply, tests/test_pins_cpu.py), one decode - on the
    trainer's stream (`serial`: these are the modules, and the library scratch, of the forward pass it follows).  Initial latents: the library's counter-based
    normals on the GPU (the HIP sampler's draw for the same clips), torch.randn from a seeded generator on the CPU."""
    mode, serial = "train", True

    def __init__(self, trainer_models: Dict[str, nn.Module], device, seed: int = 2024, ldm_cfg: Optional[dict] = None, rank: int = 0, world: int = 1, engine=None):
        super().__init__()
        self.models, self.device, self.seed, self.rank, self.world = trainer_models, torch.device(device), seed, rank, world
        self.table = sch.from_ldm_cfg(ldm_cfg, "ddim") if ldm_cfg and "scheduler" in ldm_cfg else sch.ddim_table()
        self.coef = torch.as_tensor(self.table.coef)            # (T, 8) host copy: the loop reads python floats, no device sync
        self.engine = engine                                    # a HipEngine to draw the initial latents from (GPU), or None

    def initial_latents(self, bsz: int) -> torch.Tensor:
        c0 = self.clip_counter + self.rank * bsz
        self.clip_counter += bsz * self.world
        if self.engine is not None:
            return self.engine.counter_normal(self.seed, c0, bsz, 0, 0)
        g = torch.Generator().manual_seed((self.seed * 1000003 + c0) & 0x7FFFFFFF)
        return torch.randn(bsz, 128, generator=g).to(self.device)

    @staticmethod
    def scheduler_update(row, x, eps, z=None):
        """One schedule row [sb, sa, c0, cx, ce, sigma, clip, 0] (include/amuse_hip.h amuse_schedule) in the kernels' operation order."""
        sb, sa, c0, cx, ce, sg, clipv = (float(v) for v in row[:7])
        x0 = (x - sb * eps) * (1.0 / sa)
        if clipv > 0:
            x0 = x0.clamp(-clipv, clipv)
        nx = c0 * x0
        if cx != 0:
            nx = nx + cx * x
        if ce != 0:
            nx = nx + ce * eps
        if sg != 0:
            nx = nx + sg * z
        return nx

    @torch.no_grad()
    def __call__(self, con, emo, sty, bsz, x_init: Optional[torch.Tensor] = None, return_latents: bool = False):
        den, prior = self.models["ldm"].denoiser, self.models["prior"]
        x = (self.initial_latents(bsz) if x_init is None else x_init.to(self.device)) * self.table.init_noise_sigma
        self.calls += 1
        for i, t in enumerate(self.table.timesteps):
            eps = den(x[:, None], int(t), con, emo, sty)[0][:, 0]
            z = torch.randn_like(x) if float(self.coef[i, 5]) != 0 else None          # (eta > 0 only)
            x = self.scheduler_update(self.coef[i], x, eps, z)
        feats = prior.decode(x[None], [SEQ_LEN] * bsz)
        return (feats, x) if return_latents else feats


# ------------------------------------------------------------------ the four modes, described once
class Mode(NamedTuple):
    text: str                # the bench line's config.inner_sampler, byte for byte (recorded lines are compared across rounds); also the help, the errors, the log
    needs_gpu: bool
    hip: Optional[dict]      # HipInnerSampler's arguments beyond the trainer's; None: TrainModeInnerSampler


MODES: Dict[str, Mode] = {
    "eval": Mode("eval: the persistent HIP sampler kernel (dropout off - the reference's loop runs in train mode; opt in with AMUSE_TRAIN_INNER=train-hip, or =train "
                 "for the module loop)", True, {"dropout": 0.0}),
    "train": Mode("train: the reference's train-mode loop, dropout live (TrainModeInnerSampler)", False, None),
    "train-hip": Mode("train-hip: the persistent HIP sampler kernel with the Denoiser's dropouts live + the train-mode prior.decode (the reference's semantics)", True, {}),
    "train-hip-decode": Mode("train-hip-decode: the persistent HIP sampler kernel with the Denoiser's dropouts live + the train-mode decode in the HIP decode kernels, "
                             "both on the sampler's stream (the reference's semantics)", True, {"hip_decode": True}),
}
MODES_TEXT = "; ".join(m.text for m in MODES.values())


def build(name: str, tr, device, rank: int, world: int, ldm_cfg, refresh: int, dropout: float, use_hip: bool = True) -> Optional[InnerSampler]:
    """The sampler of mode `name` on the models and flat parameters of GestureTrainer `tr`.  use_hip False: no HIP sampler is built (training without the
    gen_feature term) - and "eval", the default, then asks for nothing.  ValueError: no such mode; RuntimeError: a HIP mode on a device that is no GPU."""
    if name == "eval" and not use_hip:
        return None
    if name not in MODES:
        raise ValueError(f"inner sampler {name!r} is none of: {MODES_TEXT}")
    mode, on_gpu = MODES[name], torch.device(device).type == "cuda"
    if mode.needs_gpu and not on_gpu:
        raise RuntimeError(f"inner sampler {name!r} runs on the HIP kernels: there is no CPU path (use inner='train' on the CPU, or use_hip_sampler=False to "
                           "train without the no-gradient gen_feature term)")
    if mode.hip is None:      # the modules themselves (any device); on the GPU the initial latents are the HIP sampler's draws (only amuse_counter_normal is used)
        from .engine import HipEngine
        eng = HipEngine(numpy_state(tr.model["ldm"].denoiser), numpy_state(tr.model["prior"]), device) if on_gpu else None
        return TrainModeInnerSampler(tr.model, device, ldm_cfg=ldm_cfg, rank=rank, world=world, engine=eng)
    return HipInnerSampler(tr.model, device, refresh=refresh, ldm_cfg=ldm_cfg, flat=(tr.flat_param[:tr.n_prior], tr.flat_param[tr.n_prior:]), rank=rank, world=world,
                           **{"dropout": dropout, **mode.hip}) if use_hip else None
