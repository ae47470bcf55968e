"""Drop-in for the reference's `python main.py --fn {infer_gesture,edit_gesture} [--cfg base_new.json] [--wandb logger.json]`
(scripts/main.py:226-268 -> :113-222 -> trainer.eval_prior_latdiff_forward_backward_v1) for the path this library rebuilds:
WAV files in, SMPL-X NPZ files out, run from a reference-shaped tree.

  cd <amuse>/scripts && python -m amuse_amd.main --fn infer_gesture            # like the reference: dirname = cwd.parent
  python -m amuse_amd.main --fn edit_gesture --root <amuse>                     # or name the tree's root

What is read, exactly as the reference does (scripts/main.py:243-265):
  <root>/configs/base_new.json (or --cfg)          deep-merged with  <root>/scripts/overrides/<fn>.yaml
  <root>/configs/diff_latent_v2.json               deep-merged with  <root>/scripts/overrides/diff_o.yaml
  (prior_emotional_fing.json + prior_o.yaml only carry architecture constants the kernels are specialised for.)
The merge happens IN MEMORY: the reference rewrites the three JSON files on every start (main.py:263-265, and again
:22-26); this entry point never writes into the configuration tree.  The merged diff_latent_v2 is handed to
PretrainedLPDM_v1.setup through `config["_ldm_cfg_override"]`.
From the merged config: TRAIN_PARAM.baselines.renders.{custom_audios, custom_renders} (infer_gesture, trainer.py:507-508),
TRAIN_PARAM.test.emotion_control_list.{audios, renders, actor} (edit_gesture, trainer.py:1039-1043),
TRAIN_PARAM.test.replication_times, TRAIN_PARAM.seed, the checkpoint directories under <root>/saved-models.
The committed config carries the author's absolute paths (/home/kchhatre/...): --audios / --renders override the two
directories without touching the files.  Checkpoints: <root>/saved-models/<pretrained_lpdm>/{latdiff,prior}_*.pt and
<root>/saved-models/<pretrained_ast>/*.pt as the reference expects; --random-init substitutes the deterministic
random-init weights (no checkpoint ships with the reference) so that the path can be exercised end to end.

Outputs: <renders>/Custom_audios_<stamp>_E<epoch>/rep<i>/rst_<k>/seq_<n>/<actor>_seq_<n>_<rand6>_motion_smplx.npz
(trainer.py:534-538, visualizer.py:307-364).  Blender / ffmpeg rendering, wandb and the BEAT dataset objects
(dm.dm, LMDB) are out of scope; dataset-driven edit tasks take the dict `process_loader` receives via --eval-data.

Beyond the reference (which asks for 10 s WAVs, trainer.py:506): `--fn infer_gesture --long-form [--hop-frames 270]` turns a WAV of any length into ONE NPZ of
floor(30 x seconds) frames - overlapping 10 s windows, sampled independently, crossfaded where they overlap (amuse_amd/longform.py).  Off by default.
`--long-form-candidates K` samples K candidates of every window and joins the path of least seam cost (amuse_amd/seam.py).  Off by default (K = 1).
`--fn infer_gesture | edit_gesture --resample` converts a WAV of another rate to the 16 kHz the front-end is built for, in a HIP kernel
(amuse_amd/resample.py); the reference reads every file as 16 kHz whatever its header says.  Off by default.
`--fn infer_gesture | edit_gesture --preview --smplx-models DIR [--preview-size 512] [--preview-stride 10] [--preview-frames]` writes, beside every
*_motion_smplx.npz, *_preview.png - a contact sheet of the posed SMPL-X mesh, rasterised in HIP (amuse_amd/render.py) - and with --preview-frames
*_preview/frame_%04d.png.  A flat-shaded preview from a fixed front camera, not the reference's Blender render; the NPZ files keep their bytes.  Off by default.
With --preview-video [--preview-quality 90] also *_preview.avi: every frame as Motion-JPEG, encoded in HIP (amuse_amd/video.py), with the speech as 16-bit PCM.
`--fn infer_gesture | edit_gesture --smooth [--smooth-window 9] [--smooth-order 3] [--smooth-hands-window N]` passes every motion through a Savitzky-Golay
filter on SO(3) before it is written, in a HIP kernel (amuse_amd/smooth.py): this project's own statement of the method.  Off by default.
`--fn infer_gesture | edit_gesture --bvh --smplx-models DIR [--bvh-order ZYX] [--bvh-scale 100] [--bvh-unwrap]` writes, beside every *_motion_smplx.npz,
*_motion.bvh: the same motion as Biovision BVH of the SMPL-X skeleton, its MOTION block - Euler channels, as text - written by HIP kernels (amuse_amd/bvh.py).
The NPZ files keep their bytes.  Off by default.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import time
from contextlib import closing
from pathlib import Path

import numpy as np
import torch

from . import audio_weights as aw
from . import weights as wts
from .infer_ldm import PretrainedLPDM_v1
from .trainer import trainer


def fixseed(seed: int):
    """scripts/utils/misc.py:93-101."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def merge_dicts(config: dict, override_dict) -> dict:
    """scripts/main.py:245-256 (recursive, in place on a shallow copy - nested dicts of `config` are updated)."""
    def merge_recursive(original, override):
        for key, value in override.items():
            if isinstance(value, dict) and key in original and isinstance(original[key], dict):
                merge_recursive(original[key], value)
            else:
                original[key] = value
    if override_dict is None:
        return config
    result = config.copy()
    merge_recursive(result, override_dict)
    return result


def load_config(root: Path, fn: str, cfg_path=None):
    """-> (base config, diff_latent_v2 config), each merged with its override YAML, nothing written back."""
    import yaml
    out = []
    for override, cfg in ((f"{fn}.yaml", cfg_path or root / "configs" / "base_new.json"),
                          ("diff_o.yaml", root / "configs" / "diff_latent_v2.json")):
        config_dict = json.load(open(cfg))
        ov = root / "scripts" / "overrides" / override
        override_dict = yaml.safe_load(open(ov)) if ov.exists() else None
        out.append(merge_dicts(config_dict, override_dict))
    return out[0], out[1]


def train_gesture_entry(args, dirname: Path, config: dict):
    """--fn train_gesture (scripts/main.py:116-155): the LPDM trainer on the latent-diffusion LMDB cache named by the
    configuration - batch size, epochs, save frequency and cache path from base_new.json + scripts/overrides/train_gesture.yaml -
    through amuse_amd.train_gesture's own entry point (one process per GPU with --gpus N)."""
    from . import train_gesture
    tp = config["TRAIN_PARAM"]
    assert not tp["pretrained_infer"], f"Arg: train_gesture and pretrained_infer: {tp['pretrained_infer']} mismatch!"   # main.py:126
    assert tp["motion_extractor"]["use"] is False, "Motion extractor should be False!"
    ld = tp["latent_diffusion"]
    assert ld.get("smplx_data", True), "smplx_data must be True!"                                                        # main.py:129
    # what the configuration asks for beyond the defaults (trainer.py:94-104,177-184): refuse what this path cannot do instead of
    # silently training another objective
    if ld.get("optimizer_name", "adamw") != "adamw":
        raise SystemExit(f"train_gesture: optimizer_name {ld.get('optimizer_name')!r}: the reference's LPDM trainer builds AdamW only (trainer.py:184)")
    # the two vertex-displacement terms (latent_losses.py:135-146,173-250) need the user's own SMPL-X model files (licensed; the reference's trainer.py:94-104
    # loads them from <root>/body_models/codebase/models/smplx)
    smplx_dir = None
    if ld.get("vtex_displacement", False) and not args.skip_vtex_loss:
        from . import body
        smplx_dir = Path(args.smplx_models) if args.smplx_models else dirname / "body_models" / "codebase" / "models" / "smplx"
        body.require_models(smplx_dir, "train_gesture: TRAIN_PARAM.latent_diffusion.vtex_displacement is True (scripts/overrides/train_gesture.yaml:25): the "
                            "rec / gen vertex-displacement loss terms need the licensed SMPL-X body models (latent_losses.py:173-250), and ",
                            "(--smplx-models DIR names another directory).  Pass --skip-vtex-loss to train WITHOUT those two terms (checkpoint names then read "
                            "vtexR0.0000 / vtexG0.0000), or set vtex_displacement: False", load=False)
    elif ld.get("vtex_displacement", False):
        print("[LPDM-T] WARNING: vtex_displacement is True in the configuration but --skip-vtex-loss drops both vertex-displacement terms", flush=True)
    ldm_cfg = config.get("_ldm_cfg")
    argv = ["--batch", str(ld.get("batch_size", 32)), "--epochs", str(args.epochs or ld.get("n_epochs", 12000)),
            "--save-freq", str(ld.get("model_save_freq", 200)), "--seed", str(tp.get("seed", 2024)), "--gpus", str(args.gpus),
            "--out", str(dirname / "saved-models"), "--lr", repr(float(ld.get("lr_base", 1e-4)))]
    tmp_cfg = None
    if ldm_cfg is not None:   # configs/<arch>.json merged with diff_o.yaml: loss weights and both schedulers (the ranks may be other processes)
        import tempfile
        f = tempfile.NamedTemporaryFile("w", suffix="_ldm_cfg.json", delete=False)
        json.dump(ldm_cfg, f)
        f.close()
        tmp_cfg = f.name
        argv += ["--ldm-cfg", tmp_cfg]
    cache = dirname / "data" / "BEAT-processed" / tp.get("diffusion", {}).get("lmdb_cache", "")
    if not args.synthetic:
        if not (cache.is_dir() and tp.get("diffusion", {}).get("lmdb_cache")):
            raise SystemExit(f"train_gesture: the LMDB cache {cache} does not exist (prepare_data is the reference's job; --synthetic trains "
                             f"on random batches of the collate function's shapes)")
        argv += ["--cache", str(cache)]     # (the ablation variant is derived from this id, trainer.py:396-401)
    elif tp.get("diffusion", {}).get("lmdb_cache"):
        from .train_gesture import ablation_kind
        argv += ["--kind", ablation_kind(tp["diffusion"]["lmdb_cache"])]
    if args.device != "cuda:0":
        argv += ["--device", args.device]
    if args.iters_per_epoch:
        argv += ["--iters-per-epoch", str(args.iters_per_epoch)]
    if smplx_dir is not None:
        version = str(tp.get("wav_dtw_mfcc", {}).get("ablation_version") or "v0")
        if version not in ("v0", "v1"):
            raise SystemExit(f"train_gesture: TRAIN_PARAM.wav_dtw_mfcc.ablation_version is {version!r}: the vertex-displacement terms know the dataset versions "
                             "v0 (male / female body model by the actor) and v1 (neutral), as latent_losses.py:184-199 does")
        argv += ["--smplx-models", str(smplx_dir), "--dataset-version", version]
        if args.vtex_grad:
            argv += ["--vtex-grad"]
    print(f"Experiment init: AMUSE, fn: train_gesture, time: {time.asctime()}")
    try:
        return train_gesture.main(argv)
    finally:
        if tmp_cfg is not None:       # (the ranks have finished reading it: main returns after they exit)
            try:
                os.unlink(tmp_cfg)
            except OSError:
                pass


def _launch_ranks(args, argv, dirname: Path):
    """`--fn infer_gesture | edit_gesture --gpus N` typed directly: this process never touches the GPU; it starts N ranks of this very module as
    CHILD processes (amuse_amd/launch.py: torch.distributed.run, never exec), hands them ONE time stamp for the output directory and a scratch
    directory for their manifests, and returns the paths all ranks wrote (rank order = job order)."""
    import sys
    import tempfile
    from datetime import datetime
    from . import launch
    av = list(sys.argv[1:] if argv is None else argv)
    if args.root is None:                      # the ranks start in another process: name the tree explicitly
        av += ["--root", str(dirname)]
    with tempfile.TemporaryDirectory(prefix="amuse_ranks_") as md:
        had_stamp = "AMUSE_RUN_STAMP" in os.environ
        os.environ["AMUSE_RUN_STAMP"] = os.environ.get("AMUSE_RUN_STAMP") or datetime.now().strftime("%Y%m%d-%H%M%S")
        os.environ["AMUSE_MANIFEST_DIR"] = md
        try:
            rc = launch.run_ranks("amuse_amd.main", av, args.gpus, module=True)
        finally:
            os.environ.pop("AMUSE_MANIFEST_DIR", None)
            if not had_stamp:
                os.environ.pop("AMUSE_RUN_STAMP", None)      # (the stamp is this run's: a later run in the same process draws its own)
        if rc != 0:
            raise SystemExit(rc)
        written = []
        for r in range(args.gpus):
            f = Path(md, f"rank{r}.json")
            written += [Path(p) for p in json.loads(f.read_text())] if f.exists() else []
    print(f"AMUSE: ({args.fn[0]}) {args.gpus} ranks wrote {len(written)} NPZ files")
    return written


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="AMUSE (MI355X path)")
    ap.add_argument("--fn", nargs="*", required=True, help="infer_gesture, edit_gesture, train_gesture")
    ap.add_argument("--cfg", default=None, help="config file (default <root>/configs/base_new.json)")
    ap.add_argument("--wandb", default=None, help="accepted for command-line compatibility; wandb is out of scope")
    ap.add_argument("--root", default=None, help="the reference-shaped tree (default: cwd.parent, scripts/main.py:229)")
    ap.add_argument("--audios", default=None, help="override custom_audios / emotion_control_list.audios")
    ap.add_argument("--renders", default=None, help="override custom_renders / emotion_control_list.renders")
    ap.add_argument("--eval-data", default=None, help="torch-saved dict for process_loader (dataset-driven edit tasks)")
    ap.add_argument("--epoch", default="6000", help="checkpoint epoch; the reference hard-codes 6000 (main.py:155-157,193); 'best' = lowest total loss")
    ap.add_argument("--random-init", action="store_true", help="deterministic random-init weights instead of checkpoints")
    ap.add_argument("--sampler", default="ddim", choices=["ddim", "ddpm"])
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--precision", default="fp32x", choices=["fp32", "bf16", "fp32x", "fp16"],
                    help="fp32x (default): results match the reference's fp32 modules (eps_hat <= 1e-5) on the 16-bit MFMA; fp32: the same bars on "
                         "the fp32 MFMA, 2.6 x slower; fp16: the throughput mode (2 x fp32x, ~3e-3 on eps_hat; operands must stay below 65504: an "
                         "overflow surfaces as a non-finite output); bf16: the same speed with 8 x the rounding - only for activations beyond fp16 range")
    ap.add_argument("--audio-precision", default="bf16", choices=["bf16", "fp32x"],
                    help="arithmetic of the audio front-end (fbank + 3 x AST) of infer_gesture / edit_gesture.  bf16 (default): bf16 operands, embeddings ~5e-3 off the "
                         "fp32 encoders; fp32x: split-fp16 operands, embeddings within 1e-5 - the mode in which a --precision fp32x run is in parity FROM THE WAVEFORM "
                         "(1.04 GB more device memory for the weight images, several times the front-end's time)")
    ap.add_argument("--audio-metrics", action="store_true",
                    help="infer_gesture: also write <rep>/rst_0/<audio stem>/audio_metrics/fbank.pkl for every audio - the dict of the reference's "
                         "collect_audio_metrics (encoder features + predicted emotion / speaker labels, the fbank AST_EVP's fusion + decoder reconstruct from "
                         "them, and the encoders' outputs on that reconstruction).  Needs an AST checkpoint that holds the fusion / decoder / classifier heads")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--gpus", type=int, default=1, help="one process per GPU on this node: train_gesture = data-parallel ranks (RCCL all-reduce); infer_gesture / "
                                                         "edit_gesture = the job list cut into contiguous ranges, each rank embeds, samples and writes its own (no collective; "
                                                         "the NPZ files are byte for byte the single-process run's)")
    ap.add_argument("--all-pairs", action="store_true", help="edit_gesture: every *_source.wav edited with the emotion of every *_target.wav (S x T jobs) instead of "
                                                             "the reference's first source / first target pair (sets TRAIN_PARAM.test.emotion_control_list.all_pairs)")
    ap.add_argument("--epochs", type=int, default=None, help="train_gesture: override TRAIN_PARAM.latent_diffusion.n_epochs")
    ap.add_argument("--synthetic", action="store_true", help="train_gesture: synthetic batches instead of the LMDB cache")
    ap.add_argument("--iters-per-epoch", type=int, default=None, help="train_gesture --synthetic: iterations per epoch")
    ap.add_argument("--skip-vtex-loss", action="store_true", help="train_gesture: train without the two vertex-displacement loss terms when the "
                                                                  "configuration asks for them (they need the SMPL-X body models)")
    ap.add_argument("--vtex-grad", action="store_true", help="train_gesture: the vertex-displacement terms carry gradient to the decoder (needs --smplx-models); a "
                                                             "deviation from the reference, whose vertices are computed under no_grad (latent_losses.py:173)")
    ap.add_argument("--smplx-models", default=None, help="train_gesture: directory holding SMPLX_MALE.npz, SMPLX_FEMALE.npz, SMPLX_NEUTRAL.npz for the vertex-displacement "
                                                         "loss terms (default: <root>/body_models/codebase/models/smplx, the reference's path)")
    ap.add_argument("--long-form", action="store_true",
                    help="infer_gesture: a WAV of ANY length becomes one motion of floor(30 x seconds) frames - an extension, the reference asks for 10 s WAVs. "
                         "The waveform is cut into overlapping 10 s windows, every window is sampled as a clip of its own (independently: nothing is shared "
                         "between windows) and the frames two neighbouring windows both produced are crossfaded, which hides the seam but does not make the "
                         "windows agree.  A WAV of at most 160,000 samples gives the bytes it gives without the switch")
    ap.add_argument("--hop-frames", type=int, default=270, help="--long-form: frames between window starts, a multiple of 3 in 150..300 (default 270: one second "
                                                                "of overlap; 300: plain concatenation)")
    ap.add_argument("--long-form-candidates", type=int, default=1, metavar="K",
                    help="--long-form: K candidates of every window (1..64, default 1: nothing changes by a bit) are sampled in the WAV's one batch, every pair "
                         "of neighbouring windows' candidates is scored by how far their shared frames are apart as rotations, and the windows on the path of "
                         "least total seam cost are the ones joined - all in HIP kernels (amuse_amd/seam.py).  An extension and this project's own method, "
                         "compared with no other implementation; whether a trained checkpoint's candidates differ enough at the seams for the choice to matter "
                         "has not been measured.  A WAV of one window is not expanded.  One line per WAV reports the cost of the all-first-candidates path "
                         "-> the chosen path's.  The NPZ layout is unchanged; needs an overlap (--hop-frames below 300)")
    ap.add_argument("--resample", action="store_true",
                    help="infer_gesture / edit_gesture: a WAV whose header states another rate than 16,000 Hz is converted to 16 kHz on the GPU before the "
                         "front-end reads it - an extension, the reference drops the rate and reads every file as 16 kHz (so a 48 kHz recording is animated as "
                         "speech slowed three times).  The filter is a Hann-windowed sinc written down from memory of torchaudio's defaults, pinned against no "
                         "other implementation.  A 16 kHz file gives the bytes it gives without the switch; works with --long-form and --audio-metrics")
    ap.add_argument("--preview", action="store_true",
                    help="infer_gesture / edit_gesture: beside every *_motion_smplx.npz write *_preview.png, a contact sheet of the posed SMPL-X mesh rasterised in a "
                         "HIP kernel (amuse_amd/render.py) - an extension: a flat-shaded preview from a fixed front camera, not the reference's Blender render.  Needs "
                         "the SMPL-X model files with their triangles (--smplx-models DIR).  The NPZ files keep their bytes; works with --long-form, --resample, --gpus N")
    ap.add_argument("--preview-size", type=int, default=512, help="--preview: pixels per side of a frame")
    ap.add_argument("--preview-stride", type=int, default=10, help="--preview: every stride-th frame goes on the sheet")
    ap.add_argument("--preview-frames", action="store_true", help="--preview: also write *_preview/frame_%%04d.png for every frame")
    ap.add_argument("--preview-video", action="store_true",
                    help="--preview: also write *_preview.avi - every frame as Motion-JPEG, encoded in HIP kernels while still on the device, with the speech as "
                         "16-bit PCM (amuse_amd/video.py): infer_gesture muxes the job's WAV (with --long-form the whole WAV against the whole motion), edit_gesture "
                         "the content source WAV, a dataset-driven edit (--eval-data) clip c of its take's ld_waveform (16 kHz) when the dictionary holds one; a motion whose audio the run does not hold gets the video stream alone.  A preview encoder (fixed Huffman "
                         "tables, no chroma subsampling), an AVI 1.0 file (below 2 GiB)")
    ap.add_argument("--preview-quality", type=int, default=None, help="--preview-video: JPEG quality 1..100 (default 90)")
    ap.add_argument("--motion-metrics", action="store_true",
                    help="edit tasks on the dataset (--eval-data): after every task, APE / AVE / velocity / acceleration on posed SMPL-X joints (summed per clip in a HIP "
                         "kernel) and FID / Diversity on the motion prior's latents, between every generated motion and its source motion, written to "
                         "<model_path>/viz/motion_metrics_<stamp>_E<epoch>.json (amuse_amd/motion_metrics.py) - an extension: the reference's val_metrics.py cannot "
                         "run and its trainer passes metricsmodel=None.  Needs the SMPL-X model files (--smplx-models DIR); works under metrics_only: True")
    ap.add_argument("--metrics-diversity-times", type=int, default=300, help="--motion-metrics: clips per index set of the Diversity draw (it needs more clips than this)")
    ap.add_argument("--beat-align", action="store_true",
                    help="infer_gesture: after the run, every WAV is scored against the motion its NPZ holds - speech onsets of the waveform the front-end read against "
                         "the motion beats (local minima of joint speed) of the posed SMPL-X joints, all in HIP kernels - and "
                         "<model_path>/viz/beat_align_<stamp>_E<epoch>.json is written (amuse_amd/beat_align.py).  An extension and this project's own statement of the "
                         "metric: not compared with librosa or with BEAT's code.  Needs the SMPL-X model files (--smplx-models DIR); the NPZ files keep their bytes; "
                         "works with --long-form, --resample, --gpus N")
    ap.add_argument("--smooth", action="store_true",
                    help="infer_gesture / edit_gesture: every motion goes through a Savitzky-Golay filter over time before it is written - on SO(3) for the joints (the "
                         "polynomial fit in the tangent space at the frame being filtered, in a HIP kernel: amuse_amd/smooth.py), on R^3 for the translation; with "
                         "--long-form after the join, so across the seams as well.  An extension, off by default, and this project's own statement of the method: "
                         "pinned against no other implementation, except its Euclidean half against scipy.  The NPZ, --motion-metrics, --beat-align and --preview see "
                         "the smoothed motion; works with --long-form, --resample, --gpus N.  `python -m amuse_amd.smooth` filters the NPZ of an earlier run")
    ap.add_argument("--smooth-window", type=int, default=None, help="--smooth: frames per window, odd, 3..31 (default 9; with --smooth-order 3 at 30 fps a "
                                                                     "recollection of common practice, not a measurement)")
    ap.add_argument("--smooth-order", type=int, default=None, help="--smooth: polynomial order 0..5 (default 3)")
    ap.add_argument("--smooth-hands-window", type=int, default=None, help="--smooth: another window for the 30 finger joints (default: --smooth-window)")
    ap.add_argument("--bvh", action="store_true",
                    help="infer_gesture / edit_gesture: beside every *_motion_smplx.npz write *_motion.bvh (and *_motion.bvh.json: gender, betas, scale) - what the NPZ "
                         "holds as Biovision BVH of the SMPL-X skeleton, Euler channels in degrees, the MOTION block converted and formatted in HIP kernels "
                         "(amuse_amd/bvh.py) - an extension: the SMPL-X skeleton itself, not the reference's Blender retargeting; no BVH importer is pinned.  Needs "
                         "--smplx-models DIR (the rest joints).  Works with --long-form, --resample, --smooth, --gpus N.  `python -m amuse_amd.bvh` converts the "
                         "NPZ of an earlier run, and back")
    ap.add_argument("--bvh-order", default=None, help="--bvh: rotation channel order, one of XYZ XZY YXZ YZX ZXY ZYX (default ZYX)")
    ap.add_argument("--bvh-scale", type=float, default=None, help="--bvh: length units per metre (default 100: centimetres)")
    ap.add_argument("--bvh-unwrap", action="store_true", help="--bvh: continuous curves - each frame takes the Euler triple nearest the frame before")
    return ap


def _needs_smplx(args, flag: str, reason: str) -> None:
    """`flag` poses bodies: --smplx-models DIR must be given and hold the three model files - checked before anything is loaded or sampled"""
    from . import body
    if not args.smplx_models:
        raise SystemExit(f"{flag} needs --smplx-models DIR: {reason}")
    body.require_models(args.smplx_models, f"{flag}: ", load=False)


def check_switches(args):
    """Every refusal a command line gets before the configuration is read, in a fixed order -> the checked options of --smooth and --bvh (None: switch off)"""
    fn = args.fn[0]
    if fn not in ("infer_gesture", "edit_gesture", "train_gesture"):
        raise SystemExit(f"--fn {fn}: infer_gesture, edit_gesture and train_gesture run on this path")
    if args.vtex_grad and (fn != "train_gesture" or not args.smplx_models):
        raise SystemExit("--vtex-grad belongs to --fn train_gesture and needs --smplx-models DIR: the vertex-displacement terms it differentiates are built from the "
                         "SMPL-X body models")
    if args.resample and fn == "train_gesture":
        raise SystemExit("--resample belongs to --fn infer_gesture / edit_gesture: it converts the WAVs those read; the training reader is left as it is")
    if (args.preview or args.preview_frames or args.preview_video) and fn == "train_gesture":
        raise SystemExit("--preview belongs to --fn infer_gesture / edit_gesture: it draws the NPZ files those write")
    if args.preview_frames and not args.preview:
        raise SystemExit("--preview-frames belongs to --preview")
    if args.preview_video and not args.preview:
        raise SystemExit("--preview-video belongs to --preview")
    if args.preview_quality is not None and not args.preview_video:
        raise SystemExit("--preview-quality belongs to --preview-video")
    if args.preview_quality is not None and not 1 <= args.preview_quality <= 100:
        raise SystemExit(f"--preview-quality {args.preview_quality} outside 1..100")
    if args.motion_metrics:
        if fn == "train_gesture":
            raise SystemExit("--motion-metrics belongs to --fn infer_gesture / edit_gesture: it evaluates the pairs the edit tasks collect")
        _needs_smplx(args, "--motion-metrics", "APE / AVE are taken on the joints the SMPL-X body models pose")
        if args.metrics_diversity_times < 1:
            raise SystemExit(f"--metrics-diversity-times {args.metrics_diversity_times}: at least 1")
    if args.beat_align:
        if fn != "infer_gesture":
            raise SystemExit("--beat-align belongs to --fn infer_gesture: it scores every WAV against the motion generated from it (which WAV an edited motion "
                             "should align with is a separate question)")
        _needs_smplx(args, "--beat-align", "the motion beats are taken on the joints the SMPL-X body models pose")
    smooth_opts = None
    if not args.smooth and any(v is not None for v in (args.smooth_window, args.smooth_order, args.smooth_hands_window)):
        raise SystemExit("--smooth-window / --smooth-order / --smooth-hands-window belong to --smooth")
    if args.smooth:
        if fn == "train_gesture":
            raise SystemExit("--smooth belongs to --fn infer_gesture / edit_gesture: it filters the motions those write")
        from . import smooth as smooth_mod
        try:               # checked before anything is loaded or sampled
            smooth_opts = smooth_mod.options(args.smooth_window, args.smooth_order, args.smooth_hands_window)
        except ValueError as e:
            raise SystemExit(f"--smooth: {e}")
    bvh_opts = None
    if not args.bvh and (args.bvh_order is not None or args.bvh_scale is not None or args.bvh_unwrap):
        raise SystemExit("--bvh-order / --bvh-scale / --bvh-unwrap belong to --bvh")
    if args.bvh:
        if fn == "train_gesture":
            raise SystemExit("--bvh belongs to --fn infer_gesture / edit_gesture: it converts the NPZ files those write")
        _needs_smplx(args, "--bvh", "the hierarchy's offsets are the rest joints of the SMPL-X body models")
        from . import bvh as bvh_mod
        try:
            bvh_opts = bvh_mod.options(args.bvh_order, args.bvh_scale, args.bvh_unwrap)
        except ValueError as e:
            raise SystemExit(f"--bvh: {e}")
    if args.long_form and fn != "infer_gesture":
        raise SystemExit("--long-form belongs to --fn infer_gesture: it joins the windows of one WAV into one motion; the edit tasks work on 10 s clips")
    if args.long_form:
        from . import _lib, longform
        try:
            longform.plan(0, args.hop_frames)      # the library's own check of the hop, before anything is loaded
        except _lib.AmuseHipError as e:
            raise SystemExit(f"--hop-frames {args.hop_frames}: {e}")
    if args.long_form_candidates != 1:
        if not args.long_form:
            raise SystemExit("--long-form-candidates belongs to --long-form: it chooses among candidates of a long WAV's windows")
        from . import seam
        if not 1 <= args.long_form_candidates <= seam.MAX_CANDIDATES:
            raise SystemExit(f"--long-form-candidates {args.long_form_candidates} outside 1..{seam.MAX_CANDIDATES}")
        if args.hop_frames >= 300:
            raise SystemExit(f"--long-form-candidates needs frames that two windows share: --hop-frames {args.hop_frames} leaves none")
    return smooth_opts, bvh_opts


def long_form_config(args, test_cfg: dict) -> None:
    """--long-form [--hop-frames H] [--long-form-candidates K] -> TRAIN_PARAM.test (the keys are this path's own; without a switch the configuration is left as
    it is, and long_form_candidates is written only when K > 1)"""
    if args.long_form:
        test_cfg["long_form"], test_cfg["hop_frames"] = True, int(args.hop_frames)
        if args.long_form_candidates > 1:
            test_cfg["long_form_candidates"] = int(args.long_form_candidates)


def post_run(args, tr, written, models, bvh_opts, device) -> None:
    """This rank's own NPZ files after the run: the preview, then the BVH export - of what the files hold (lower body frozen, the stitch, the smoothing)"""
    if args.preview:
        from . import render
        from .video import preview_wav
        with closing(render.Previewer(models, device, args.preview_size, args.preview_stride, args.preview_frames, video=args.preview_video,
                                      quality=90 if args.preview_quality is None else args.preview_quality)) as pv:
            drawn = [f for p in written for f in pv.preview(p, wav=preview_wav(tr.preview_audio.get(str(p))) if args.preview_video else None)]
        n_avi = sum(1 for f in drawn if Path(f).suffix == ".avi")
        print(f"[amuse_amd] --preview: {len(drawn) - n_avi} PNG files" + (f" and {n_avi} AVI files" if n_avi else "") + f" beside {len(written)} NPZ files")
    if bvh_opts is not None:            # in one batch
        from . import bvh as bvh_mod
        try:
            n_bvh = len(bvh_mod.motion_to_bvh_batch(written, models, device=device, **bvh_opts))
        except bvh_mod.BvhRangeError as e:
            raise SystemExit(f"--bvh: {e}")
        print(f"[amuse_amd] --bvh: {n_bvh} BVH files beside {len(written)} NPZ files")


def main(argv=None):
    args = build_parser().parse_args(argv)
    fn = args.fn[0]
    smooth_opts, bvh_opts = check_switches(args)
    tic = time.time()
    dirname = Path(args.root) if args.root else Path.cwd().parent
    config, ldm_cfg = load_config(dirname, fn, args.cfg)
    tp = config["TRAIN_PARAM"]
    if fn == "train_gesture":
        config["_ldm_cfg"] = ldm_cfg
        return train_gesture_entry(args, dirname, config)
    models = None             # the SMPL-X body models of --preview / --motion-metrics / --beat-align / --bvh: one directory, read once for all of them
    if args.preview:          # checked before anything is loaded or sampled: the model files, and their triangles
        from . import render
        models = render.load_preview_models(Path(args.smplx_models) if args.smplx_models else dirname / "body_models" / "codebase" / "models" / "smplx")
        if args.preview_size < 1 or args.preview_size > 1024 or args.preview_stride < 1:
            raise SystemExit(f"--preview-size {args.preview_size} (1..1024: the renderer takes 2048 samples per axis at 2 x supersampling) / --preview-stride "
                             f"{args.preview_stride} (>= 1)")
    from . import launch
    if args.gpus > 1 and not launch.launched_by_torchrun():
        return _launch_ranks(args, argv, dirname)
    world, rank, local_rank = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world > 1:
        if args.device not in ("cuda", "cuda:0") and os.environ.get("AMUSE_SHARE_GPU") != "1":
            raise SystemExit(f"--device {args.device} with {world} ranks would put every rank on one GPU: drop the index (rank r uses cuda:<LOCAL_RANK>)")
        if os.environ.get("AMUSE_SHARE_GPU") != "1":     # (tests on a one-GPU box: AMUSE_SHARE_GPU=1 keeps every rank on --device)
            args.device = f"cuda:{local_rank}"
        torch.cuda.set_device(torch.device(args.device))
    if args.all_pairs:
        tp["test"].setdefault("emotion_control_list", {})["all_pairs"] = True
    pg = False
    if world > 1 and (args.motion_metrics or args.beat_align or (fn == "edit_gesture" and tp["test"].get("emotion_control_list", {}).get("all_pairs"))):
        # the ONE exchange of the inference path: S sources x T targets - every rank's jobs read most WAVs, so each rank embeds a share and
        # the embeddings (3 x 256 floats per WAV) are all-gathered.  RCCL between the GPUs; gloo when the ranks share a device (tests).
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("AMUSE_SHARE_GPU") == "1":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(args.device))
        pg = True
    assert tp["pretrained_infer"], f"Arg: {fn} and pretrained_infer: {tp['pretrained_infer']} mismatch!"   # main.py:129
    assert tp["motion_extractor"]["use"] is False, "Motion extractor should be False!"
    if args.audios or args.renders:
        r, ecl = tp["baselines"]["renders"], tp["test"].get("emotion_control_list", {})
        if args.audios:
            r["custom_audios"], ecl["audios"] = args.audios, args.audios
        if args.renders:
            r["custom_renders"], ecl["renders"] = args.renders, args.renders
    device = torch.device(args.device)
    processed = dirname / "data" / "BEAT-processed"
    model_path = dirname / "saved-models"
    print(f"Experiment init: AMUSE, device: {device}, time: {time.asctime()}")
    fixseed(tp["seed"])
    print(f"Inferring for epoch {args.epoch}")
    tp["latent_diffusion"]["pretrained_prior_lpdm_e"] = args.epoch if args.epoch == "best" else int(args.epoch)
    tp["latent_diffusion"]["pretrained_ldm_lpdm_e"] = tp["latent_diffusion"]["pretrained_prior_lpdm_e"]
    baseline, modelversion, diffonly = False, tp["wav_dtw_mfcc"]["ablation"], tp["test"]["diff_only"]
    audio_list = tp["test"]["audio_list"]["use"]
    short_audio_list = tp["test"]["audio_list"]["short_audio_list"]
    if args.random_init:
        print("[amuse_amd] --random-init: deterministic random-init denoiser / prior / AST weights (seed 0)")
        model = PretrainedLPDM_v1.from_state_dicts(wts.make_denoiser_weights(0), wts.make_prior_weights(0), ldm_cfg,
                                                   device, seed=tp["seed"])
        for k in ("style_transfer", "emotion_control", "content_control", "style_Xemo_transfer"):
            setattr(model, k, tp["test"][k]["use"])
        wd = tp["wav_dtw_mfcc"]
        model.set_audio_encoders(*(aw.make_ast_weights(0, n) for n in aw.ENCODERS), wd.get("dataset_mean", -9.173025),
                                 wd.get("dataset_std", 5.062332), wd.get("frame_based_feats", True), precision=args.audio_precision,
                                 tail_sd=aw.make_ast_tail_weights(0) if args.audio_metrics else None)
        ldm_epoch = 0
    else:
        config["_ldm_cfg_override"] = ldm_cfg
        tp["wav_dtw_mfcc"]["audio_precision"] = args.audio_precision
        model = PretrainedLPDM_v1(None)
        ldm_epoch = model.setup(config, device, processed, None, False, baseline, verbose=False, diffonly=diffonly)
    tp["test"]["audio_metrics"] = bool(args.audio_metrics)
    if args.resample:        # (as below: the key is this path's own; without the switch the configuration is left as it is)
        tp["test"]["resample"] = True
    long_form_config(args, tp["test"])
    if smooth_opts is not None:     # (as above: the key is this path's own)
        tp["test"]["smooth"] = smooth_opts
    if args.motion_metrics:  # (the keys are this path's own; without the switch the configuration is left as it is)
        tp["test"]["motion_metrics"], tp["test"]["metrics_diversity_times"] = True, int(args.metrics_diversity_times)
    if args.beat_align:      # (as above: the key is this path's own)
        tp["test"]["beat_align"] = True
    if models is None and (args.motion_metrics or args.beat_align or args.bvh):
        from . import body
        models = body.require_models(args.smplx_models, "--smplx-models: ")
    model.precision = args.precision
    print(f"[amuse_amd] sampler / decoder precision: {args.precision}; audio front-end precision: {args.audio_precision}"
          + (" (split-fp16 AST encoders: with --precision fp32 / fp32x the run is in parity from the waveform)" if args.audio_precision == "fp32x"
             else " (bf16 AST encoders: the embeddings carry bf16 rounding; --audio-precision fp32x is the mode in which a --precision fp32x run is in parity "
                  "from the waveform)"))
    model.set_sampler(args.sampler, args.steps)
    eval_loader = torch.load(args.eval_data, weights_only=False) if args.eval_data else None
    tr = trainer(config, device, train_loader=eval_loader, model_path=model_path, tag="LPDM_infer", logger_cfg=None,
                 model=model, processed=processed, metricsmodel=None, b_path=None, EXEC_ON_CLUSTER=False,
                 debug=tp.get("debug", True), pretrained_infer=True, rank=rank, world=world, body_models=models if args.motion_metrics or args.beat_align else None)
    written = tr.eval_prior_latdiff_forward_backward_v1(baseline, ldm_epoch, audio_list, short_audio_list,
                                                        modelversion=modelversion, ammetric=True)
    torch.cuda.synchronize()
    post_run(args, tr, written, models, bvh_opts, device)
    print(f"AMUSE: ({fn}) completed in: {(time.time() - tic) / 3600} hrs; {len(written)} NPZ files" + (f" on rank {rank} of {world}" if world > 1 else ""))
    if world > 1 and os.environ.get("AMUSE_MANIFEST_DIR"):      # the launcher collects what the ranks wrote
        Path(os.environ["AMUSE_MANIFEST_DIR"], f"rank{rank}.json").write_text(json.dumps([str(p) for p in written]))
    if pg:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return written


if __name__ == "__main__":
    main()
