/*
 * amuse_hip.h - C ABI of libamuse_hip.so: the MI355X (gfx950) implementation of AMUSE's
 * latent-diffusion gesture-sampling hot path.
 *
 * The reference (kiranchhatre/amuse) has NO native/FFI seam on this path: the boundary is the Python
 * object protocol of models/latent_diffusion/infer_ldm.py (PretrainedLPDM_v1).  Each entry point
 * below names the reference interface it replaces (paths relative to the reference root); the
 * ctypes binding a maintainer adds on the reference side is shown in INTEGRATION.md and shipped in
 * amuse_amd/_lib.py.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no torch/HIP types in signatures (hipStream_t travels as void*)
 *   - every `dev` pointer is DEVICE memory on the ctx's GPU, fp32, row-major, caller-owned;
 *     every `host` pointer is host memory; inputs are never written, outputs are fully overwritten
 *   - return 0 on success, a negative AMUSE_E* code on failure; amuse_last_error() gives the text
 *     (thread-local).  No exceptions cross the ABI.
 *   - one ctx per (GPU, weight set); calls on one ctx must not overlap in time (they share workspace)
 *   - kernels are enqueued on `stream` (NULL = the legacy default stream) and NOT synchronised
 *     before returning, except where stated
 */
#ifndef AMUSE_HIP_H
#define AMUSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Switches.  Kernel choices are API, not environment: amuse_set_decode_path / amuse_set_clips_per_group pin them per context, amuse_plan states the library's own rule.
 * The library reads NO environment variable.  What is left in the whole package (INTEGRATION.md has the same table):
 *   build macro  AMUSE_OP_F16          the declared second compilation of the three 16-bit kernels for fp16 operands (csrc/k_sampler8h.hip, k_vae_fusedh.hip, k_den_fusedh.hip)
 *   build macro  AMUSE_FPROF=1         variant builds only (tools/build_variant.sh): s_memtime phase stamps of the fused per-clip kernels
 *   environment  AMUSE_HIP_LIB         amuse_amd/_lib.py: load another build of this ABI (kernel A/B measurements)
 *   environment  AMUSE_SHARE_GPU=1     amuse_amd/main.py: every --gpus rank stays on --device (two-process tests on a one-GPU box)
 *   environment  AMUSE_BENCH_SHARE_GPU=1   bench.py: --gpus N ranks on one GPU over gloo (the two-rank bench tests on a one-GPU box)
 *   environment  AMUSE_RUN_STAMP, AMUSE_MANIFEST_DIR   launcher -> rank hand-over inside amuse_amd/main.py (not set by users)
 *   environment  AMUSE_TRAIN_FUSED=0, AMUSE_TRAIN_VALIDATE=1   train_gesture: eager layers / torch's distribution checks (amuse_amd/train_ops.py)
 *   environment  AMUSE_TRAIN_INNER=eval|train|train-hip|train-hip-decode   train_gesture's in-loop sampler: the persistent kernel in eval mode (default) / the
 *                                      reference's train-mode module loop / the persistent kernel with the dropouts live (amuse_set_sample_dropout) + the train-mode
 *                                      decode on the trainer's torch modules / the same sampler + the train-mode decode in the HIP decode kernels (amuse_set_decode_dropout)
 * The ~30 environment switches and 51 -DAMUSE_* macros of rounds 1-5 (A/B residue) were retired in round 6: tools/probes/retired_switches/. */
#define AMUSE_ABI_VERSION 5   /* 5: amuse_plan / amuse_debug_last_plan (the launch plan); the process-wide environment overrides of kernel choices are gone;
                                 4: amuse_train_* (training-step glue kernels);
                                 3: Denoiser variants (amuse_create_arch, AMUSE_ARCH_*, amuse_denoise_step_pose, amuse_feats_to_smplx);
                                 2: AMUSE_PREC_F32X / _F16, AMUSE_UPD_F32X / _F16; tile-major amuse_debug_gemm; clips per group 1..5 */

/* architecture the kernels are specialised for (configs/diff_latent_v2.json:23-47,
 * configs/prior_emotional_fing.json:6-20, configs/base_new.json "train_pose_framelen") */
#define AMUSE_D_MODEL 128
#define AMUSE_N_HEADS 4
#define AMUSE_FF 512
#define AMUSE_N_LAYERS 9
#define AMUSE_COND_DIM 256
#define AMUSE_N_FRAMES 300
#define AMUSE_N_JOINTS 55
#define AMUSE_N_FEATS 333
#define AMUSE_DENOISER_PARAMS 2192384u /* 130 tensors, state-dict order of Denoiser (denoiser.py:16-133) */
#define AMUSE_PRIOR_PARAMS 4643277u    /* 297 tensors, state-dict order of MotionPrior (vae.py:24-146) */
#define AMUSE_MAX_STEPS 1000

/* Denoiser variants (models/latent_diffusion/denoiser.py:64-66,92-131,174-204): `arch` and `diffusion_only` of
 * configs/diff_latent_v2.json "arch_denoiser".
 *   ENC       arch "trans_enc", latent sample: the shipped configuration - 5 tokens [latent, time, con, emo, sty], skip encoder
 *   DEC       arch "trans_dec", latent sample: tgt = the latent as ONE token (+ query_pos), memory = [time, con, emo, sty]
 *             (+ mem_pos); 9 TransformerDecoderLayer.forward_post (cross_attention.py:323-345: self-attention, cross-attention
 *             onto the 2..4 memory tokens, FFN) + decoder.norm
 *   ENC_POSE  diffusion_only + "trans_enc": the sample is the 300 x 333 pose sequence; [time, con, emo, sty | pose_embd(frames)]
 *             = S = 304 tokens through the skip encoder (NO key mask, denoiser.py:182), pose_proj of the frame rows
 *   DEC_POSE  diffusion_only + "trans_dec": tgt = pose_embd(frames) (S = 300), memory as DEC, pose_proj
 * The per-clip state of the sampling loop is AMUSE_D_MODEL floats for the latent variants and AMUSE_POSE_STATE = 300 * 333 for
 * the pose-space ones (amuse_state_dim); every `x` / `eps` / noise array below is [B][state_dim]. */
enum { AMUSE_ARCH_ENC = 0, AMUSE_ARCH_DEC = 1, AMUSE_ARCH_ENC_POSE = 2, AMUSE_ARCH_DEC_POSE = 3 };
#define AMUSE_POSE_STATE (AMUSE_N_FRAMES * AMUSE_N_FEATS)
#define AMUSE_DENOISER_PARAMS_DEC 2657536u        /* 176 tensors */
#define AMUSE_DENOISER_PARAMS_ENC_POSE 2278093u   /* 134 tensors: pose_embd, pose_proj first (denoiser.py:64-66) */
#define AMUSE_DENOISER_PARAMS_DEC_POSE 2743245u   /* 180 tensors */

enum { AMUSE_OK = 0, AMUSE_EINVAL = -1, AMUSE_EHIP = -2, AMUSE_ENOMEM = -3, AMUSE_ESTATE = -4 };

/* arithmetic of the MFMA GEMMs.  F32: fp32 weights/operands (v_mfma_f32_16x16x4_f32, exact fp32
 * FMA chains) - the parity mode.  BF16: bf16 weights + bf16-rounded operands, fp32 accumulate,
 * fp32 residual stream / LayerNorm / softmax / scheduler state - the throughput mode.
 * F32X: the fast parity mode of the sampling loop - every GEMM operand (weights on the host, activations in registers)
 * is split into two fp16 pieces, x = hi + lo (22 significand bits), and a product is three v_mfma_f32_16x16x32_f16
 * (Wh.xh + Wh.xl + Wl.xh) accumulated in fp32; softmax, LayerNorm, erf GELU and the scheduler update are the F32 code.
 * Holds the F32 mode's parity bars (eps_hat <= 1e-5 against the reference's modules) at a fraction of its step time.
 * Range: GEMM operands pass through fp16, so activations and weights must stay below 65504 in magnitude (beyond that the hi
 * piece is infinite) - three orders of magnitude above what this network carries (LayerNorm'd rows, |weights| < 1, latents up to
 * ~150 under DDPM); small values lose nothing: lo pieces below 2^-14 are fp16 subnormals, which the MI355X MFMA keeps.
 * amuse_vae_decode / amuse_vae_encode run the same split arithmetic in their staged kernels (k_vae.hip PREC_F16X2).
 * F16: the throughput mode on fp16 instead of bf16 operands - the BF16 mode's kernels (8-wave sampler, fused decoder) built for
 * v_mfma_f32_16x16x32_f16 / v_cvt_pk_f16_f32: same speed, same bytes, 11 significand bits instead of 8 - about an eighth of the BF16
 * mode's drift against F32.  Range as for F32X.  amuse_vae_decode / amuse_vae_encode: the BF16 mode's kernels
 * (fused per-clip decoder, staged rows / attention kernels) in their fp16 instantiations, chosen by the same rule. */
enum { AMUSE_PREC_F32 = 0, AMUSE_PREC_BF16 = 1, AMUSE_PREC_F32X = 2, AMUSE_PREC_F16 = 3 };

/* matrix -> quaternion convention of the axis-angle epilogue (infer_ldm.py:172):
 * P3D   = pytorch3d >= 0.5 candidate selection, no sign standardisation (what the reference's
 *         committed outputs show: |axis-angle| up to 4.69 > pi);
 * LEGACY = the snapshot vendored at models/diffusion/utils/rotation_conversions.py:97-119 (q_w >= 0). */
enum { AMUSE_QUAT_P3D = 0, AMUSE_QUAT_LEGACY = 1 };

typedef struct amuse_ctx amuse_ctx;

/* One denoising schedule = what diffusers' scheduler.set_timesteps + scheduler.step need
 * (infer_ldm.py:116-125,142-147,160-161).  Per step i the update applied in-kernel is
 *   x0 = (x - sb*eps) / sa ; if (clip > 0) x0 = clamp(x0, -clip, clip)
 *   x' = c0*x0 (+ cx*x) (+ ce*eps) (+ sigma*z)
 * coef[i] = { sb, sa, c0, cx, ce, sigma, clip, 0 }.  DDIM: cx = 0; DDPM: ce = 0.  Terms whose
 * coefficient is exactly 0 are skipped.  amuse_amd/scheduler.py builds these tables. */
typedef struct {
    int n_steps;            /* T, 1..AMUSE_MAX_STEPS */
    const int* timesteps;   /* host [T]: the integer timestep fed to the time embedding at step i */
    const float* coef;      /* host [T][8] */
    const float* freqs;     /* host [128] or NULL: exp(-ln(1e4) k/128), k = 0..127 (embeddings.py:262-267).
                               The reference evaluates this with torch.exp; a caller that wants bit-equal
                               time embeddings passes torch's values, NULL = libm expf. */
} amuse_schedule;

/* Replaces PretrainedLPDM_v1.setup()'s model construction + weight load (infer_ldm.py:66-109) and
 * PretrainedVAE.load_model (infer_pretrained_vae.py:13-49).  `denoiser_params` / `prior_params`
 * are HOST fp32 arrays holding every state-dict tensor, concatenated in state-dict order (sizes
 * must equal AMUSE_DENOISER_PARAMS / AMUSE_PRIOR_PARAMS).  Packs both precisions' MFMA-fragment
 * weight streams and uploads them.  Returns NULL on failure. */
amuse_ctx* amuse_create(int device, const float* denoiser_params, size_t n_denoiser,
                        const float* prior_params, size_t n_prior);
/* The same for a Denoiser variant: `denoiser_params` holds the state dict of Denoiser(arch, diffusion_only) in its own
 * registration order (amuse_denoiser_param_count(arch) floats; amuse_amd/weights.py denoiser_param_spec lists the keys).
 * prior_params may be NULL (n_prior 0) for the pose-space variants, which never decode (infer_ldm.py:165,177);
 * amuse_vae_* then fail with AMUSE_ESTATE.  arch AMUSE_ARCH_ENC == amuse_create. */
amuse_ctx* amuse_create_arch(int device, int arch, const float* denoiser_params, size_t n_denoiser,
                             const float* prior_params, size_t n_prior);
size_t amuse_denoiser_param_count(int arch);   /* 0 for an unknown arch */
int amuse_arch(const amuse_ctx* ctx);
size_t amuse_state_dim(const amuse_ctx* ctx);  /* floats per clip of the sampled state: 128 or AMUSE_POSE_STATE */
/* New weights into an existing context (same architecture): re-packs and overwrites the weight streams in place.
 * Replaces what the reference gets for free from sharing nn.Module parameters between its training step and the
 * in-loop sampler (scripts/trainer.py:411-415: ldm.diffusion_backward + prior.decode on the weights just stepped).
 * Either array may be NULL (left as is).  `what` limits the host-side packing to what the caller will run:
 * AMUSE_UPD_F32 | AMUSE_UPD_BF16 | AMUSE_UPD_F32X | AMUSE_UPD_F16 = the weight streams of that precision, AMUSE_UPD_ENCODER =
 * MotionPrior.encode's streams too.  Small parameters (biases, LayerNorm, embeddings) are always replaced, so after a partial update only the
 * re-packed precision is valid - running the other one mixes old matrices with new vectors.  Synchronises `stream` first; after a denoiser update the
 * schedule must be set again (the time-token table is a function of the time-embedding weights). */
enum { AMUSE_UPD_F32 = 1, AMUSE_UPD_BF16 = 2, AMUSE_UPD_ENCODER = 4, AMUSE_UPD_F32X = 8, AMUSE_UPD_F16 = 16, AMUSE_UPD_ALL = 31 };
int amuse_update_weights(amuse_ctx* ctx, const float* denoiser_params, size_t n_denoiser, const float* prior_params,
                         size_t n_prior, int what, void* stream);
/* The same from DEVICE arrays (fp32, state-dict order, as above), stream-ordered on `stream` with no host round trip: every packed
 * image is a gather of the parameters, so a kernel re-packs (and rounds to bf16) in place.  The gather maps are built on the first
 * call.  This is what train_gesture's in-loop sampler uses every iteration (amuse_amd/train_gesture.py): the host path costs
 * 24-26 ms per call.  Results are bitwise those of amuse_update_weights on the same values; the schedule stays set (its time-token
 * table is rebuilt on the stream). */
int amuse_update_weights_device(amuse_ctx* ctx, const float* denoiser_params_dev, const float* prior_params_dev, int what,
                                void* stream);
void amuse_destroy(amuse_ctx* ctx);
const char* amuse_last_error(void);
int amuse_abi_version(void);

/* Replaces diffusers.DDIMScheduler(...).set_timesteps(N) (infer_ldm.py:116-123,143-144) and hoists
 * Timesteps + TimestepEmbedding (embeddings.py:245-322; denoiser.py:146-149) out of the loop: builds
 * the [T,128] time-token table on the GPU.  Synchronises `stream`. */
int amuse_set_schedule(amuse_ctx* ctx, const amuse_schedule* sched, void* stream);

/* Replaces the timestep loop of PretrainedLPDM_v1.diffusion_backward (infer_ldm.py:137-161):
 * initial noise, T x { Denoiser.forward, scheduler.step }.
 *   con/emo/sty  dev [B][256]; emo and/or sty may be NULL (token dropped, denoiser.py:159-171)
 *   x_init       dev [B][128] or NULL -> counter-based N(0,1) from (seed, clip_index0 + b)
 *   step_noise   dev [T][B][128] or NULL -> counter-based; only read at steps with sigma != 0
 *   latents_out  dev [B][128]  final latents
 *   traj_out     dev [T][B][128] or NULL: latent after every step (tests)
 * Uses the schedule set by amuse_set_schedule.  Denoiser variants (amuse_create_arch): 128 reads amuse_state_dim(ctx) in every
 * shape above - the pose-space variants sample the [300][333] feature sequence itself, lengths all 300 as the reference's
 * loop passes them (infer_ldm.py:135). */
int amuse_sample(amuse_ctx* ctx, const float* con, const float* emo, const float* sty, int B,
                 int precision, uint64_t seed, uint64_t clip_index0, const float* x_init,
                 const float* step_noise, float* latents_out, float* traj_out, void* stream);

/* Replaces one Denoiser.forward call (denoiser.py:135-204) - teacher-forced single step for tests:
 * eps_out[B][128] = eps_hat(x_t, timestep, con, emo, sty).  Does not need a schedule.
 * tap_out (dev, nullable, [11][16][128]): token rows of the first clip tile after token assembly
 * (slot 0), after each of the 9 blocks (slots 1..9) and after the final LayerNorm (slot 10). */
int amuse_denoise_step(amuse_ctx* ctx, const float* x_t, int timestep, const float* con,
                       const float* emo, const float* sty, int B, int precision, float* eps_out,
                       float* tap_out, void* stream);

/* The pose-space variants' teacher-forced step with the `lengths` argument of Denoiser.forward (denoiser.py:135-145,187,199):
 * eps rows of frames >= lengths[b] are zeroed (`sample[~mask.T] = 0`); the padded frames are still attended (the reference
 * passes no key mask).  lengths host [B] or NULL (= all 300).  x_t, eps_out dev [B][300][333]. */
int amuse_denoise_step_pose(amuse_ctx* ctx, const float* x_t, int timestep, const float* con, const float* emo,
                            const float* sty, const int* lengths, int B, int precision, float* eps_out, void* stream);

/* Replaces the arithmetic of LatentDiffusionModel.diffusion_forward (models/latent_diffusion/ldm.py:71-97), the
 * training-time twin of the sampling step, in eval semantics (no dropout): noisy = sqrt_ab * z0 + sqrt_1m_ab * noise
 * (DDPMScheduler.add_noise) and noise_pred = Denoiser(noisy, timesteps, cond) with ONE TIMESTEP PER CLIP.
 *   z0, noise              dev [B][128]
 *   timesteps              host [B]   (torch.randint(0, num_train_timesteps, (bsz,)) in the reference)
 *   sqrt_ab, sqrt_1m_ab    host [B]   sqrt(alphas_cumprod[t_b]), sqrt(1 - alphas_cumprod[t_b])
 *   noisy_out (nullable), noise_pred_out   dev [B][128] */
int amuse_diffusion_forward(amuse_ctx* ctx, const float* z0, const float* noise, const int* timesteps,
                            const float* sqrt_ab, const float* sqrt_1m_ab, const float* con,
                            const float* emo, const float* sty, int B, int precision, float* noisy_out,
                            float* noise_pred_out, void* stream);

/* Replaces PretrainedVAE.get_motion -> MotionPrior.decode (infer_pretrained_vae.py:58-62,
 * vae.py:216-278) plus the 6D -> matrix -> axis-angle conversion (infer_ldm.py:168-173).
 *   z          dev [B][128]
 *   lengths    host [B] or NULL (= all 300): frames >= length are masked as keys and zeroed
 *   feats_out  dev [B][300][333] or NULL (the raw decoder features)
 *   poses_out  dev [B][300][55][3], trans_out dev [B][300][3] (either may be NULL) */
int amuse_vae_decode(amuse_ctx* ctx, const float* z, const int* lengths, int B, int precision,
                     int quat_mode, float* feats_out, float* poses_out, float* trans_out,
                     void* stream);

/* Replaces PretrainedVAE.get_latent -> MotionPrior.encode (infer_pretrained_vae.py:51-56,
 * vae.py:154-214; call site infer_ldm.py:465): features -> skel_embedding, two distribution tokens
 * prepended, learned PE, 9-block skip-transformer encoder with key-padding mask; mu / logvar are the
 * two distribution rows, std = exp(logvar) ** 0.5, latent = mu + std * eps (Normal.rsample).
 *   feats      dev [B][300][333] motion features (6D rotations | translation)
 *   lengths    host [B] or NULL (= all 300): frames >= length are masked as attention keys
 *   eps        dev [B][128] standard-normal draw for rsample, or NULL (latent_out = mu)
 *   mu_out, std_out, latent_out   dev [B][128], each nullable (at least one required) */
int amuse_vae_encode(amuse_ctx* ctx, const float* feats, const int* lengths, int B, int precision,
                     const float* eps, float* mu_out, float* std_out, float* latent_out,
                     void* stream);

/* Replaces the motion preparation of PretrainedLPDM_v1._loader_helper_v1 (infer_ldm.py:459-464):
 * SMPL-X axis-angle -> rotation matrix -> 6D (first two rows), concatenated with the translation.
 *   poses dev [B][300][55][3], trans dev [B][300][3]  ->  feats_out dev [B][300][333] */
int amuse_smplx_to_feats(amuse_ctx* ctx, const float* poses, const float* trans, int B,
                         float* feats_out, void* stream);

/* Replaces PretrainedLPDM_v1.diffusion_backward end to end (infer_ldm.py:130-178):
 * amuse_sample followed by amuse_vae_decode on the final latents. */
int amuse_diffusion_backward(amuse_ctx* ctx, const float* con, const float* emo, const float* sty,
                             int B, int precision, int quat_mode, uint64_t seed,
                             uint64_t clip_index0, const float* x_init, const float* step_noise,
                             float* latents_out, float* poses_out, float* trans_out, void* stream);

/* The output conversion of PretrainedLPDM_v1.diffusion_backward alone (infer_ldm.py:168-173): features (6D rotations |
 * translation) -> SMPL-X axis-angle.  feats dev [B][300][333] -> poses_out dev [B][300][55][3], trans_out dev [B][300][3].
 * amuse_diffusion_backward of a pose-space variant = amuse_sample + this (the sampled state IS the feature sequence; the
 * reference itself raises at infer_ldm.py:177 where its decode-free branch would be). */
int amuse_feats_to_smplx(amuse_ctx* ctx, const float* feats, int B, int quat_mode, float* poses_out, float* trans_out,
                         void* stream);

/* The build's counter-based normal generator, exposed for tests: out[B][state_dim] for clips
 * clip_index0..+B, `step`, stream 0 (initial latent) or 1 (ancestral noise).  Element e of a clip's state is draw e % 4 of
 * Philox counter (clip, step, e / 4, stream). */
int amuse_counter_normal(amuse_ctx* ctx, uint64_t seed, uint64_t clip_index0, int B, int step,
                         int rng_stream, float* out, void* stream);

/* Diagnostics: runs amuse_sample's kernel with s_memtime stamps taken by the waves of workgroup 0
 * during step `prof_step`; stamps_out dev 768 x uint64 (unused entries 0).
 *   fp32 (4-wave kernel): [4 waves][192] - step start, then per
 *     block: block start, in_proj, attention, out_proj, combine 1, LN1, four FFN quarters, combine 2,
 *     LN2; finally scheduler update.
 *   bf16 (8-wave kernel): [8 waves][96] - step start, then per block: block start (after the skip linear),
 *     attention phase, out_proj combine, FFN, linear2 combine; finally scheduler update.
 * Used by tools/gpu_phase_profile*.py to build profiles/. */
int amuse_profile_sample(amuse_ctx* ctx, const float* con, const float* emo, const float* sty, int B,
                         int precision, int prof_step, unsigned long long* stamps_out, void* stream);

/* Clips per workgroup tile in the sampling kernels: 0 = auto (amuse_plan's clips_per_group for the CALL's clip count), else 1..5; the value used is
 * clamped to 16 / S (S = 5, 4 or 3 tokens per clip: at most 3, 4 or 5 clips share the 16 rows of a tile).
 * Results are bitwise reproducible across launches / shards that use the same value and start at multiples of it
 * (a clip's slot inside its tile decides the rounding of its attention sums); amuse_amd/shard.py applies that rule. */
int amuse_set_clips_per_group(amuse_ctx* ctx, int g);

/* Train-mode sampling: the Denoiser's encoder dropouts live in amuse_sample, amuse_denoise_step, amuse_profile_sample and the sampling half of
 * amuse_diffusion_backward (AMUSE_ARCH_ENC; AMUSE_PREC_F32 / _BF16 / _F16), as in the reference's training loop, which samples with the networks in
 * train() mode (scripts/trainer.py).  p = 0 (the default) = eval mode, the kernels of before.  p NaN, < 0 or >= 1: AMUSE_EINVAL.  With p > 0 a sample or
 * step call in AMUSE_PREC_F32X or on another arch returns AMUSE_ESTATE and launches nothing.  The decode has a switch of its own
 * (amuse_set_decode_dropout below); encode and amuse_diffusion_forward stay in eval semantics.
 * Mask contract (tests/test_gpu_sample_dropout.py restates it).  Dropout sites of encoder layer l = 0..8 in execution order (input blocks 0-3, middle,
 * output blocks 0-3), as TransformerEncoderLayer.forward_post (utils/cross_attention.py):
 *   site s = 0  softmax probabilities before . V        element e = (h S + q) S + k   (h = head 0..3, q / k = query / key token, S = 3..5 tokens)
 *   site s = 1  dropout1 on out_proj's output (+ bias)  e = tok 128 + f
 *   site s = 2  the FFN's dropout(gelu(linear1))        e = tok 512 + f
 *   site s = 3  dropout2 on linear2's output (+ bias)   e = tok 128 + f
 * None on the positional encoding, the time / condition projections, the skip linears or the final LayerNorm (the reference has none there).
 * Element e uses draw e % 4 of Philox4x32-10 with key = seed (lo, hi) and counter = (clip, step, ((l 4 + s) << 16) | (e / 4), 2 + epoch): clip = the
 * global clip index (clip_index0 + b; b for amuse_denoise_step), step = the loop index i (0 for amuse_denoise_step), epoch = the training dropout
 * epoch word (amuse_train_epoch_advance / _set: a captured step draws fresh masks per replay).  Word 3 starts at 2: no collision with the noise
 * streams 0 and 1.  Keep <=> (draw >> 8) >= thr, thr = (uint32)(p 2^24); kept values are multiplied by 1 / (1 - p) (the amuse_train_* convention). */
int amuse_set_sample_dropout(amuse_ctx* ctx, float p, uint64_t seed);

/* Train-mode decode: the dropouts of MotionPrior.decode live in amuse_vae_decode and in the decode half of amuse_diffusion_backward, as in the reference's
 * training loop, which decodes its in-loop samples with the prior in train() mode (scripts/trainer.py).  A switch of its own: amuse_set_sample_dropout is not
 * touched by it, nor are amuse_vae_encode, amuse_diffusion_forward, amuse_denoise_step*, amuse_sample.  p = 0 (the default) = eval mode, the kernels and the plan
 * of before.  p NaN, < 0 or >= 1, or a NULL ctx: AMUSE_EINVAL.  With p > 0:
 *   - AMUSE_PREC_F32, _BF16, _F16: the decode runs on the staged kernel family (csrc/k_vae.hip; STAGED below) at every clip count, whatever amuse_set_decode_path
 *     says, and amuse_debug_last_plan reports AMUSE_DECODE_STAGED; the fused per-clip kernels stay eval-only.  A clip's result does not depend on the batch it is in.
 *   - AMUSE_PREC_F32X, or a context without a prior: AMUSE_ESTATE, nothing launched (amuse_diffusion_backward: not even the sampler).
 * Clip b of an amuse_vae_decode call has global clip index clip_index0 + b with THIS function's clip_index0; inside amuse_diffusion_backward that call's own
 * clip_index0 argument is used instead, so the decode's masks follow the sampler's clips.  The index is truncated to 32 bits, as in the sampler.
 * Mask contract (tests/test_decode_dropout_cpu.py restates it; tests/golden/decode_dropout.npz holds the reference module's output under these masks).
 * TransformerDecoderLayer.forward_post (utils/cross_attention.py) has six dropout sites (torch's nn.MultiheadAttention drops its softmax probabilities); layer
 * l = 0..8 in execution order (input blocks 0-3, middle, output blocks 0-3), S = 300 rows whatever the clip's length, h = head 0..3, q / k = query / key frame:
 *   site s = 0  self-attention probabilities before . V           element e = (h S + q) S + k   (after the softmax has normalised: the row sum is the unmasked one)
 *   site s = 1  dropout1 on the self-attention out_proj (+ bias)  e = q 128 + f
 *   site s = 2  cross-attention probabilities onto the ONE memory token (softmax over one key = 1, so 0 or 1 / (1 - p) per head and query)   e = h S + q
 *   site s = 3  dropout2 on the cross-attention out_proj (+ bias) e = q 128 + f
 *   site s = 4  the FFN's dropout(gelu(linear1))                  e = q 512 + f
 *   site s = 5  dropout3 on linear2 (+ bias)                      e = q 128 + f
 * None on the positional encoding, the skip linears, decoder.norm or final_layer (the reference has none there).
 * Element e uses draw e % 4 of Philox4x32-10 with key = seed (lo, hi) and counter = (clip, 0x80000000 | (8 l + s), e / 4, 2 + epoch): epoch = the training
 * dropout epoch word (amuse_train_epoch_advance / _set: a captured decode draws fresh masks per replay).  Bit 31 of word 1 keeps these streams clear of the
 * sampler's under an equal seed (there word 1 is the step, at most AMUSE_MAX_STEPS); word 3 starts at 2: no collision with the noise streams 0 and 1.
 * Keep <=> (draw >> 8) >= thr, thr = (uint32)(p 2^24); kept values are multiplied by 1 / (1 - p) in fp32 (the amuse_train_* convention). */
int amuse_set_decode_dropout(amuse_ctx* ctx, float p, uint64_t seed, uint64_t clip_index0);

/* Which kernels amuse_vae_decode (and amuse_diffusion_backward), amuse_vae_encode and the pose-space Denoiser's step use.  Every mode but fp32 has more
 * than one kernel family for MotionPrior.decode (vae.py:216-278); they compute the same function and differ in summation order only (fp32x: 1.5e-6 on
 * features of magnitude 3):
 *   STAGED  the row / attention launches of csrc/k_vae.hip (one 16-row tile per workgroup, split-K); the only family of the fp32 mode.
 *   FUSED   bf16 / fp16: the fused per-clip kernel (csrc/k_vae_fused.hip: one persistent workgroup per clip, residual stream in registers, K/V of the
 *           current head in LDS); fp32x: the row kernel without split-K (csrc/k_vae_rows8.hip: a tile per wave, weights through LDS once per workgroup).
 *   CLIP    fp32x: one persistent workgroup per clip in the parity arithmetic (csrc/k_vae_fusedx.hip: q / k / v never leave the CU); FUSED elsewhere.
 *   AUTO    what amuse_plan returns for the CALL's clip count: FUSED from 64 clips, in fp32x CLIP where the clips fill rounds of the chip's 256 CUs.
 * A sharded job pins the WHOLE job's choice (amuse_plan on the job's total) on every shard, so shards reproduce the single-GPU bits. */
enum { AMUSE_DECODE_AUTO = 0, AMUSE_DECODE_STAGED = 1, AMUSE_DECODE_FUSED = 2, AMUSE_DECODE_CLIP = 3 };
int amuse_set_decode_path(amuse_ctx* ctx, int path);

/* The launch plan of a JOB - the single statement of the library's kernel-choice rules (csrc/amuse_host.hpp plan_*); needs no GPU and no context.
 * For a job of clips_total clips of `tokens` tokens each (5 = latent + time + content + emotion + style; 4 / 3 with emotion / style dropped), Denoiser
 * variant `arch`, mode `precision`:
 *   *clips_per_group  clips per 16-row tile of the latent trans_enc sampler (1 for the other variants): what amuse_sample takes on AUTO for a call of
 *                     that many clips, and the alignment of shard starts (amuse_set_clips_per_group on every shard)
 *   *decode_path / *encode_path / *step_path   AMUSE_DECODE_STAGED / _FUSED / _CLIP: what amuse_vae_decode / amuse_vae_encode / one pose-space Denoiser
 *                     step take on AUTO for a call of that many clips (amuse_set_decode_path with the job's decode_path on every shard)
 * Any output pointer may be NULL.  amuse_debug_last_plan reports what the last amuse_sample / amuse_vae_decode / amuse_vae_encode / pose-space step of a
 * context ACTUALLY took (0 = none yet); tests/test_plan_cpu.py sweeps 1..8192 clips and holds the two equal. */
int amuse_plan(int arch, int precision, int clips_total, int tokens, int* clips_per_group, int* decode_path, int* encode_path, int* step_path);
int amuse_debug_last_plan(const amuse_ctx* ctx, int* clips_per_group, int* decode_path, int* encode_path, int* step_path);

/* ------------------------------------------------------------------------------------------------
 * Audio front-end: replaces PretrainedLPDM_v1.process_single_seq
 * (models/latent_diffusion/infer_ldm.py:180-193) = torchaudio.compliance.kaldi.fbank -> zero-pad / crop to 1024
 * frames -> (x - mean) / (2 std) -> Pretrained_AST_EVP.get_features (models/audio/infer_pretrained_ast_evp.py:42-46)
 * -> AST_EVP.eval_func (AST_EVP.py:84-90): three ASTModel encoders (audio_main_new.py:174-204), 'feature' of each.
 * bf16 GEMM / attention operands, fp32 accumulation and residual stream.
 *
 * Parameters: one flat fp32 array per encoder holding the forward-pass tensors of ASTModel in this order (timm 0.4.5
 * DistilledVisionTransformer names): v.cls_token, v.dist_token, v.pos_embed [1214][768], v.patch_embed.proj.weight
 * [768][1][16][16], .bias, then for blocks 0..11: norm1.weight, norm1.bias, attn.qkv.weight [2304][768], attn.qkv.bias,
 * attn.proj.weight, attn.proj.bias, norm2.weight, norm2.bias, mlp.fc1.weight [3072][768], mlp.fc1.bias,
 * mlp.fc2.weight [768][3072], mlp.fc2.bias; v.norm.weight, v.norm.bias, feature_head.0.weight, .bias,
 * feature_head.1.weight [256][768], .bias   (AMUSE_AST_PARAMS floats). */
typedef struct amuse_audio_ctx amuse_audio_ctx;
#define AMUSE_AST_PARAMS 86385664u
#define AMUSE_AUDIO_CON 0
#define AMUSE_AUDIO_EMO 1
#define AMUSE_AUDIO_STY 2
/* mel_banks host [128][257], window host [400] (kaldi fbank tables: amuse_amd/audio.py builds them);
 * norm_mean / norm_std = configs/base_new.json wav_dtw_mfcc.dataset_mean / dataset_std;
 * frame_based_feats = wav_dtw_mfcc.frame_based_feats (mean over patch tokens) or 0 ((cls + dist) / 2). */
amuse_audio_ctx* amuse_audio_create(int device, const float* con_params, const float* emo_params,
                                    const float* sty_params, size_t n_each, const float* mel_banks,
                                    const float* window, float norm_mean, float norm_std,
                                    int frame_based_feats);
void amuse_audio_destroy(amuse_audio_ctx* ctx);
/* waves dev [B][n_samples] fp32 (16 kHz mono)  ->  fbank_out dev [B][1024][128], normalised and padded */
int amuse_audio_fbank(amuse_audio_ctx* ctx, const float* waves, int n_samples, int B, float* fbank_out,
                      void* stream);
/* One encoder on prepared fbanks: feat_out dev [B][256]; hidden_out (nullable) dev [B][1214][768] receives the
 * fp32 residual stream after block `tap_block` (0..11) for tests. */
int amuse_audio_encode(amuse_audio_ctx* ctx, int which, const float* fbank, int B, float* feat_out,
                       float* hidden_out, int tap_block, void* stream);
/* process_single_seq for B waveforms: con_out / emo_out / sty_out dev [B][256] (each nullable).  Stream-ordered on
 * `stream`; the three encoders run concurrently (per chunk of 32 clips) on two context-owned side streams, forked from
 * and joined back into `stream` with events (results identical to amuse_audio_encode one encoder at a time). */
int amuse_audio_features(amuse_audio_ctx* ctx, const float* waves, int n_samples, int B, float* con_out,
                         float* emo_out, float* sty_out, void* stream);

/* The arithmetic of amuse_audio_encode (its hidden_out tap included) and amuse_audio_features; amuse_audio_fbank is fp32 in
 * either mode.  AMUSE_PREC_BF16 (the default): bf16 operands, fp32 accumulation - bit for bit what a context that never
 * left the mode computes, also after a round trip through AMUSE_PREC_F32X.  AMUSE_PREC_F32X, the parity mode - the contract:
 *   - every GEMM operand x is used as hi = rn16(x), lo = rn16(x - hi) in IEEE fp16, rn16 = round-to-nearest-even with
 *     gradual underflow (the bits of amuse_debug_f16_split and of v_cvt_pk_f16_f32): the weights, the im2col patches, the
 *     LayerNorm outputs, q (pre-scaled by head_dim ** -0.5 * log2 e before the split), k, v, the un-normalised softmax
 *     probabilities, the attention output and the GELU output.  A product is Wl.xh + Wh.xl + Wh.xh on
 *     v_mfma_f32_16x16x32_f16 with fp32 accumulation; the lo.lo term (2^-22 relative) is dropped;
 *   - everything else is fp32: the residual stream; LayerNorm (two passes; eps 1e-6 in the blocks and the final norm, 1e-5
 *     in the feature head); softmax in exp2 units with the running-maximum rule of the fp32x decode attention - a chunk
 *     of 64 keys moves a row's maximum only when a score exceeds it by more than 6 log2 units, so p never exceeds 2^6, and
 *     the division by the row sum removes the scale; the row sums of the split P (hi + lo, the values the P.V product
 *     uses); pooling;
 *   - GELU is the exact erf form (fp32 rounding class; the bf16 kernels' clamped polynomial is 1.9e-4 off);
 *   - the 768 -> 256 feature head runs on plain fp32 FMAs from fp32 weights, k ascending: its input is NOT split;
 *   - |x| >= 65504 saturates hi (>= 65520: infinity).  No operand of the shipped architecture gets there: LayerNorm
 *     outputs, the pre-scaled q, k and v of LayerNorm-ed rows, p <= 64, convex combinations of v, GELU of those;
 *   - a clip's bits do not depend on its batch position, on the 32-clip chunking or on the call (encode / features).
 * The mode's weight images (4 B per parameter: 345 MB per encoder) are built on the FIRST switch to AMUSE_PREC_F32X from a
 * host copy of the parameters that amuse_audio_create keeps until then, its activation workspace (two fp16 planes per
 * operand matrix, 39 MB per clip and encoder) grows with the calls as the bf16 one does; amuse_audio_destroy frees both.
 * amuse_audio_create uploads what it always did.  Not stream-ordered: call it between, not during, the context's calls.
 * Returns AMUSE_EINVAL for a NULL ctx or any other precision, AMUSE_ESTATE (and changes nothing) from a build of the
 * library without the mode's translation unit (amuse_audio_x.hip); amuse_audio_precision returns the mode. */
int amuse_audio_set_precision(amuse_audio_ctx* ctx, int precision);
int amuse_audio_precision(const amuse_audio_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * Audio model metrics: the tail of AST_EVP behind the three encoders, as PretrainedLPDM_v1.collect_audio_metrics reaches it
 * (models/latent_diffusion/infer_ldm.py:195-208 -> Pretrained_AST_EVP.get_reconstructed_fbank -> AST_EVP.eval_func(metrics=True),
 * models/audio/AST_EVP.py:84-103): the classifier heads of emo_enc / sty_enc (audio_main_new.py:76-81,191-204), FusionBlock and
 * DecoderBlock (AST_EVP.py:12-42,63-82).  The two-encoder ablations (fusion_ablation / reconstruct_ablation) are not built.
 *
 * Parameters: ONE flat fp32 array of AMUSE_AST_TAIL_PARAMS floats, AST_EVP's state-dict entries in this order (amuse_amd/audio_weights.py
 * ast_tail_param_spec is the authority): for enc in (emo_enc, sty_enc), L = 8 / 30: mlp_head.0.weight [256], .bias, mlp_head.1.weight [L][256], .bias,
 * mlp_head_featbased.0.weight [768], .bias, mlp_head_featbased.1.weight [L][768], .bias; fusion.layers.{0,1} (d = 768), fusion.norm.weight, .bias,
 * fusion.fc.weight [512][768], .bias; decode.layers.{0..3} (d = 512), decode.norm.weight, .bias, decode.projection.0.weight [1024][512], .bias,
 * decode.projection.2.weight [131072][1024], .bias.  A layer is nn.TransformerEncoderLayer(d, nhead=4) in torch's order: self_attn.in_proj_weight [3d][d],
 * self_attn.in_proj_bias, self_attn.out_proj.weight [d][d], .bias, linear1.weight [2048][d], .bias, linear2.weight [d][2048], .bias, norm1.weight, .bias,
 * norm2.weight, .bias (post-norm, ReLU, eps 1e-5, dropout inactive).
 *
 * Arithmetic.  Heads, fusion, decoder layers and the 512 -> 1024 projection are fp32 in BOTH precisions of the context: fp32 weights, FMAs with fp32
 * accumulation, two-pass LayerNorm, q scaled by head_dim ** -0.5, softmax over the at most 16 keys of a group.  The 1024 -> 131072 projection follows
 * amuse_audio_set_precision: AMUSE_PREC_BF16 - weights and activations rounded to bf16 (nearest even), fp32 accumulation on v_mfma_f32_16x16x32_bf16, fp32
 * bias; AMUSE_PREC_F32X - the contract of the encoders' parity mode: hi = rn16(x), lo = rn16(x - hi) of weights and activations, a product is
 * Wl.xh + Wh.xl + Wh.xh on v_mfma_f32_16x16x32_f16, lo.lo dropped; that mode's weight image (537 MB; the bf16 one is 268 MB) is built on the first
 * reconstruct in the mode from a host copy kept until then.  bf16 results are bit for bit unchanged by a round trip through AMUSE_PREC_F32X.
 *
 * amuse_audio_set_tail uploads the parameters (host memory; again replaces them).  Not stream-ordered.  The tail has ONE workspace: its calls on one
 * context must not overlap on different streams. */
#define AMUSE_AST_TAIL_PARAMS 158950988u
int amuse_audio_set_tail(amuse_audio_ctx* ctx, const float* tail_params, size_t n);
/* amuse_audio_encode with the pooling chosen per call (frame_based 1: mean over the patch tokens, 0: (cls + dist) / 2, < 0: the context's - feat_out is then
 * bit for bit what amuse_audio_encode writes), plus the encoder's classifier head: logits_out dev [B][8] (AMUSE_AUDIO_EMO) / [B][30] (AMUSE_AUDIO_STY),
 * nullable.  Frame-based: mlp_head_featbased((cls + dist) / 2 of the final norm) - a second pooling launch over the same residual stream; otherwise
 * mlp_head(features).  Returns AMUSE_EINVAL for a non-NULL logits_out with AMUSE_AUDIO_CON (label_dim 0: the reference's predicted_labels is None),
 * AMUSE_ESTATE when logits are asked for and no tail is set or the build lacks the tail's translation unit (amuse_audio_tail.hip); nothing is launched then. */
int amuse_audio_encode_labels(amuse_audio_ctx* ctx, int which, int frame_based, const float* fbank, int B, float* feat_out, float* logits_out, void* stream);
/* AST_EVP.reconstruct(cat(emo, sty, con), reconstruct_only=True): con / emo / sty dev [B][256] -> fbank_out dev [B][1024][128] (output f = 128 h + w).
 * The reference hands the layers a 2-D tensor, which torch treats as ONE sequence whose tokens are the batch rows: the rows of a call attend to each other.
 * `group` = S in 1..16 with B % S == 0 restates that: consecutive runs of S rows form one sequence (S = B: the reference's batch; S = 1: the single clip of
 * collect_audio_metrics, softmax exactly 1).  A row's bits depend on its group's contents and its position inside the group and on nothing else (not on
 * B, the group's index or the 32-row chunking).  AMUSE_EINVAL for a bad B / group or NULL, AMUSE_ESTATE without a tail (as above); nothing is launched then. */
int amuse_audio_reconstruct(amuse_audio_ctx* ctx, const float* con, const float* emo, const float* sty, int B, int group, float* fbank_out, void* stream);
/* The same up to the last Linear's input, for tests: hidden_out dev [B][1024] = ReLU(decode.projection.0(...)), fp32. */
int amuse_debug_tail_hidden(amuse_audio_ctx* ctx, const float* con, const float* emo, const float* sty, int B, int group, float* hidden_out, void* stream);

/* The last Linear's kernel in isolation (csrc/k_audio_tail.hip), for tests and tools/gpu_audio_tail_cost.py: out[B][N] = A[B][K] . W[N][K]^T + bias, A / bias /
 * out dev fp32 row-major, B >= 1 (passes of 32 rows), N % 256 == 0, K % 64 == 0, 64 <= K <= 1024, precision AMUSE_PREC_BF16 or AMUSE_PREC_F32X.
 * W_packed (dev) is the kernel's own weight order, written by amuse_debug_tail_pack (host memory, no GPU call): 1 KiB units of [64 lanes][8 x 16 bit] = 16
 * features x 32 k, lane (g, i) = W[16 t + i][32 s + 8 g .. + 7]; the units of feature tile t are consecutive (s ascending), tiles ascending.  As an index
 * into 16-bit elements:
 *     bf16:  ((f >> 4) * (K >> 5) + (k >> 5)) * 512 + ((((k & 31) >> 3) << 4) + (f & 15)) * 8 + (k & 7)              holds bf16(W[f][k]), N * K elements
 *     fp32x: ((f >> 4) * (K >> 5) + (k >> 5)) * 1024 + plane * 512 + (the same lane / element term)                   plane 0 = hi, 1 = lo (amuse_debug_f16_split), 2 * N * K
 * A wave reads a contiguous run of tiles, i.e. one contiguous byte range. */
int amuse_debug_tail_pack(const float* W, int N, int K, int precision, void* out);
int amuse_debug_tail_gemm(const float* A, const void* W_packed, const float* bias, int B, int N, int K, int precision, float* out, void* stream);

/* The front-end's GEMM kernel in isolation, for tests and tools/gpu_gemm_bench.py: out = A . W^T + bias.
 * The front-end keeps every GEMM operand TILE-MAJOR in HBM (16-row x 32-feature tiles of 64 lanes x 8 elements, a bf16
 * tile being one MFMA fragment; amuse_amd/csrc/amuse_audio.hpp): A dev bf16 tile-major [M rounded up to 128][K], W dev
 * bf16 in the kernel's packed fragment order (amuse_audio_api.hip pack_w), N % 256 == 0, K % 64 == 0;
 * epi 0: out dev bf16 tile-major [M rounded up to 128][N], epi 3: the same in fp32. */
int amuse_debug_gemm(const void* A, const void* W, const float* bias, int M, int N, int K, int epi,
                     void* out, void* stream);
/* Row-major <-> tile-major copies for the above (F % 32 == 0).  what 0: bf16 row-major [M][F] -> tile-major [M rounded up
 * to 128][F], pad rows zeroed; 1: bf16 tile-major -> row-major [M][F]; 2: fp32 tile-major -> row-major [M][F]. */
int amuse_debug_tile(const void* src, void* dst, int M, int F, int what, void* stream);

/* Debugging taps of the FUSED bf16 decode kernel (k_vae_fused.hip), for tests: while tap_out (dev [11][300][128] fp32) is set,
 * every fused amuse_vae_decode launch writes clip 0's residual stream after decoder blocks 0..8 (slots 0..8), after
 * decoder.norm (slot 9) and behind block 0's norm1 (slot 10: norm1(PE + SA(PE)), the per-weight-set constant full-length clips start
 * from) there, through a separate instantiation of the kernel; NULL switches the taps off again. */
int amuse_debug_set_decode_tap(amuse_ctx* ctx, float* tap_out);

/* Timing ablation of the fused per-clip kernels (k_vae_fused.hip, k_den_fused.hip), for bench.py's attention-only roofline figure:
 * mask 1 = launch the instantiation WITHOUT softmax(Q K^T) V (projections, K / V images, out_proj and every barrier stay) - outputs
 * are wrong by construction; full - ablated launch time = the S ~ 300 self-attention's time.  mask 0 restores the product kernel. */
int amuse_debug_set_ablation(amuse_ctx* ctx, int mask);

/* The host packer's fp32 -> (hi, lo) fp16 split of AMUSE_PREC_F32X, for tests (host memory, no GPU call):
 * hi[i] = rn16(w[i]), lo[i] = rn16(w[i] - hi[i]), round-to-nearest-even with gradual underflow - bit for bit what
 * v_cvt_pk_f16_f32 produces on the device for the activations (and amuse_update_weights_device for the weights). */
int amuse_debug_f16_split(const float* w, size_t n, uint16_t* hi, uint16_t* lo);

/* ------------------------------------------------------------------ training-step glue (csrc/k_train.hip; amuse_amd/train_ops.py)
 * The row-wise arithmetic of a transformer layer's forward and backward pass in the train_gesture iteration (reference
 * scripts/trainer.py:335-498; layers utils/cross_attention.py:259-272,323-345; the reference gets these from torch's eager kernels:
 * nn.Dropout, the residual add, nn.LayerNorm, F.gelu and the bias gradients' reductions).  fp32, row-major [rows][C]; no context - plain
 * device pointers and a stream.  Dropout masks are counter-based: element e is draw e % 4 of Philox4x32-10(key seed, counter (e / 4, offset));
 * the backward calls regenerate the mask from the same (p, seed, offset).  p = 0 is eval mode.
 * `ws` (amuse_train_ws_floats() floats) holds the partial column sums of a call (deterministic: added up in a fixed order by a second launch) and
 * must not be shared by calls that may overlap on different streams. */
size_t amuse_train_ws_floats(void);
/* The library's OWN scratch (split-k partials of the weight gradients and of the generic GEMM) exists once per device and LANE (0 or 1): calls that may overlap on two
 * streams of a device - the trainer issues the Denoiser's forward / backward pass beside the prior's - run on different lanes.  Sets the lane of the CALLING THREAD for
 * its following amuse_train_* calls (initially 0). */
int amuse_train_set_lane(int lane);
/* out = LayerNorm_128(x + dropout(y + bias)) (x, bias nullable); zhat [rows][128] = the normalised rows and rstd [rows] for the backward
 * pass (both nullable) */
int amuse_train_ln_fwd(const float* x, const float* y, const float* bias, const float* gamma, const float* beta, float p, uint64_t seed,
                       uint64_t offset, long rows, float* out, float* zhat, float* rstd, void* stream);
/* dz = LayerNorm backward of dout + dout2 (dout2 nullable: the second branch's gradient of a residual stream); dx = dz (nullable),
 * dy = dz . mask / (1 - p); dgamma, dbeta, dbias = sum_rows dy (each nullable) */
int amuse_train_ln_bwd(const float* dout, const float* dout2, const float* zhat, const float* rstd, const float* gamma, float p, uint64_t seed, uint64_t offset,
                       long rows, float* dx, float* dy, float* dgamma, float* dbeta, float* dbias, float* ws, void* stream);
/* out = dropout(gelu(h + b)), exact erf; h, out [rows][F], F a multiple of 4 up to 1024 */
int amuse_train_bias_gelu_drop_fwd(const float* h, const float* b, float p, uint64_t seed, uint64_t offset, long rows, int F, float* out,
                                   void* stream);
/* dh = da . mask / (1 - p) . gelu'(h + b); db [F] = sum_rows dh */
int amuse_train_bias_gelu_drop_bwd(const float* da, const float* h, const float* b, float p, uint64_t seed, uint64_t offset, long rows,
                                   int F, float* dh, float* db, float* ws, void* stream);
/* out [C] = sum_rows x[r][:] (a bias gradient), C a multiple of 4 up to 1024 */
int amuse_train_colsum(const float* x, long rows, int C, float* out, float* ws, void* stream);

/* Self-attention core of a layer (nn.MultiheadAttention between its in- and out-projection, 4 heads of 32, S <= 304 tokens) in fp32 on the matrix cores
 * (csrc/k_train_attn.hip): o [B S][128] = dropout(softmax(q k^T / sqrt(32))) v per (clip, head) from the packed projections qkv [B S][384] (q | k | v,
 * heads contiguous 32-column slices), lse [B][4][S] for the backward pass; the backward call returns d(qkv).  The dropout mask is a hash of
 * (seed, offset, clip, head, query, key): the backward call regenerates it from the same (p, seed, offset).  mask_debug (nullable): [B][4][S][S] keep / (1 - p). */
int amuse_train_attn_fwd(const float* qkv, int B, int S, float p, uint64_t seed, uint64_t offset, float* o, float* lse, float* mask_debug, void* stream);
int amuse_train_attn_bwd(const float* qkv, const float* o, const float* lse, const float* dout, int B, int S, float p, uint64_t seed, uint64_t offset,
                         float* dqkv, void* stream);
/* torch.optim.AdamW (amsgrad off) over a contiguous range of flat fp32 buffers, `step` = this update's 1-based count (trainer.py:181-184: the reference's
 * optimizer over prior + ldm parameters; amuse_amd/train_gesture.py keeps parameters, gradients and both moments in one buffer each) */
int amuse_train_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1, double beta2, double eps,
                      double weight_decay, long step, void* stream);
/* The same update with the step count on the DEVICE - for a training step captured as a HIP graph, whose host-side count is frozen at capture:
 * advance != 0 first adds 1 to *step_dev and leaves the two bias-correction scalars (computed in double, as the host path does) in scal_dev[0..1]; the update
 * then reads them.  One advancing call per optimizer step, advance = 0 for the step's further ranges.  step_dev, scal_dev: device memory (8 + 8 bytes). */
int amuse_train_adamw_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1, double beta2, double eps,
                          double weight_decay, long* step_dev, float* scal_dev, int advance, void* stream);
/* The dropout epoch: one device word per GPU that every mask-drawing kernel of the training step (LayerNorm / FFN / value-path dropouts, the attention's hash)
 * mixes into its counter.  It is 0 unless advanced - eager training hands every call a fresh (seed, offset) from the host.  A step captured as a HIP graph
 * replays with the offsets it was captured with, so the graph ends with amuse_train_epoch_advance(1): every replay then draws fresh masks, and the forward and
 * backward halves of one step still see the same value.  amuse_train_epoch_set pins it (tests, resuming). */
int amuse_train_epoch_advance(unsigned add, void* stream);
int amuse_train_epoch_set(unsigned value, void* stream);
/* Layer-level entry points: a whole TransformerEncoderLayer / TransformerDecoderLayer (forward_post, memory of one token) but its self-attention
 * core, forward and backward, in one call each - the kernels above plus the layer's plain GEMMs on the library's own fp32-MFMA kernels
 * (csrc/k_train_gemm.hip; no vendor BLAS).  The caller computes q | k | v = amuse_train_linear_fwd(x, in_proj), runs its attention on them (o2 = the heads' outputs
 * concatenated), calls amuse_train_layer_fwd; on the way back amuse_train_layer_bwd returns d(o2) for the attention's backward pass, whose d(q | k | v)
 * goes through amuse_train_linear_bwd(..., dx = L.dx, accumulate_dx = 1).  Linear weights in PyTorch's [out][in] layout, everything fp32 and dense. */
typedef struct amuse_train_layer {
    long rows; int B, S, H, ff;                 /* rows = B x S tokens of 128 features; H heads; ff = linear1's width (multiple of 4, <= 1024) */
    float p, p_attn;                            /* dropout probabilities: the layer's nn.Dropout modules / the attention's (0 = eval mode) */
    uint64_t seed, off[5];                      /* mask offsets: [0] behind the self-attention, [1] behind the cross-attention, [2] inside the FFN,
                                                   [3] behind the FFN, [4] the cross-attention's probabilities */
    const float *Wo, *bo, *g1, *be1;            /* self_attn.out_proj, norm1 */
    const float *Wv, *bv, *Wc, *bc, *g2, *be2;  /* decoder layer: multihead_attn's value rows of in_proj, its out_proj, norm2 (NULL for an encoder layer) */
    const float *W1, *b1, *W2, *b2, *g3, *be3;  /* linear1, linear2, the last norm (an encoder layer's norm2) */
    const float *x, *o2, *mem;                  /* in: residual stream [rows][128], attention output [rows][128], memory [B][128] (NULL: encoder layer) */
    float *x1, *zh1, *r1;                       /* kept for the backward pass: behind norm1 ([rows][128], normalised rows, [rows]) */
    float *c, *vk, *xm, *zh2, *r2;              /* decoder: value projection [B][128], its masked copy [rows][128], behind norm2 */
    float *h, *a;                               /* [rows][ff]: linear1's output, the FFN activation */
    float *out, *zh3, *r3;                      /* the layer's output and the last norm's state */
    float *tmp;                                 /* [rows][128] scratch */
    const float* dout;                          /* backward in: d(out) */
    float *dx, *do2, *dmem;                     /* backward out: d(x) WITHOUT the attention's share, d(o2), d(mem) [B][128] */
    float *dWo, *dbo, *dg1, *dbe1, *dWv, *dbv, *dWc, *dbc, *dg2, *dbe2, *dW1, *db1, *dW2, *db2, *dg3, *dbe3;
    float *s128a, *s128b, *s512a, *s512b, *sdc; /* backward scratch: 2 x [rows][128], 2 x [rows][ff], [B][128] */
    float* ws;                                  /* amuse_train_ws_floats() floats */
    /* optional: the layer's self-attention inside the same calls (Win != NULL; 4 heads, S <= 304).  Forward: qkv = x Win^T + bin, o2 = attention(qkv)
     * (o2 then is an OUTPUT buffer), lse kept; backward: d(qkv) from d(o2), dWin / dbin, and dx receives the attention's share too. */
    const float *Win, *bin;                     /* self_attn.in_proj_weight [384][128], in_proj_bias [384] */
    float *qkv, *lse;                           /* [rows][384], [B][4][S]: kept for the backward pass */
    float *dqkv, *dWin, *dbin;                  /* backward: [rows][384] scratch, the in-projection's gradients */
    uint64_t off_self;                          /* mask offset of the self-attention's dropout */
} amuse_train_layer;
int amuse_train_layer_fwd(const amuse_train_layer* layer, void* stream);
/* (amuse_train_layer_bwd of a decoder layer with >= 1,024 rows issues the memory token's branch - d(c), dWv, dbv, d(mem) - on a stream of the library's own, forked from
 * and joined back into `stream` inside the call: everything is complete in `stream` order when the call returns, also under stream capture) */
int amuse_train_layer_bwd(const amuse_train_layer* layer, void* stream);
/* out [rows][N] = x [rows][K] W^T + b (b nullable);  dW [N][K] = dy^T x, db [N] = sum_rows dy, dx [rows][K] (+)= dy W (each output nullable) */
int amuse_train_linear_fwd(const float* x, const float* W, const float* b, long rows, int K, int N, float* out, void* stream);
int amuse_train_linear_bwd(const float* dy, const float* x, const float* W, long rows, int K, int N, float* dW, float* db, float* dx,
                           int accumulate_dx, float* ws, void* stream);

/* ------------------------------------------------------------------ SMPL-X body model (csrc/amuse_body.hip, k_body.hip, amuse_body_grad.hip, k_body_bwd.hip; amuse_amd/body.py)
 * Replaces what the reference gets from the `smplx` package in LatentPriorLosses._get_vertices (models/latent_diffusion/utils/latent_losses.py:135-146,173-250):
 * SMPLX(num_betas = n_betas, use_pca=False, flat_hand_mean=True) called with expression = 0 - linear blend skinning, generic in the vertex count - and the two
 * vertex-displacement terms built on it.  A context of its own, independent of amuse_ctx; the arrays are what a user loads from their own SMPLX_*.npz.
 * `smplx` is not a dependency of this project: parity is against a RESTATEMENT of the published algorithm (tests/body_ref.py), not a pin.
 * Per frame: v_shaped = v_template + shapedirs . betas; J = J_regressor . v_shaped (both hoisted per subject: amuse_body_set_subjects); R_j = Rodrigues(pose_j)
 * (angle = |pose_j + 1e-8|, a zero vector gives the identity) or the Gram-Schmidt of rotation_6d_to_matrix; pose_feature = (R_1..R_54 - I) row-major [486];
 * v_posed = v_shaped + pose_feature . posedirs; the kinematic chain over `parents`; A_j = [G_j.R | G_j.t - G_j.R J_j];
 * vertex_v = (sum_j w[v][j] A_j) . [v_posed_v; 1] + transl, posed joint j = G_j.t + transl.
 * Host arrays of the model (fp32 / int32, copied by amuse_body_create):
 *   v_template [V][3], shapedirs [V][3][n_betas], posedirs [486][V * 3] (the file's [V][3][486] transposed), J_regressor [55][V], weights [V][55],
 *   parents [55] with parents[0] = -1 and 0 <= parents[j] < j (AMUSE_EINVAL otherwise: amuse_body_create returns NULL). */
typedef struct amuse_body_ctx amuse_body_ctx;
typedef struct {
    int V, n_betas;
    const float* v_template;
    const float* shapedirs;
    const float* posedirs;
    const float* J_regressor;
    const float* weights;
    const int* parents;
} amuse_body_model;
/* rotation input: AA = axis-angle rows, 6D = the project's feature rows [N][F][333] (55 x 6D | translation) */
enum { AMUSE_BODY_ROT_AA = 0, AMUSE_BODY_ROT_6D = 1 };
/* Packs the pose-corrective matrix into MFMA-fragment order (four output slots x, y, z, pad per vertex; hi and lo fp16 planes of the entries pre-scaled by a
 * power of two - exact, undone on the accumulator - so that their pieces stay clear of fp16's subnormals) and the skinning weights into per-vertex
 * (joint, weight) lists padded to the model's largest non-zero count (exact for any weight matrix, dense rows included).  Returns NULL on failure. */
amuse_body_ctx* amuse_body_create(int device, const amuse_body_model* model);
void amuse_body_destroy(amuse_body_ctx* ctx);
/* betas host [S][n_betas]: v_shaped and J of every subject, on the host in double, uploaded as fp32 (the reference recomputes them per frame: the same values).
 * Not stream-ordered: call it between, not during, the context's calls. */
int amuse_body_set_subjects(amuse_body_ctx* ctx, const float* betas, int S);
/* Sizes the workspace for calls of up to `frames` = N * F frames (three motion sets).  The compute calls size it themselves on first use; after a reserve that
 * covers them they allocate nothing and synchronise nothing, so they can sit inside a captured graph.  Preconditions:
 *   - growing allocates (so it must not happen inside a capture: reserve, or run the call once eagerly, BEFORE capturing); the outgrown workspace stays alive
 *     until amuse_body_destroy, so a graph captured earlier keeps replaying into valid memory;
 *   - a context has ONE workspace: its compute calls must not overlap in time, i.e. one stream per context (or calls ordered by events), as for amuse_ctx.
 * Not stream-ordered itself: call it between, not during, the context's calls. */
int amuse_body_reserve(amuse_body_ctx* ctx, size_t frames);
/* rot_kind AA: rot dev [N][F][55][3], trans dev [N][F][3] or NULL (zero); 6D: rot dev [N][F][333], trans ignored (the row's last three).
 * subject_dev: DEVICE int32 [N], the subject (row of amuse_body_set_subjects) of each clip; a clip whose value lies outside 0..S-1 is SKIPPED: its output rows
 * are left untouched and it adds nothing to the loss sums (the trainer's gendered split: each model's call names its own clips, on the device).
 * joints_out dev [N][F][55][3], vertices_out dev [N][F][V][3], either nullable (64-bit offsets).
 * precision: AMUSE_PREC_F32X - the pose-blend product on split-fp16 operands (Pl.fh + Ph.fl + Ph.fh on v_mfma_f32_16x16x32_f16, fp32 accumulation) - or
 * AMUSE_PREC_F16 (one product); everything else is fp32 in both.  Other values: AMUSE_EINVAL. */
int amuse_body_forward(amuse_body_ctx* ctx, const float* rot, int rot_kind, const float* trans, const int* subject_dev, int N, int F, int precision,
                       float* joints_out, float* vertices_out, void* stream);
/* The two vertex-displacement terms: sums_out dev double [2] = the SmoothL1 (beta 1) SUMS over all N F V 3 vertex coordinates of (a, ref) and (b, ref); b may be
 * NULL (sums_out[1] = 0).  The caller divides (by N F V 3 for the reference's mean).  ref / a / b: rot_kind 6D dev [N][F][333]; AA dev [N][F][168] = 55 x 3
 * axis-angle | translation (the trainer's ld_motion rows).  No vertex array is written: the sets of a frame tile meet in registers.  Deterministic: per-workgroup
 * fp32 partials, then a fixed-order double sum in a second launch; no float atomics. */
int amuse_body_vertex_loss(amuse_body_ctx* ctx, const float* ref, const float* a, const float* b, int rot_kind, const int* subject_dev, int N, int F,
                           int precision, double* sums_out, void* stream);
/* Gradients of the vertex objective (csrc/amuse_body_grad.hip, k_body_bwd.hip).  OPT-IN: the reference computes its vertices under no_grad
 * (latent_losses.py:173) and the calls above are its values; nothing of them changes when gradients are enabled.
 * amuse_body_enable_grad builds and uploads a second packed image of posedirs, TRANSPOSED (512 feature rows x the padded vertex slots of a pair of vertex
 * groups, hi | lo planes, the forward image's halfs bit for bit), which the backward pass's transposed pose-blend product reads: pairs x 65,536 bytes with
 * pairs = ceil(ceil(V / 4) / 2), i.e. 85,852,160 bytes at V = 10,475.  A context that never calls it keeps the memory it had.  From then on the workspace
 * (amuse_body_reserve, or a call's own sizing) also holds the backward kernels' per-workgroup partials: (frames16 / 16 + 512) x 75,264 bytes.
 * Not stream-ordered (it copies synchronously and allocates): call it between the context's calls and BEFORE any capture.  Idempotent. */
int amuse_body_enable_grad(amuse_body_ctx* ctx);
/* d/d(a), d/d(b) of the SmoothL1 (beta 1) SUMS amuse_body_vertex_loss returns: grad_a / grad_b dev [N][F][333] = scale_a x dS_a/da, scale_b x dS_b/db (the
 * 330 6D columns and the three translation columns); the reference motion gets no gradient.  b and grad_b are NULL together.  Rows of skipped clips (subject
 * outside 0..S-1) are left untouched.  SmoothL1's derivative clamp(d, -1, 1) is continuous, so no input has to avoid |d| = 1.
 * rot_kind must be AMUSE_BODY_ROT_6D: axis-angle rows return AMUSE_EINVAL, because the published Rodrigues form (angle = |r + 1e-8|) has no usable derivative
 * at the zero vector, which rest poses contain.  AMUSE_ESTATE before amuse_body_enable_grad.
 * The forward pass of the reference and one candidate per pass is recomputed (same fragments and precision as amuse_body_vertex_loss; `precision` also
 * selects split-fp16 or one-product fp16 for the transposed product), no vertex is written.  Deterministic - the same inputs give the same bits: the skinning
 * gradients accumulate as int64 fixed point (value x 2^38; integer sums do not depend on arrival order) in LDS, the matrix-core accumulators of a workgroup's
 * waves are added in wave order, and a per-frame kernel adds the per-workgroup partials in index order in double.  No float atomics.
 * Workspace rules as for amuse_body_reserve: after a reserve (made after amuse_body_enable_grad) that covers the call it allocates nothing and synchronises
 * nothing; growing never frees what an earlier graph may replay into. */
int amuse_body_vertex_loss_grad(amuse_body_ctx* ctx, const float* ref, const float* a, const float* b, int rot_kind, const int* subject_dev, int N, int F,
                                int precision, float scale_a, float scale_b, float* grad_a, float* grad_b, void* stream);
/* diagnostics (host values): what = 0 V, 1 largest non-zero count of a skinning row, 2 the power-of-two pre-scale exponent of posedirs, 3 subjects set,
 * 4 gradients enabled (0 | 1) */
int amuse_body_info(const amuse_body_ctx* ctx, int what);

/* ------------------------------------------------------------------ long-form inference (csrc/amuse_stitch_host.hpp, amuse_stitch.hip, k_stitch.hip; amuse_amd/longform.py)
 * AN EXTENSION: the reference has no such path - it asks for 10 s WAVs ("Make sure each audio is a 10 sec wav file", scripts/trainer.py:506).  A longer waveform is
 * cut into overlapping windows of the model's clip (F = 300 frames = 160,000 samples: 16 kHz audio, 30 fps motion, the rates the reference assumes of every file;
 * nothing resamples), every window is embedded and sampled as a clip of its own - INDEPENDENTLY: the Denoiser's state is one latent per clip, nothing is shared
 * between windows - and the frames two neighbouring windows both produced are crossfaded.  The crossfade hides the seam; it does not make the windows agree
 * (the long-form candidates section below CHOOSES, among K samples of every window, the ones that agree best where they meet; for K = 1 the sentence stands).
 *
 * The window plan, stated once; needs no GPU and no context.  hop_frames h: the stride between window starts, a multiple of 3 (so that the hop is the whole
 * number h / 3 * 1600 of samples) with 150 <= h <= 300 (so that at most two windows cover a frame); the product's default is 270, one second of overlap.
 *   *frames       L = max(300, floor(3 n / 1600))
 *   *windows      W = 1 if L <= 300, else ceil((L - 300) / h) + 1
 *   *hop_samples  hs = h / 3 * 1600
 * Window w reads the samples [w hs, min(w hs + 160000, n)) and yields the frames [w h, w h + 300) of the sequence, cut at L.  The last window may be short: it
 * goes through the front-end's pad path, as a short WAV does.  By this arithmetic the last window of W > 1 always holds MORE than 300 - h frames of audio
 * ((W - 1) h < L - 300 + h and n >= 1600 L / 3), i.e. every frame past the last overlap comes from audio, never from padding alone.  n <= 160,000 gives W = 1,
 * L = 300: one clip, as without the plan.  Any output pointer may be NULL.  AMUSE_EINVAL for n < 0 (or beyond an int of frames) and for a bad h. */
int amuse_longform_plan(long long n_samples, int hop_frames, int* windows, int* frames, int* hop_samples);
/* The join.  Context-free and stream-ordered; no allocation, no copy, no host synchronisation: it can be captured.  The per-sequence offsets travel by value in
 * the kernel arguments, 32 sequences per launch; a call with more sequences takes ceil(S / 32) launches.
 *   poses dev [sum W_s][F][55][3] axis-angle, trans dev [sum W_s][F][3]: the windows of S sequences back to back, as amuse_diffusion_backward writes them
 *   windows / frames: HOST int [S], W_s and L_s;  blend dev [F - hop] (may be NULL when hop == F);  poses_out dev [sum L_s][55][3], trans_out dev [sum L_s][3]
 *   trans and trans_out are NULL together (poses only).
 * Output frame f of a sequence, with k = min(f / hop, W - 1), i = f - k hop, O = F - hop:
 *   k == 0 or i >= O   a BITWISE copy of window k's row i (rotations beyond pi stay as they are)
 *   otherwise          window k - 1's row i + hop (a) and window k's row i (b) at weight w = blend[i]: translation (1 - w) a + w b; each joint in fp32: axis-angle
 *                      -> unit quaternion; q_b negated where q_a . q_b = d < 0; Omega = atan2(|q_b - d q_a|, d); (sin((1 - w) Omega) q_a + sin(w Omega) q_b) /
 *                      sin Omega (the linear form (1 - w) q_a + w q_b where sin Omega < 1e-4), normalised, negated if its real part is negative, -> axis-angle
 *                      by the arithmetic of the decode tail.  Blended rows therefore carry angles <= pi.
 * The product's weights are 0.5 - 0.5 cos(pi (i + 1) / (O + 1)), i = 0 .. O - 1, computed in double and rounded to fp32 (amuse_amd/longform.py blend_weights).
 * Checked before any HIP call, AMUSE_EINVAL otherwise: S >= 1; F >= 2 (the product passes 300); F / 2 <= hop <= F; for every s, W_s >= 1 and
 * (W_s - 1) hop < L_s <= (W_s - 1) hop + F; the pointers above non-NULL; the call's window rows and 56 x its output frames within an int. */
int amuse_stitch_windows(const float* poses, const float* trans, int S, const int* windows, const int* frames, int F, int hop, const float* blend,
                         float* poses_out, float* trans_out, void* stream);

/* ------------------------------------------------------------------ long-form candidates (csrc/amuse_seam_host.hpp, amuse_seam.hip, k_seam.hip; amuse_amd/seam.py)
 * AN EXTENSION of the extension above, off by default: K candidates of every window are sampled in the one batch long-form inference launches anyway, every
 * (candidate of window k, candidate of window k + 1) pair is scored by how far the frames the two windows share are apart AS ROTATIONS, and the path through the
 * windows with the least total cost is what the join above then crossfades.  The project's OWN method: compared with no other implementation, checked against its
 * own float64 restatement (tests/seam_ref.py) only.  Whether the candidates of a TRAINED checkpoint differ enough at the seams for the choice to matter has not
 * been measured by anybody (profiles/seam_cost.txt: random-init weights only).
 *
 * Batch layout: row g K + c is candidate c of window g (windows in sequence order, then window order, as above; candidate fastest).  K = 1 is the join's layout.
 * All four calls are context-free; the last three are stream-ordered, allocate nothing, copy nothing and never synchronise: they can be captured.  Per-sequence
 * offsets travel by value in the kernel arguments, 32 sequences per launch.  Every check is made before any HIP call and answers AMUSE_EINVAL.
 *
 * amuse_seam_plan: host only.  *seams = sum (W_s - 1); *workspace_bytes = seams x 2 x K x (F - hop) x 55 x 16: the unit quaternions of every overlap row, each
 * converted ONCE (0 without a seam).  The one statement of both numbers; either pointer may be NULL.  Checked: S >= 1; windows given, 1 <= W_s <= 32768; K in
 * 1..64; F >= 2; F / 2 <= hop < F when any W_s > 1 (hop <= F otherwise); the call's batch rows x F and seams x K x K within an int. */
int amuse_seam_plan(int S, const int* windows, int K, int F, int hop, long long* seams, size_t* workspace_bytes);
/* The cost matrix.
 *   poses dev [sum W_s K][F][55][3] axis-angle, trans dev [sum W_s K][F][3] or NULL (then trans_weight must be 0);  windows / frames: HOST int [S], as for the join,
 *   with its (W - 1) hop < L <= (W - 1) hop + F check;  row_weight dev [F - hop], joint_weight dev [55], trans_weight: REQUIRED finite and >= 0 - the two device
 *   arrays cannot be checked without a copy, so they are not: a negative or non-finite weight gives a cost that means nothing (trans_weight is checked);
 *   workspace dev, 16-byte aligned, what amuse_seam_plan asks for;  cost_out dev double [seams][K][K], the seams of sequence s from sum_{s' < s} (W_s' - 1).
 * Seam k of a sequence, a = candidate of window k, b = candidate of window k + 1, over the overlap rows that reach the output, i < O_k = min(F - hop, L - (k + 1) hop):
 *   cost[k][a][b] = sum_i row_weight[i] ( sum_j joint_weight[j] theta_ij^2 + trans_weight |t_a(i + hop) - t_b(i)|^2 )
 * theta_ij, in fp32: q = axis-angle -> unit quaternion of joint j of a's row i + hop and of b's row i (the join's arithmetic, series below 1e-6); r = conj(q_a) q_b;
 * theta = 2 atan2(|r.xyz|, |r.w|) - no acos, and the hemisphere by the absolute value: the 2 pi - theta alias of a rotation costs what the rotation costs.  The
 * translation's differences are fp32.  The squares, the products with the weights and all sums are double, in ONE order: per joint (and for the translation) over
 * the rows i = 0, 1, .. as acc += row_weight[i] * (weight * square); then those 56 sums (and 8 zeros) as 64 lanes by the xor butterfly at distances 32, 16, 8, 4,
 * 2, 1.  A pair's cost has the same bits whatever K, launch, sequence position or batch it is computed in.  No atomics.
 * With no seam in the call nothing is launched and row_weight, workspace and cost_out may be NULL. */
int amuse_seam_cost(const float* poses, const float* trans, int S, const int* windows, const int* frames, int K, int F, int hop, const float* row_weight,
                    const float* joint_weight, float trans_weight, void* workspace, double* cost_out, void* stream);
/* The best path: exact dynamic programming in double, one wave per sequence, a lane per candidate.
 *   cost dev double [seams][K][K] as above;  choice_out dev int [sum W_s]: the chosen BATCH ROW g K + c of every window;  total_out dev double [S].
 *   best[0][c] = 0;  best[k][b] = min over a = 0, 1, .. of v(best[k - 1][a] + cost[k - 1][a][b]);  the end candidate: the minimiser of best[W - 1][.];  then back
 *   along the minimisers.  v(x) = x if x is finite, +infinity otherwise.  Every minimum starts from (+infinity, candidate 0) and is replaced on `<` only: ties go to
 *   the lowest index, and where nothing is finite the candidate is 0 (and the total +infinity).  W = 1: candidate 0, total 0.  Any W (back-pointers are kept in LDS
 *   for 960 windows at a time; longer sequences repeat the forward pass). */
int amuse_seam_path(const double* cost, int S, const int* windows, int K, int* choice_out, double* total_out, void* stream);
/* The gather: output row r is a BITWISE copy of input row choice[r], into the layout the join reads.
 *   poses dev [n_in][F][55][3], trans dev [n_in][F][3];  choice dev int [n];  poses_out dev [n][F][55][3], trans_out dev [n][F][3].  trans and trans_out are NULL
 *   together.  A choice outside 0 .. n_in - 1 is never read: its output row is NaN.  No output range may overlap an input range or the other output. */
int amuse_seam_select(const float* poses, const float* trans, const int* choice, int n, int n_in, int F, float* poses_out, float* trans_out, void* stream);

/* ------------------------------------------------------------------ motion smoothing (csrc/amuse_smooth_host.hpp, amuse_smooth.hip, k_smooth.hip; amuse_amd/smooth.py)
 * AN EXTENSION, off by default: the reference writes the decoder's rows as they come, frame by frame.  A Savitzky-Golay filter over time, on SO(3) for the
 * 55 joints and on R^3 for the translation.  It is this project's OWN statement of the method, in the manner of "geometric Savitzky-Golay filtering" on SO(3),
 * written down from memory: pinned against no other implementation, except the Euclidean half (the bank and the translation) against scipy.signal
 * (tests/test_smooth_cpu.py); the rotation half is checked against its own float64 restatement (tests/smooth_ref.py) only.  The product's default of a 9-frame
 * window at order 3 (30 fps) is a RECOLLECTION of common practice, not a measurement.
 *
 * Parameters: a half-window m_j in 0..15 for each of the 55 joints and one for the translation (56 values), and ONE polynomial order p in 0..5.  The effective
 * order at half-window m is p_m = min(p, 2 m).
 * The bank: for m >= 1, H_m = A (A^T A)^-1 A^T with A[i][d] = (i - m)^d, i = 0 .. 2 m, d = 0 .. p_m - the (2 m + 1) x (2 m + 1) hat matrix of the local
 * polynomial fit.  Row m is the classic central Savitzky-Golay kernel; the other rows evaluate the SAME fit at the window's other positions and are used at a
 * sequence's two ends (scipy.signal.savgol_filter(mode="interp")).  Computed on the host in double (through an orthonormal basis of A's columns on the
 * abscissae scaled to [-1, 1]: the same matrix, without the conditioning of A^T A) and rounded to fp32.
 * amuse_smooth_banks: host only, no GPU, no context.  Writes H_1 .. H_15 back to back, row-major - 9 + 25 + ... + 961 = 5,455 floats; H_m starts at float
 * n (4 n^2 + 12 n + 11) / 3, n = m - 1 - for p_m = min(order, 2 m).  AMUSE_EINVAL for an order outside 0..5 or a NULL pointer. */
#define AMUSE_SMOOTH_MAX_HALF 15
#define AMUSE_SMOOTH_BANK_FLOATS 5455
int amuse_smooth_banks(int order, float* banks_out_host);
/* The filter.  Context-free and stream-ordered; allocates nothing, copies nothing, never synchronises: it can be captured.  The per-sequence offsets and the 56
 * half-windows travel by value in the kernel arguments, 32 sequences per launch; a call with more sequences takes ceil(S / 32) launches.
 *   poses dev [sum L_s][55][3] axis-angle, trans dev [sum L_s][3]: S sequences back to back;  frames: HOST int [S], L_s;  half_window: HOST unsigned char [56],
 *   m_0 .. m_54 of the joints and m_55 of the translation;  banks_dev: dev [5455], what amuse_smooth_banks wrote;  poses_out / trans_out: as the inputs.
 *   trans and trans_out are NULL together (poses only).
 * Output frame f of a sequence of L frames, joint j, m = m_j:
 *   m == 0 or L < 2 m + 1   a BITWISE copy of the input row (angles beyond pi stay as they are)
 *   otherwise               window start s = clamp(f - m, 0, L - 1 - 2 m), bank row r = f - s; every step in fp32:
 *       q_k = the unit quaternion of input frame s + k, k = 0 .. 2 m: axis-angle a, t = |a|, (cos(t / 2), a sin(t / 2) / t), with sin(t / 2) / t taken as
 *             1 / 2 - t^2 / 48 where t < 1e-6 (the decode tail's axis-angle arithmetic, read the other way; the stitch's)
 *       q_c = q_r, the frame itself;  d_k = conj(q_c) q_k, negated where its real part is < 0
 *       v_k = log(d_k) as a rotation vector: n = |vec d_k|, v_k = (2 atan2(n, w) / n) vec d_k, the factor taken as 2 where n < 1e-6
 *       v = sum over k = 0 .. 2 m, in that order, of H_m[r][k] v_k
 *       out = q_c exp(v) (exp: the axis-angle -> quaternion step above), normalised, negated if its real part is negative, -> axis-angle by the arithmetic of
 *       the decode tail.  Smoothed rows therefore carry angles <= pi.
 *   translation (m = m_55): sum over k = 0 .. 2 m, in that order, in fp32, of H_m[r][k] x[s + k], per component; the same copy rule.
 * This is the polynomial fit in the tangent space AT THE FRAME BEING FILTERED - the only space in which the negative lobes of a Savitzky-Golay kernel mean
 * anything; nothing is fitted to Euler angles or raw rotation vectors, which is wrong near pi and for large rotations.  A frame's result depends on the
 * frames of its window alone: not on the sequence's place in the call, nor on the launch or tile it falls in (one code path for interior and edge frames).
 * Checked before any HIP call, AMUSE_EINVAL otherwise: S >= 1; every L_s >= 1; every half_window[i] <= 15; 56 x sum L_s within an int; poses, frames,
 * half_window, banks_dev, poses_out non-NULL and the trans pair as stated; no output range may overlap an input range (the filter reads a frame's
 * neighbours: in place is refused). */
int amuse_smooth_motion(const float* poses, const float* trans, int S, const int* frames, const unsigned char* half_window, const float* banks_dev,
                        float* poses_out, float* trans_out, void* stream);

/* ------------------------------------------------------------------ BVH export (csrc/amuse_bvh_host.hpp, amuse_bvh.hip, k_bvh.hip; amuse_amd/bvh.py)
 * AN EXTENSION, off by default: the reference retargets its NPZ output to BVH through Blender; this writes the SMPL-X skeleton itself as BVH - the hierarchy on
 * the host, the MOTION block (Euler channels in degrees, as text) on the GPU.  No BVH importer is pinned anywhere in this project: the files are checked against
 * the format's grammar through the project's own reader and their numbers against scipy (tests/test_gpu_bvh.py).
 *
 * A MOTION row is 168 numbers: the root's three position channels, then three rotation channels per joint, joints in the DEPTH-FIRST order of the parent list
 * with children in ascending index.  Every number is the 11 characters of C's "%11.6f" and one separator byte - a space, '\n' after a row's last number - so a
 * row is 168 x 12 = 2,016 bytes and a clip of F frames is F x 2,016 bytes at a known offset: there is no size pass.
 *
 * amuse_bvh_layout: host only, no GPU, no context.  dfs_out[c] = the joint of column c for parents[0] = -1, 0 <= parents[j] < j.  AMUSE_EINVAL otherwise, for
 * n outside 1..65536 and for NULL pointers. */
#define AMUSE_BVH_COLS 168
#define AMUSE_BVH_FIELD 12
enum { AMUSE_BVH_XYZ = 0, AMUSE_BVH_XZY = 1, AMUSE_BVH_YXZ = 2, AMUSE_BVH_YZX = 3, AMUSE_BVH_ZXY = 4, AMUSE_BVH_ZYX = 5 };
int amuse_bvh_layout(const int* parents, int n, int* dfs_out);
/* The formatter on its own.  Context-free and stream-ordered; allocates nothing, copies nothing, never synchronises: it can be captured.
 *   values dev fp32 [n];  text_out dev bytes [12 n], 4-byte aligned;  status dev int [1].
 * Field i is exactly C's "%11.6f" of values[i] - round-half-even at the sixth decimal, "-0.000000" for -0 and for negatives that round to zero - followed by
 * '\n' where i % per_row == per_row - 1 and by a space elsewhere.  (An fp32 times 1e6 is exact in double, so rint(double(x) * 1e6) is the integer printf prints.)
 * A value that does not fit - |x| rounding to 1000 or more, NaN, infinity - has its 11 characters filled with '#' and sets *status to 1 by a plain store;
 * status is never cleared here.  No byte outside [0, 12 n) is written.
 * AMUSE_EINVAL before any HIP call: n < 1, per_row < 1, a NULL pointer, text_out not 4-byte aligned. */
int amuse_bvh_format(const float* values, long long n, int per_row, void* text_out, int* status, void* stream);
/* The exporter.  Context-free, stream-ordered, capturable; the per-sequence offsets and the column order travel by value in the kernel arguments, 32 sequences
 * per launch.
 *   poses dev [rows][55][3] axis-angle, trans dev [rows][3] or NULL (zero): S sequences back to back, rows = sum F_s;  root_rest dev [S][3]: J_rest[0] of each
 *   sequence's body;  frames HOST int [S], every F_s >= 1;  dfs HOST int [55]: what amuse_bvh_layout wrote;  order: AMUSE_BVH_*, channel list "A B C" meaning
 *   R = R_A R_B R_C;  scale > 0;  euler_out dev fp32 [rows][168] or NULL;  text_out dev bytes [rows][2016] or NULL, 4-byte aligned;  status dev int [S],
 *   cleared by the caller.
 * Columns 0..2 of a row: (root_rest[s] + trans) x scale.  Columns 3 + 3 c ..: joint dfs[c], in fp32 and without a rotation matrix:
 *   unit quaternion (w, q): t = |a|, w = cos(t / 2), q = a sin(t / 2) / t with the factor taken as 1 / 2 - t^2 / 48 where t < 1e-3
 *   for channel axes (i, j, k) and e = the sign of the permutation (k, j, i):  a = w - q_j, b = q_k + e q_i, c = q_j + w, d = e q_i - q_k
 *   middle angle 2 atan2(hypot(c, d), hypot(a, b)) - pi / 2;  hs = atan2(b, a), hd = atan2(d, c);  first angle e (hs + hd), third hs - hd, both wrapped
 *   into [-180, 180) degrees.  At exact gimbal lock the pair that vanishes takes the other's angle, so the third channel is 0.
 * This keeps the ROTATION accurate where the individual angles are ill-conditioned.
 * unwrap != 0: a second launch walks each (sequence, joint) in frame order; at frame t > 0 it weighs (alpha, beta, gamma) against (alpha + 180, 180 - beta,
 * gamma + 180) - the same rotation - each channel moved by the multiple of 360 nearest to the value emitted at t - 1, and keeps the one with the smaller sum of
 * absolute channel differences (ties: the first).  Frame 0 keeps its principal values.
 * euler_out holds exactly the fp32 values that are formatted, and the text is amuse_bvh_format of them.  A sequence's bytes depend on its own rows alone.
 * A sequence with a value that does not fit the field gets status[s] = 1 (and '#' fields).
 * AMUSE_EINVAL before any HIP call: S < 1, an F_s outside 1..(INT_MAX - 256) / 56, an order outside 0..5, dfs not a permutation of 0..54, scale not positive
 * and finite, poses / root_rest / frames / dfs / status NULL, euler_out and text_out both NULL, text_out not 4-byte aligned. */
int amuse_bvh_motion(const float* poses, const float* trans, const float* root_rest, int S, const int* frames, const int* dfs, int order, float scale, int unwrap,
                     float* euler_out, void* text_out, int* status, void* stream);
/* The inverse.  channels dev fp32 [rows][168] as euler_out above;  poses_out dev [rows][55][3], trans_out dev [rows][3].  Degrees -> three axis quaternions
 * multiplied in channel order -> axis-angle by the decode tail's own arithmetic, angle <= pi;  trans = position / scale - root_rest[s].  Same checks. */
int amuse_bvh_decode(const float* channels, int S, const int* frames, const int* dfs, int order, float scale, const float* root_rest, float* poses_out,
                     float* trans_out, void* stream);

/* ------------------------------------------------------------------ sample-rate conversion (csrc/amuse_resample_host.hpp, amuse_resample.hip, k_resample.hip; amuse_amd/resample.py)
 * AN EXTENSION, off by default: the reference never resamples - scripts/trainer.py:520 drops the file's rate and feeds whatever samples it holds to a 16 kHz fbank.
 * The filter is a band-limited, Hann-windowed sinc in polyphase form.  Its constants (6 zero crossings, roll-off 0.99) are a RECOLLECTION of
 * torchaudio.functional.resample's defaults; torchaudio is pinned nowhere in this project, the filter is checked against its own float64 restatement
 * (tests/resample_ref.py) and scipy.signal.upfirdn only.
 *
 * For integer rates r_in -> r_out: g = gcd, M = r_in / g, L = r_out / g, base = 0.99 min(M, L), lpw = 6, Hw = ceil(lpw M / base), K = 2 Hw + 2,
 * n_out = ceil(n_in L / M).  Output sample m, with phase i = m mod L and j0 = floor(m M / L) - Hw (64-bit integers; no index comes from a float):
 *   y[m] = sum over k = 0 .. K - 1, in that order, in fp32, of h[i][k] x[j0 + k]        (x is zero outside 0 .. n_in - 1)
 *   h[i][k] = (base / M) sinc(pi t) cos^2(pi t / (2 lpw)) where |t| < lpw, else 0;  t = base ((floor(i M / L) - Hw + k) / M - i / L);  sinc(0) = 1
 * The bank h is computed once on the host in double and rounded to fp32.  EQUAL rates are the identity: M = L = 1, Hw = 0, K = 1, h = {1}, and the output is
 * the format conversion of channel 0, bitwise.
 *
 * amuse_resample_plan: the plan, stated once; needs no GPU and no context.  *up = L, *down = M, *taps = K, *n_out as above; any output pointer may be NULL.
 * AMUSE_EINVAL for rates outside 4,000..384,000 Hz, for a bank L x K x 4 bytes above 2 MiB (44101 -> 16000 Hz: 16000 phases), for n_in < 1 and for n_in or
 * n_out beyond an int. */
enum { AMUSE_PCM_U8 = 0, AMUSE_PCM_S16 = 1, AMUSE_PCM_S32 = 2, AMUSE_PCM_F32 = 3 };
typedef struct amuse_resampler amuse_resampler;
int amuse_resample_plan(int rate_in, int rate_out, long long n_in, int* up, int* down, int* taps, long long* n_out);
/* One resampler per (GPU, rate pair): builds the bank and uploads it (L x K floats of device memory).  NULL on failure (amuse_last_error). */
amuse_resampler* amuse_resampler_create(int device, int rate_in, int rate_out);
void amuse_resampler_destroy(amuse_resampler* r);
/* One waveform.  pcm dev [n_in][channels]: interleaved frames as a WAV's data chunk holds them, `format` one of AMUSE_PCM_*; CHANNEL 0 ONLY is read (as the
 * front-end and kaldi read it), converted as the WAV loader converts it: U8 (x - 128) / 128, S16 x / 32768, S32 float(x) / 2^31, F32 as it is.
 * out dev fp32 [out_capacity], the first n_out written.  Stream-ordered; allocates nothing, copies nothing, never synchronises: it can be captured.
 * Checked before any HIP call, AMUSE_EINVAL otherwise: what amuse_resample_plan checks; channels in 1..8; a known format; out_capacity >= n_out; pointers non-NULL. */
int amuse_resample(amuse_resampler* r, const void* pcm, int format, int channels, long long n_in, float* out, long long out_capacity, void* stream);
/* tests: the fp32 bank of a rate pair into HOST memory, [up][taps] (sizes from amuse_resample_plan); no GPU needed */
int amuse_debug_resample_bank(int rate_in, int rate_out, float* bank_out_host);

/* ------------------------------------------------------------------ preview rendering (csrc/amuse_render_host.hpp, amuse_render.hip, k_render.hip; amuse_amd/render.py)
 * AN EXTENSION, off by default: the reference hands its NPZ to Blender and ffmpeg; this is a PREVIEW - the posed mesh flat-shaded from one fixed camera -
 * and matches no other renderer's image.  Once the vertices are snapped to the sub-sample grid, coverage and depth are integer arithmetic, so the winning
 * triangle of every sample is a pure function of the snapped vertices (tests/render_ref.py restates it in numpy int64, bit for bit).
 *
 * Camera: x_cam = R x + t (R row-major), looking down +z; u = fx x / z + cx, v = cy - fy y / z; near_z, far_z bound the depth range.
 * Screen record of a vertex, int32 (X, Y, Zq), with ss in {1, 2} the supersampling factor per axis:
 *   X = rint(16 ss u), Y = rint(16 ss v): fp32, round half to even (4 sub-sample bits); the view-space position is fp32 fma chains, t added first
 *   Zq = floor(zndc (2^24 - 1) + 0.5), zndc = far (z - near) / (z (far - near)) - linear in screen space - computed in DOUBLE from the fp32 vertex (with its own
 *        double z): 24 bits of depth do not survive fp32 roundings
 *   invalid - stored as (0, 0, -1) - for z < near, z > far, a non-finite coordinate, or X / Y outside [-32768, 65535] (the guard band).  A caller-made record
 *   (amuse_debug_render_raster) is invalid when Zq is outside 0 .. 2^24 - 1 or X / Y outside the guard band.
 * Triangle t (vertices a, b, c): skipped when a vertex is invalid or the doubled area A2 = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) is 0; b and c are swapped
 * when A2 < 0 (two-sided: no culling).  Sample (sx, sy) has its centre at P = (16 sx + 8, 16 sy + 8).  Edge functions, int64, for the edge p -> q:
 * E(P) = (Xq - Xp)(Py - Yp) - (Yq - Yp)(Px - Xp); w_c = E_ab, w_a = E_bc, w_b = E_ca, w_a + w_b + w_c = A2.  Covered: all three >= 0, and where one is 0 its
 * edge must be a top edge (Yq == Yp, Xq > Xp) or a left edge (Yq < Yp) - the D3D11 top-left rule in a y-down frame.
 *   zpix = (w_a Zq_a + w_b Zq_b + w_c Zq_c) div A2 (floor, int64: A2 < 2^35 inside the guard band, so the numerator stays below 2^59)
 *   key = (zpix << 32) | t;  the sample's winner is the MINIMUM key (nearest, ties to the lower index); an empty sample holds all ones.
 * Shading of a sample, fp32: n = (p_b - p_a) x (p_c - p_a) of the winner's view-space positions, c = ambient + (1 - ambient) |n . l| / |n| (c = ambient when
 * |n| = 0), l the unit light direction; channel = floor(body_rgb c + 0.5); an empty sample is bg_rgb.  ss = 2: pixel = (s00 + s01 + s10 + s11 + 2) >> 2 per
 * channel on the uint8 samples.  Defaults (shading NULL): light (0, 0, -1) - a headlight -, ambient 0.25, body (200, 200, 208), background (32, 32, 36).
 * Limits: width ss and height ss in 1 .. 2048, V >= 1, T >= 1 (an int: below 2^32).
 *
 * amuse_render_plan: the plan, stated once; needs no GPU.  Tiles of 32 x 32 samples: *tiles_x = ceil(width ss / 32), *tiles_y = ceil(height ss / 32).  A call's
 * frames are processed *chunk_frames at a time: min(frames, 256, max(1, floor(16 MiB / (24 V)))); *workspace_bytes = the records and view positions of one chunk
 * (2 x chunk_frames x 12 V bytes, each rounded up to 256).  Any output pointer may be NULL. */
typedef struct amuse_renderer amuse_renderer;
typedef struct { float R[9], t[3], fx, fy, cx, cy, near_z, far_z; } amuse_camera;
typedef struct { float light[3], ambient; unsigned char body_rgb[3], bg_rgb[3]; } amuse_shading;
int amuse_render_plan(int width, int height, int ss, int V, int T, int frames, int* tiles_x, int* tiles_y, int* chunk_frames, size_t* workspace_bytes);
/* One renderer per (GPU, mesh topology, image size): uploads the faces (host int [T][3], every index in 0 .. V - 1).  NULL on failure (amuse_last_error). */
amuse_renderer* amuse_renderer_create(int device, const int* faces, int T, int V, int width, int height, int ss);
void amuse_renderer_destroy(amuse_renderer* r);
/* M frames.  vertices dev [M][V][3] (amuse_body_forward's vertices_out, flattened over clips); rgb_out dev uint8 [M][height][width][3]; keys_out (nullable) dev
 * [M][height ss][width ss] the winning keys; screen_out (nullable) dev int [M][V][3] the screen records.  shading NULL = the defaults above.
 * The workspace follows amuse_body_reserve's rules: sized on first use, grows only, nothing freed before destroy; after the first call of a given M (beyond
 * chunk_frames all sizes are one) a call is stream-ordered, allocates nothing and synchronises nothing.  One workspace per renderer: its calls must not overlap
 * on two streams.  Bitwise reproducible: no float atomics, the minimum of packed integers does not depend on arrival order.
 * Checked before any HIP call, AMUSE_EINVAL otherwise: r, vertices, camera, rgb_out non-NULL; M >= 1; 0 < near_z < far_z and every camera number finite;
 * a light direction of non-zero finite length and 0 <= ambient <= 1 when shading is given. */
int amuse_render(amuse_renderer* r, const float* vertices_dev, int M, const amuse_camera* camera, const amuse_shading* shading, unsigned char* rgb_out_dev,
                 unsigned long long* keys_out_dev, int* screen_out_dev, void* stream);
/* tests: the raster stage alone, from caller-made screen records dev int [M][V][3]: keys only, dev [M][height ss][width ss].  Uses no workspace. */
int amuse_debug_render_raster(amuse_renderer* r, const int* screen_dev, int M, unsigned long long* keys_out_dev, void* stream);

/* ------------------------------------------------------------------ motion metrics (csrc/amuse_motion_metrics_host.hpp, amuse_motion_metrics.hip, k_motion_metrics.hip; amuse_amd/motion_metrics.py)
 * AN EXTENSION, off by default: the reference states the intent (models/latent_diffusion/utils/val_metrics.py ComputeMetrics: APE / AVE on joints) in a file
 * that cannot run - torchmetrics is absent and its helpers are defined nowhere - and passes metricsmodel=None.  The variance below is a RECOLLECTION of MLD's
 * variance(x, T, dim=0), pinned only against its own float64 restatement (tests/motion_metrics_ref.py).  The velocity / acceleration sums are this project's
 * addition: val_metrics.py has no jitter measure.
 *
 * Per clip n with L = lengths_dev[n] frames, G / R the generated / reference joints [F][55][3] as amuse_body_forward writes joints_out (metres, y up), root =
 * joint 0, traj = components (0, 2) of the root, local[f][j] = X[f][j] - X[f][0].  ONLY frames f < L are read into any result; frames at or beyond L may hold
 * anything, NaN included.  var(x) = sum_f (x_f - mean)^2 / (L - 1) per coordinate, two-pass (the mean first, then the deviations).  |.| is the L2 norm.
 * One row of amuse_motion_metrics_row() = 442 doubles per clip:
 *   offset  length  block
 *        0       1  ape_root    sum_{f<L} |G[f][0] - R[f][0]|
 *        1       1  ape_traj    the same on traj (2 components)
 *        2      54  ape_pose    sum_f |local_G[f][j] - local_R[f][j]|, j = 1..54
 *       56      55  ape_joints  sum_f |G[f][j] - R[f][j]|, j = 0..54
 *      111       1  ave_root    |var(G[:][0]) - var(R[:][0])| (3 components)
 *      112       1  ave_traj    the same on traj
 *      113      54  ave_pose    |var(local_G[:][j]) - var(local_R[:][j])|, j = 1..54
 *      167      55  ave_joints  |var(G[:][j]) - var(R[:][j])|
 *      222      55  vel_gen     sum_{f=1}^{L-1} |G[f][j] - G[f-1][j]|
 *      277      55  vel_ref     the same on R
 *      332      55  acc_gen     sum_{f=1}^{L-2} |G[f+1][j] - 2 G[f][j] + G[f-1][j]| (0 when L = 2)
 *      387      55  acc_ref     the same on R
 * Inputs are fp32; every operation after the load is double.  One workgroup per clip, no atomics; the order of every sum depends on L alone, so a clip's row
 * does not depend on N or on the clip's position in the batch: same clip, same bits.
 * Context-free and stream-ordered; no allocation, no copy, no host synchronisation: it can be captured.
 * Checked before any HIP call, AMUSE_EINVAL otherwise: every pointer non-NULL; N >= 1; F >= 2; N F and 442 N within an int.
 * The lengths live on the DEVICE - the host cannot see them without a synchronisation - so they are checked there: a clip whose length lies outside 2..F gets
 * a row of 442 NaN, reads nothing and harms no other clip. */
int amuse_motion_metrics_row(void);
int amuse_motion_metrics(const float* joints_gen, const float* joints_ref, const int* lengths_dev, int N, int F, double* rows_out, void* stream);

/* ------------------------------------------------------------------ beat alignment (csrc/amuse_beat_host.hpp, amuse_beat.hip, k_beat.hip; amuse_amd/beat_align.py)
 * AN EXTENSION, off by default: the reference has no such measure.  Speech onsets of the 16 kHz waveform against the motion beats of every SMPL-X joint, scored by
 * how close the two sets lie in time.  This is THIS PROJECT'S OWN statement of the metric, in the manner of BEAT's `alignment` and of librosa's spectral-flux
 * onset detector, both written down from memory: neither is on the build machine, nothing here is pinned against either, and no number this code gives has been
 * compared with librosa or with BEAT's own code.  It is checked against its own float64 restatement (tests/beat_ref.py) and, for the motion beats, against
 * scipy.signal.argrelextrema.  Deviation stated: a frame's time is its window CENTRE (audio) and the middle of the two motion frames a speed is taken between.
 *
 * Definitions (csrc/amuse_beat_host.hpp restates the row offsets; the kernels and tests/beat_ref.py follow these):
 *   log-mel   S[t][m]: the kaldi fbank log energy of amuse_audio_fbank BEFORE its normalisation, same tables (mel [128][257], window [400]): frame t covers
 *             the samples [160 t, 160 t + 400): DC removal, pre-emphasis 0.97, window, 512-point FFT, floor 1.1920929e-07, natural log.
 *             T = 0 if n < 400, else 1 + (n - 400) / 160   (amuse_beat_plan)
 *   envelope  e[0] = 0;  e[t] = (1 / 128) sum_m max(0, S[t][m] - S[t-1][m]), fp32
 *   onsets    double after the fp32 load, no division by the maximum.  M = max_t e[t] over the clip's valid frames; M <= 0: no onset.  Frame t is an onset iff
 *               1. e[t] >  e[t-i] for i = 1..onset_window with t - i >= 0        (strict on the left,
 *               2. e[t] >= e[t+i] for i = 1..onset_window with t + i < T          not on the right: a plateau gives its FIRST frame)
 *               3. e[t] >= mean(e[max(0, t-a) .. min(T-1, t+a)]) + onset_delta M, a = onset_avg_window; the mean is the ascending sum over the count
 *             Two onsets are therefore more than onset_window frames apart; no greedy pass.  Onset time tau_a = (160 t + 200) / 16000 s.
 *   beats     joint j, f = 0..L-2: s_j[f] = |X[f+1][j] - X[f][j]| fps, double after the fp32 load.  f is a beat iff s[f] < s[clip(f +- i, 0, L-2)] for all
 *             i = 1..motion_order (strict; an index that clips onto f itself fails): scipy.signal.argrelextrema(s, np.less, order) in its default clip mode.
 *             Beat time tau_m = (f + 0.5) / fps.
 * One row of amuse_beat_align_row() = 166 doubles per clip:
 *   offset  length  block
 *        0       1  n_onsets   onsets with tau_a <= (L - 1) / fps; later ones are dropped everywhere
 *        1      55  n_beats    motion beats of joint j
 *       56      55  a2m        sum_a exp(-min_m (tau_a - tau_m)^2 / (2 sigma_s^2)); 0 when joint j has no beat
 *      111      55  m2a        sum_m exp(-min_a (tau_m - tau_a)^2 / (2 sigma_s^2)); 0 when there is no onset
 * Sums run in ascending time, in double (exp included), one lane per joint: no atomics, the order depends on the clip alone, so the same clip gives the same
 * bits at any N and any position in the batch.  Only frames f < L are read; frames at or beyond L may hold NaN.
 *
 * Parameters: amuse_beat_default_params fills sigma_s 0.1 s, onset_delta 0.07, onset_window 3 and onset_avg_window 10 (frames of 10 ms), motion_order 3
 * (motion frames), fps 30.  A NULL params pointer means the defaults.  Checked on the host, AMUSE_EINVAL otherwise: sigma_s > 0 and finite; onset_delta >= 0
 * (and finite); both onset windows >= 1; 1 <= motion_order <= 32 (the speeds a lane keeps); fps > 0 and finite.
 *
 * Every call below is stream-ordered, makes no host synchronisation and checks its arguments before any HIP call. */
typedef struct amuse_beat amuse_beat;
typedef struct { double sigma_s, onset_delta; int onset_window, onset_avg_window, motion_order; double fps; } amuse_beat_params;
int amuse_beat_default_params(amuse_beat_params* params);
/* The context owns the two tables on the device (host arrays mel_banks [128][257], window [400], as amuse_audio_create takes them).  NULL on failure. */
amuse_beat* amuse_beat_create(int device, const float* mel_banks, const float* window);
void amuse_beat_destroy(amuse_beat* ctx);
/* *frames = T as above; needs no GPU.  AMUSE_EINVAL for n_samples < 0 or a T beyond an int. */
int amuse_beat_plan(long long n_samples, int* frames);
/* Only for amuse_beat_onsets with envelope_out == NULL: makes the context's own envelope buffer hold B clips of n_samples.  Grows only; what an earlier call
 * may still read is freed at destroy, never before.  This is the one call here that allocates. */
int amuse_beat_reserve(amuse_beat* ctx, int B, int n_samples);
/* waves_dev [B][n_samples]; n_valid_dev [B] or NULL (every clip has n_samples; a value is clamped to 0..n_samples) for ragged batches: clip b has
 * T_b = plan(n_valid[b]) frames.  envelope_out [B][T], onset_mask_out [B][T] (1 = onset), T = plan(n_samples); either may be NULL, not both; with envelope_out
 * NULL the envelope goes to the reserved buffer (AMUSE_EINVAL if amuse_beat_reserve has not covered B x T).  Frames beyond T_b get envelope 0 and mask 0.
 * Two launches: the envelope (one workgroup per run of 16 frames, no [T][128] intermediate) and exactly the stage of amuse_beat_pick.  T == 0 launches nothing.
 * AMUSE_EINVAL: NULL ctx / waves; B < 1; n_samples < 1; B x max(T, 1) beyond an int; bad params. */
int amuse_beat_onsets(amuse_beat* ctx, const float* waves_dev, const int* n_valid_dev, int n_samples, int B, const amuse_beat_params* params,
                      float* envelope_out, unsigned char* onset_mask_out, void* stream);
/* Context-free: the pick stage alone on a caller's envelope dev [B][T]; frames_dev [B] (clamped to 0..T).  AMUSE_EINVAL: a NULL pointer; B < 1; T < 1;
 * B x T beyond an int; bad params. */
int amuse_beat_pick(const float* envelope_dev, const int* frames_dev, int B, int T, const amuse_beat_params* params, unsigned char* onset_mask_out, void* stream);
int amuse_beat_align_row(void);
/* Context-free.  onset_mask_dev [N][T] (non-zero = onset), audio_frames_dev [N] (clamped to 0..T); joints dev [N][F][55][3] as amuse_body_forward writes them;
 * lengths_dev [N]; rows_out dev [N][166]; beat_mask_out dev [N][F][55] or NULL (1 = beat; 0 at every frame that cannot be one).  A clip whose length lies
 * outside 2..F gets a row of NaN (and a beat mask of 0), reads nothing and harms no other clip.  One workgroup per clip.
 * AMUSE_EINVAL: a NULL pointer other than beat_mask_out (onset_mask_dev may be NULL when T == 0); N < 1; F < 2; T < 0 or T > 131072 (the onset bits a
 * workgroup keeps in LDS: 21 minutes of audio); N x F, N x T or 166 N beyond an int; bad params. */
int amuse_beat_align(const unsigned char* onset_mask_dev, const int* audio_frames_dev, int T, const float* joints, const int* lengths_dev, int N, int F,
                     const amuse_beat_params* params, double* rows_out, unsigned char* beat_mask_out, void* stream);

/* ------------------------------------------------------------------ preview video (csrc/amuse_mjpeg_host.hpp, amuse_mjpeg.hip, k_mjpeg.hip; amuse_amd/video.py)
 * AN EXTENSION, off by default: the reference muxes its Blender frames with ffmpeg; this encodes the preview renderer's frames, still on the device, as
 * baseline JPEG files for a Motion-JPEG AVI.  A PREVIEW encoder: fixed Huffman tables, no chroma subsampling; compared with libjpeg through PIL only
 * (tests/mjpeg_ref.py restates it), and no player has been run against it in a test.
 *
 * Format: baseline sequential DCT (SOF0), 8 bit, components Y Cb Cr with H = V = 1, interleaved in one scan; one MCU = one 8 x 8 block per component in the
 * order Y, Cb, Cr.  Segments in order: SOI, APP0 (JFIF 1.01, aspect 1:1), DQT luma, DQT chroma, SOF0 (true width and height), DHT DC luma, AC luma, DC chroma,
 * AC chroma (ITU-T T.81 Annex K.3), DRI, SOS, entropy data, EOI.  Restart interval = one MCU row, Ri = ceil(width / 8); interval k >= 1 is preceded by RSTm,
 * m = (k - 1) mod 8; DC predictors are 0 at the start of an interval; an interval is padded to a byte with 1-bits; a data byte 0xFF is followed by 0x00.
 * Tables from quality by libjpeg's rule on Annex K.1 / K.2: s = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((base s + 50) / 100, 1, 255), integers.
 * Arithmetic, fp32: Y = 0.299 R + 0.587 G + 0.114 B - 128, Cb = -0.168735892 R - 0.331264108 G + 0.5 B, Cr = 0.5 R - 0.418687589 G - 0.081312411 B, not
 * rounded; a width or height that is no multiple of 8 repeats the last column / row; F = orthonormal 8 x 8 DCT-II; coefficient = F / t rounded half away from
 * zero, DC clamped to [-1024, 1023], AC to [-1023, 1023].  The entropy coding is a pure function of the coefficients and is bit exact: DC difference against
 * the previous block of the component inside the interval, category + magnitude bits; AC run / size with ZRL (0xF0) per 16 zeros; EOB unless coefficient 63 is
 * non-zero.
 *
 * amuse_mjpeg_tables: host only; the two tables of a quality in natural (row-major) order.
 * amuse_mjpeg_plan: host only; *mcus_x = ceil(width / 8), *mcus_y = ceil(height / 8), *header_bytes = SOI .. SOS (629), *workspace_bytes = what
 * amuse_mjpeg_reserve(frames) allocates (the coefficients, 384 bytes per MCU, and 8 bytes per interval + 4 per frame of sizes and offsets, each section rounded
 * up to 256), *worst_case_bytes_per_frame = header + mcus_y x 2 ceil(mcus_x x 3 x 1660 / 8) + 2 (mcus_y - 1) + 2 (every block at its 1660-bit maximum, every
 * byte stuffed): about 1.2 KB per MCU, which is why a call reserves no worst-case slots.  Any output pointer may be NULL. */
typedef struct amuse_mjpeg amuse_mjpeg;
int amuse_mjpeg_tables(int quality, unsigned char* luma_q64, unsigned char* chroma_q64);
int amuse_mjpeg_plan(int width, int height, int frames, int* mcus_x, int* mcus_y, int* header_bytes, size_t* workspace_bytes, size_t* worst_case_bytes_per_frame);
/* One encoder per (GPU, image size, quality): uploads the header, the Huffman words and the divisors.  NULL on failure (amuse_last_error). */
amuse_mjpeg* amuse_mjpeg_create(int device, int width, int height, int quality);
/* Makes the workspace hold calls of up to `frames` frames.  Grows only; an outgrown block is freed at destroy, never before.  With create, the only call here
 * that allocates. */
int amuse_mjpeg_reserve(amuse_mjpeg* e, int frames);
void amuse_mjpeg_destroy(amuse_mjpeg* e);
/* M frames, rgb dev uint8 [M][height][width][3] (amuse_render's rgb_out).  The frames come out back to back in out_dev, each a complete file SOI .. EOI;
 * offsets_dev [M], sizes_dev [M] and *total_dev (the sum of the sizes) are written whatever out_capacity is.  NO BYTE IS WRITTEN AT OR BEYOND out_capacity,
 * whatever the input: every store is checked.  A frame with offset + size <= out_capacity is complete; any other is not, and total_dev > out_capacity says so:
 * call again with total bytes.  The same frame gives the same bytes alone, at any position of any batch, on any run: sizes become offsets by sums in a fixed
 * order, no atomics.  Stream-ordered, allocates nothing, never synchronises (capture into a graph has not been tested).  One workspace per encoder: its calls must not overlap on two
 * streams.  Checked before any HIP call, AMUSE_EINVAL otherwise: width and height 1..4096, quality 1..100 (create); every pointer non-NULL; M >= 1 and within
 * the frames reserved; the launches' block counts within an int. */
int amuse_mjpeg_encode(amuse_mjpeg* e, const unsigned char* rgb_dev, int M, unsigned char* out_dev, size_t out_capacity, unsigned long long* offsets_dev,
                       unsigned int* sizes_dev, unsigned long long* total_dev, void* stream);
/* tests: the transform alone; coef dev int16 [M][mcus_y][mcus_x][3][64], every block in zigzag order.  Uses no workspace. */
int amuse_debug_mjpeg_coefficients(amuse_mjpeg* e, const unsigned char* rgb_dev, int M, short* coef_dev, void* stream);
/* tests: the header (SOI .. SOS) of a size and quality into HOST memory; *bytes = its length, copied only when capacity holds it.  No GPU needed. */
int amuse_debug_mjpeg_header(int width, int height, int quality, unsigned char* out_host, size_t capacity, int* bytes);

#ifdef __cplusplus
}
#endif
#endif /* AMUSE_HIP_H */
