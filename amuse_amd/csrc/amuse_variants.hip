// Denoiser variants (reference models/latent_diffusion/denoiser.py:64-66,92-131,174-204): host side - state-dict index, weight
// streams, hoisted tables, launch sequences.  Kernels: k_sampler_dec.hip (arch "trans_dec", latent sample: persistent T-step kernel),
// k_vae.hip M_DEN_E / M_DEN_D (diffusion_only: one step = the staged rows / attention kernels at S = 304 / 300), k_misc.hip prologues.
#include "amuse_pack.hpp"
#include "amuse_variants.hpp"

struct amuse_variant {
    // arch DEC: [4 waves][units + kRing][64] per precision (PREC_* index)
    uint4* dec_w[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t dec_units[4] = {0, 0, 0, 0};
    // pose-space archs: the step's network.  ENC_POSE (diffusion_only + trans_enc) is a skip network with every stream - rows8: stages 1..8 (k_vae_rows8.hip, ENC form),
    // fusedx / fused16: the whole step as one stream for k_den_fusedx / k_den_fused; DEC_POSE has the staged streams only.  emb_bias / final_bias: pose_embd.bias,
    // pose_proj.bias; pe: the context's query_pos table.  Every arch: net.pvec, PV_* (ENC_POSE) / PVX_* (trans_dec archs) layout
    RowNet net;
    float* m_pe = nullptr;           // mem_pos.pe [500][128]
    float *wkv_t = nullptr, *bkv = nullptr;       // trans_dec: cross-attention k / v projections [9][2][128 in][128 out], [9][2][128]
    float* tkv_sched = nullptr;      // [AMUSE_MAX_STEPS][9][2][128]: K / V of the time memory token per step of the schedule
    // workspaces
    float* ckv = nullptr; size_t ckv_cap = 0;     // [B][ncond][9][2][128]
    float* tkv1 = nullptr; size_t tkv1_cap = 0;   // teacher-forced steps: [1 or B][9][2][128]
    float* ws = nullptr; size_t ws_cap = 0;       // pose stages: x, q, k, v, o, 4 skip levels of [B][304][128]
    uint4* skip = nullptr; size_t skip_cap = 0;   // ENC_POSE: the fused step kernel's (k_den_fused.hip) skip stack, clips
    float* tt = nullptr; size_t tt_cap = 0;       // teacher-forced steps: time tokens [1 or B][128] | device copy of the timesteps
};

namespace {
constexpr int kTkv = kLayers * 2 * kD;        // floats of one token's K / V over the nine layers
constexpr int kPoseRowsMax = kFrames + 4;
constexpr size_t kPoseWsPerClip = (size_t)kPoseRowsMax * kD * (1 + 3 + 1 + 4);
constexpr int kPoseChunk = 256;

bool arch_dec(int arch) { return arch & 1; }
bool arch_pose(int arch) { return arch & 2; }

ParamIndex variant_index(int arch) {
    ParamIndex P;
    if (arch_pose(arch)) {
        P.add("pose_embd.weight", 128 * kFeats); P.add("pose_embd.bias", 128);
        P.add("pose_proj.weight", kFeats * 128); P.add("pose_proj.bias", kFeats);
    }
    P.add("time_embedding.linear_1.weight", 128 * 256); P.add("time_embedding.linear_1.bias", 128);
    P.add("time_embedding.linear_2.weight", 128 * 128); P.add("time_embedding.linear_2.bias", 128);
    for (const char* n : {"con", "emo", "sty"}) {
        P.add(std::string("emb_proj_") + n + ".1.weight", 128 * 256);
        P.add(std::string("emb_proj_") + n + ".1.bias", 128);
    }
    P.add("query_pos.pe", 500 * 128); P.add("mem_pos.pe", 500 * 128);
    if (arch_dec(arch)) {   // TransformerDecoder: layers, then norm (cross_attention.py:195-203)
        for (int i = 0; i < kLayers; ++i) dec_layer(P, "decoder.layers." + std::to_string(i));
        P.add("decoder.norm.weight", 128); P.add("decoder.norm.bias", 128);
    } else {
        skip_stack(P, "encoder", false);
    }
    return P;
}
const ParamIndex& index_of(int arch) {
    static const ParamIndex idx[4] = {variant_index(0), variant_index(1), variant_index(2), variant_index(3)};
    return idx[arch & 3];
}
std::string dec_name(int l) { return "decoder.layers." + std::to_string(l); }

// PVX_* parameter vector of the nine TransformerDecoderLayers + decoder.norm
std::vector<float> build_pvec_dec(const Params& P) {
    std::vector<float> pv(PVX_TOTAL, 0.f);
    for (int l = 0; l < kLayers; ++l) {
        float* b = pv.data() + l * PVX_BLOCK;
        const std::string p = dec_name(l);
        fill_block_pvec(b, P, p, true);
        memcpy(b + PVX_CQ_B, P.get(p + ".multihead_attn.in_proj_bias"), 128 * 4);
        memcpy(b + PVX_CO_B, P.get(p + ".multihead_attn.out_proj.bias"), 128 * 4);
    }
    memcpy(pv.data() + PVX_FINAL_W, P.get("decoder.norm.weight"), 128 * 4);
    memcpy(pv.data() + PVX_FINAL_B, P.get("decoder.norm.bias"), 128 * 4);
    return pv;
}

// wave w's units of one decoder layer behind its self-attention, in consumption order (k_sampler_dec.hip decoder_layer;
// k_vae.hip M_DEN_D stage): [self v (latent archs) |] self out_proj slice, cross q, cross out_proj slice, linear1, linear2
void pack_dec_layer(std::vector<uint4>& s, int prec, const Params& P, int l, int w, bool self_value_path) {
    const std::string p = dec_name(l);
    if (self_value_path) pack_gemm(s, prec, P.get(p + ".self_attn.in_proj_weight"), 384, 128, {16 + 2 * w, 16 + 2 * w + 1}, range(0, 8));
    pack_gemm(s, prec, P.get(p + ".self_attn.out_proj.weight"), 128, 128, range(0, 8), {2 * w, 2 * w + 1});
    pack_gemm(s, prec, P.get(p + ".multihead_attn.in_proj_weight"), 384, 128, {2 * w, 2 * w + 1}, range(0, 8));
    pack_gemm(s, prec, P.get(p + ".multihead_attn.out_proj.weight"), 128, 128, range(0, 8), {2 * w, 2 * w + 1});
    pack_gemm(s, prec, P.get(p + ".linear1.weight"), 512, 128, range(8 * w, 8 * w + 8), range(0, 8));
    pack_gemm(s, prec, P.get(p + ".linear2.weight"), 128, 512, range(0, 8), range(8 * w, 8 * w + 8));
}

// condition tokens (+ positions) into c->cond_tok [B][ncond][128]; trans_dec archs: their K / V into v->ckv
int variant_cond(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int* ncond_out, hipStream_t st) {
    amuse_variant* v = c->var;
    CondArgs ca{};
    int n = 0;
    const float* zs[3] = {con, emo, sty};
    for (int i = 0; i < 3; ++i)
        if (zs[i]) { ca.z[n] = zs[i]; ca.wt[n] = c->cond_wt[i]; ca.bias[n] = c->cond_b[i]; ++n; }
    if (int e = ensure(&c->cond_tok, &c->cond_cap, (size_t)B * 3 * kD)) return e;
    // emb_latent = cat(time, con, emo, sty): positions 1.. of query_pos (diffusion_only + trans_enc, denoiser.py:180-181) or of
    // mem_pos (trans_dec, denoiser.py:194)
    ca.pe = arch_dec(c->arch) ? v->m_pe : c->den_pe;
    ca.pe_base = 1;
    ca.out = c->cond_tok; ca.B = B; ca.ncond = n;
    HIP_TRY(launch_cond_tokens(ca, st));
    if (arch_dec(c->arch)) {
        if (int e = ensure(&v->ckv, &v->ckv_cap, (size_t)B * 3 * kTkv)) return e;
        HIP_TRY(launch_mem_kv(c->cond_tok, B * n, v->wkv_t, v->bkv, v->ckv, st));
    }
    *ncond_out = n;
    return 0;
}
const float* time_pe_row(const amuse_ctx* c) { return arch_dec(c->arch) ? c->var->m_pe : c->den_pe; }   // position 0 of the token's table

// one denoising step of a pose-space variant on clips [0, nb) of the given arrays: ten row stages, nine attention launches
struct PoseStep {
    const float* x_in; float* x_out; float* eps_out; const float* coef; const float* step_noise;
    const float* ttok; size_t ttok_stride; const float* tkv; size_t tkv_clip_stride;
    const float* cond_tok; const float* ckv; const int* lengths_dev;
    int ncond, step; uint64_t seed, clip0;
    bool rows8;   // fp32x staged step: stages 1..8 on k_vae_rows8x (decided from the CALL's clip count)
    bool fusedx;  // ... or, where the call's clips fill rounds of the chip, the whole step as ONE per-clip kernel (k_den_fusedx)
};
// kernels of one pose-space Denoiser step: the pin (amuse_set_decode_path) or the plan (amuse_host.hpp plan_step_path), keyed by the CALL's clip count: the fused
// per-clip step kernel of the 16-bit modes (k_den_fused.hip), fp32x's row kernel without split-K for the staged step's stages 1..8 (FUSED) and its per-clip kernel
// (k_den_fusedx, CLIP) where the clips fill rounds of the chip - AMUSE_ARCH_ENC_POSE only; everything else is staged
int step_path_of(amuse_ctx* c, int precision, int B) {
    int path = resolve_path(c->decode_path, plan_step_path(c->arch, precision, B), precision);
    if (c->arch != AMUSE_ARCH_ENC_POSE) path = AMUSE_DECODE_STAGED;
    if (path == AMUSE_DECODE_CLIP && !c->var->net.fusedx) path = AMUSE_DECODE_FUSED;
    if (path == AMUSE_DECODE_FUSED && precision == PREC_F16X2 && !c->var->net.rows8) path = AMUSE_DECODE_STAGED;
    return c->last_plan[3] = path;
}

int pose_step(amuse_ctx* c, const PoseStep& p, int nb, int precision, bool fused, hipStream_t st) {
    amuse_variant* v = c->var;
    const RowNet& n = v->net;
    const bool dec = arch_dec(c->arch);
    if (fused) {
        DenFusedArgs fa{};
        fa.wstream = n.fused16[precision == PREC_F16]; fa.pvec = n.pvec; fa.final_bias = n.final_bias; fa.emb_bias = n.emb_bias;
        fa.pe = n.pe; fa.ttok = p.ttok; fa.ttok_stride = p.ttok_stride; fa.ctok = p.cond_tok; fa.skip = v->skip;
        fa.eps_out = p.eps_out; fa.coef = p.coef; fa.step_noise = p.step_noise; fa.lengths = p.lengths_dev;
        fa.seed = p.seed; fa.clip0 = p.clip0; fa.step = p.step; fa.B = nb; fa.npre = 1 + p.ncond;
        fa.ablate_attention = c->ablate & 1;
        // the kernel updates its state array in place; a teacher-forced step (no coefficients) only reads it
        if (p.x_out && p.x_out != p.x_in) HIP_TRY(hipMemcpyAsync(p.x_out, p.x_in, (size_t)nb * AMUSE_POSE_STATE * sizeof(float), hipMemcpyDeviceToDevice, st));
        fa.x = p.x_out ? p.x_out : const_cast<float*>(p.x_in);
        HIP_TRY(precision == PREC_F16 ? launch_den_fusedh(fa, st) : launch_den_fused(fa, st));
        return 0;
    }
    const int npre = dec ? 0 : 1 + p.ncond, S = kFrames + npre;
    const StageWs w = carve_stage_ws(v->ws, (size_t)nb * S);
    if (p.rows8 && p.fusedx && n.fusedx) {   // the whole step as one persistent workgroup per clip (its scratch: this path's attn_o and skip arrays)
        DenFusedXArgs fx{};
        fx.wstream = n.fusedx; fx.pvec = n.pvec; fx.emb_bias = n.emb_bias; fx.final_bias = n.final_bias; fx.pe = n.pe;
        fx.ttok = p.ttok; fx.ttok_stride = p.ttok_stride; fx.ctok = p.cond_tok;
        fx.x_in = p.x_in; fx.x_out = p.x_out; fx.eps_out = p.eps_out; fx.coef = p.coef; fx.step_noise = p.step_noise; fx.lengths = p.lengths_dev;
        fx.obuf = w.attn_o; fx.skip = w.skip; fx.seed = p.seed; fx.clip0 = p.clip0; fx.step = p.step; fx.B = nb; fx.S = S; fx.npre = npre;
        HIP_TRY(launch_den_fusedx(fx, st));
        return 0;
    }
    StageArgs a = stage_args(n, precision, w, nb);
    VaeRowsArgs& ra = a.rows;
    ra.lengths = p.lengths_dev;   // (the frames' eps rows; the attention sees every row)
    ra.enc_feats = p.x_in; ra.feats_out = p.eps_out; ra.x_out = p.x_out; ra.coef = p.coef; ra.step_noise = p.step_noise;
    ra.seed = p.seed; ra.clip0 = p.clip0; ra.step = p.step;
    ra.S = a.attn.S = S; ra.npre = npre;
    ra.pre_tok_t = p.ttok; ra.pre_tok_t_stride = p.ttok_stride; ra.pre_tok_c = p.cond_tok;
    ra.mem = MemKV{p.tkv, p.tkv_clip_stride, p.ckv, p.ncond};
    // (fp32x, trans_enc: stages 1..8 are plain encoder-layer stages - the row kernel without split-K, as MotionPrior.encode's)
    twin_rows8(a, n, p.rows8);
    return run_stages(a, precision, {dec ? VAE_MODE_DEN_D : VAE_MODE_DEN_E, 0, 1, p.rows8 ? 8 : 0, VAE_MODE_ENC, false}, st);
}
int ensure_pose_ws(amuse_variant* v, int chunk, bool fused) {
    if (fused) return ensure(&v->skip, &v->skip_cap, (size_t)chunk, (size_t)chunk * (kVaeFusedSkipBytesPerClip / sizeof(uint4)));
    return ensure(&v->ws, &v->ws_cap, (size_t)chunk * kPoseWsPerClip);
}
// which kernels the steps of a call take and how its clips are chunked (step_path_of: from the CALL's clip count)
struct PoseRun { bool fused, rows8, fusedx; int chunk; };
PoseRun pose_run_of(amuse_ctx* c, int precision, int B) {
    const int spath = step_path_of(c, precision, B);
    PoseRun r;
    r.fused = is_op16(precision) && spath != AMUSE_DECODE_STAGED;        // k_den_fused
    r.rows8 = precision == PREC_F16X2 && spath != AMUSE_DECODE_STAGED;   // k_vae_rows8x<ENC> for stages 1..8
    r.fusedx = precision == PREC_F16X2 && spath == AMUSE_DECODE_CLIP;    // k_den_fusedx
    r.chunk = r.fused ? B : (B < kPoseChunk ? B : kPoseChunk);
    return r;
}
}  // namespace

size_t variant_param_count(int arch) {
    if (arch < 0 || arch > 3) return 0;
    return index_of(arch).total;
}

int variant_build(amuse_ctx* c, const float* den, int what) {
    if (!c->var) c->var = new amuse_variant();
    amuse_variant* v = c->var;
    const int arch = c->arch;
    const Params D{index_of(arch), den};
    const bool dec = arch_dec(arch), pose = arch_pose(arch);
    if (!pose) {   // arch DEC: the persistent kernel's per-wave ring streams (pack_ring4_stream), one pass over the nine layers per step
        for (int prec = 0; prec < 4; ++prec) {
            if (!(what & kUpdBit[prec])) continue;
            std::vector<uint4> all;
            const auto pass = [&](std::vector<uint4>& s, int w) {
                for (int l = 0; l < kLayers; ++l) pack_dec_layer(s, prec, D, l, w, true);
            };
            if (int e = pack_ring4_stream(all, &v->dec_units[prec], pass)) return e;
            if (v->dec_units[prec] % kRing) return fail(AMUSE_ESTATE, "internal: a trans_dec step is not whole ring revolutions");
            if (upload(c, &v->dec_w[prec], all.data(), all.size() * sizeof(uint4), prec, kUpdBit[prec])) return AMUSE_EHIP;
        }
    } else {
        const float *w_emb = D.get("pose_embd.weight"), *w_proj = D.get("pose_proj.weight");
        RowNet& n = v->net;
        if (!dec) {
            // trans_enc: a skip network with pose_embd in front of stage 0 and pose_proj behind stage 9.  Stages 1..8 on the row kernel without split-K (pose_embd /
            // pose_proj + update stay with k_vae_rows); the whole step as one per-clip stream for k_den_fusedx and, 16-bit, for k_den_fused
            if (int e = build_rownet_streams(c, n, D, {"encoder", w_emb, w_proj, 1, 8, true, 0}, what)) return e;
        } else {
            // trans_dec, staged streams only (pack_staged_stream): between pose_embd and pose_proj, stage i + 1 holds what follows decoder layer i's self-attention
            // (pack_dec_layer) + in_proj(i + 1)
            for (int prec = 0; prec < 4; ++prec) {
                if (!(what & kUpdBit[prec])) continue;
                std::vector<uint4> all;
                const auto content = [&](std::vector<uint4>& s, int st, int w) {
                    if (st == 0) pack_in_matrix_wave(s, prec, w_emb, w);
                    if (st >= 1) pack_dec_layer(s, prec, D, st - 1, w, false);
                    if (st < 9) pack_qkv(s, prec, D.get(dec_name(st) + ".self_attn.in_proj_weight"), w, false);
                    if (st == 9) pack_out_matrix_wave(s, prec, w_proj, w);
                };
                if (int e = pack_staged_stream(all, n.stage_base[prec], n.stage_units[prec], content)) return e;
                if (upload(c, &n.staged[prec], all.data(), all.size() * sizeof(uint4), prec, kUpdBit[prec])) return AMUSE_EHIP;
            }
        }
        std::vector<float> fb(16 * kFeatTiles, 0.f);
        memcpy(fb.data(), D.get("pose_proj.bias"), kFeats * 4);
        if (upload(c, &n.final_bias, fb.data(), fb.size() * 4) || upload(c, &n.emb_bias, D.get("pose_embd.bias"), 128 * 4)) return AMUSE_EHIP;
    }
    {
        const std::vector<float> pv = dec ? build_pvec_dec(D) : build_pvec(D, "encoder", false);
        if (upload(c, &v->net.pvec, pv.data(), pv.size() * 4)) return AMUSE_EHIP;
    }
    if (dec) {
        std::vector<float> wkv((size_t)kLayers * 2 * kD * kD), bkv((size_t)kLayers * 2 * kD);
        for (int l = 0; l < kLayers; ++l)
            for (int kvi = 0; kvi < 2; ++kvi) {
                const std::string p = dec_name(l) + ".multihead_attn";
                const auto t = transpose(D.get(p + ".in_proj_weight") + (size_t)(1 + kvi) * kD * kD, kD, kD);
                memcpy(wkv.data() + ((size_t)l * 2 + kvi) * kD * kD, t.data(), (size_t)kD * kD * 4);
                memcpy(bkv.data() + ((size_t)l * 2 + kvi) * kD, D.get(p + ".in_proj_bias") + (1 + kvi) * kD, kD * 4);
            }
        if (upload(c, &v->wkv_t, wkv.data(), wkv.size() * 4) || upload(c, &v->bkv, bkv.data(), bkv.size() * 4)) return AMUSE_EHIP;
        if (!v->tkv_sched) HIP_TRY(hipMalloc((void**)&v->tkv_sched, (size_t)AMUSE_MAX_STEPS * kTkv * sizeof(float)));
    }
    // what every arch shares with the shipped configuration: positions, timestep frequencies, time-embedding MLP + condition projections
    if (upload(c, &c->den_pe, D.get("query_pos.pe"), 500 * 128 * 4) || upload(c, &v->m_pe, D.get("mem_pos.pe"), 500 * 128 * 4)) return AMUSE_EHIP;
    v->net.pe = c->den_pe;
    float fr[128];
    for (int k = 0; k < 128; ++k) fr[k] = expf(-logf(10000.f) * (float)k / 128.f);
    if (!c->den_freqs && upload(c, &c->den_freqs, fr, sizeof(fr), PREC_F32, kImgConst)) return AMUSE_EHIP;   // (amuse_set_schedule may have installed the caller's values)
    return upload_embeddings(c, D);
}

void variant_destroy(amuse_ctx* c) {
    amuse_variant* v = c->var;
    if (!v) return;
    void* ptrs[] = {v->tkv_sched, v->ckv, v->tkv1, v->ws, v->tt, v->skip};   // tables and workspaces (the uploaded images belong to c->owned)
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete v;
    c->var = nullptr;
}

int variant_set_schedule(amuse_ctx* c, hipStream_t st) {
    // time token of every step + its position: query_pos.pe[0] in front of the frames, mem_pos.pe[0] as the first memory token
    HIP_TRY(time_tokens(c, c->d_timesteps, c->T, time_pe_row(c), c->d_time_tok, st));
    if (arch_dec(c->arch)) HIP_TRY(launch_mem_kv(c->d_time_tok, c->T, c->var->wkv_t, c->var->bkv, c->var->tkv_sched, st));
    return 0;
}

int variant_sample(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int precision, uint64_t seed,
                   uint64_t clip0, const float* x_init, const float* step_noise, float* out, float* traj_out, hipStream_t st) {
    amuse_variant* v = c->var;
    int ncond = 0;
    if (int e = variant_cond(c, con, emo, sty, B, &ncond, st)) return e;
    if (!arch_pose(c->arch)) {
        SampleDecArgs a{};
        a.wstream = v->dec_w[precision]; a.wave_units = v->dec_units[precision];
        a.pvec = v->net.pvec; a.pe0 = c->den_pe;
        a.mem = MemKV{v->tkv_sched, 0, v->ckv, ncond};
        a.tkv_step_stride = kTkv;
        a.coef = c->d_coef; a.x_init = x_init; a.step_noise = step_noise;
        a.latents_out = out; a.traj_out = traj_out;
        a.seed = seed; a.clip0 = clip0; a.B = B; a.T = c->T; a.no_update = 0;
        HIP_TRY(launch_sample_dec(a, precision, st));
        return 0;
    }
    // pose-space archs: the state is the [300][333] feature sequence, updated in place in `out` step by step
    const size_t sd = AMUSE_POSE_STATE;
    if (x_init) HIP_TRY(hipMemcpyAsync(out, x_init, (size_t)B * sd * sizeof(float), hipMemcpyDeviceToDevice, st));
    else HIP_TRY(launch_counter_normal(seed, clip0, B, 0, 0, out, st, (int)sd));
    const PoseRun run = pose_run_of(c, precision, B);
    if (int e = ensure_pose_ws(v, run.chunk, run.fused)) return e;
    for (int step = 0; step < c->T; ++step) {
        const int e = for_chunks(B, run.chunk, [&](int b0, int nb) {
            PoseStep p{};
            p.x_in = out + (size_t)b0 * sd; p.x_out = out + (size_t)b0 * sd; p.eps_out = nullptr;
            p.coef = c->d_coef + (size_t)step * 8;
            p.step_noise = step_noise ? step_noise + ((size_t)step * B + b0) * sd : nullptr;
            p.ttok = c->d_time_tok + (size_t)step * kD; p.ttok_stride = 0;
            p.tkv = arch_dec(c->arch) ? v->tkv_sched + (size_t)step * kTkv : nullptr; p.tkv_clip_stride = 0;
            p.cond_tok = c->cond_tok + (size_t)b0 * ncond * kD;
            p.ckv = v->ckv ? v->ckv + (size_t)b0 * ncond * kTkv : nullptr;
            p.lengths_dev = nullptr;   // the sampling loop passes full lengths (infer_ldm.py:135)
            p.ncond = ncond; p.step = step; p.seed = seed; p.clip0 = clip0 + (uint64_t)b0; p.rows8 = run.rows8; p.fusedx = run.fusedx;
            return pose_step(c, p, nb, precision, run.fused, st);
        });
        if (e) return e;
        if (traj_out) HIP_TRY(hipMemcpyAsync(traj_out + (size_t)step * B * sd, out, (size_t)B * sd * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

int variant_denoise(amuse_ctx* c, const float* x_t, const int* timesteps, bool per_clip, const float* con, const float* emo,
                    const float* sty, const int* lengths, int B, int precision, float* eps_out, float* tap_out, hipStream_t st) {
    amuse_variant* v = c->var;
    const int nt = per_clip ? B : 1;
    // per-call scratch: time tokens [nt][128] (+ their K / V) and the device copy of the timesteps
    if (int e = ensure(&v->tt, &v->tt_cap, (size_t)B * (kD + 1))) return e;
    float* ttok = v->tt;                                         // [nt][128]
    int* ts = reinterpret_cast<int*>(ttok + (size_t)B * kD);     // [nt]
    HIP_TRY(hipMemcpyAsync(ts, timesteps, (size_t)nt * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // the host array belongs to the caller
    HIP_TRY(time_tokens(c, ts, nt, time_pe_row(c), ttok, st));
    if (arch_dec(c->arch)) {
        if (int e = ensure(&v->tkv1, &v->tkv1_cap, (size_t)nt * kTkv)) return e;
        HIP_TRY(launch_mem_kv(ttok, nt, v->wkv_t, v->bkv, v->tkv1, st));
    }
    int ncond = 0;
    if (int e = variant_cond(c, con, emo, sty, B, &ncond, st)) return e;
    if (!arch_pose(c->arch)) {
        SampleDecArgs a{};
        a.wstream = v->dec_w[precision]; a.wave_units = v->dec_units[precision];
        a.pvec = v->net.pvec; a.pe0 = c->den_pe;
        a.mem = MemKV{v->tkv1, per_clip ? (size_t)kTkv : 0, v->ckv, ncond};
        a.tkv_step_stride = 0;
        a.coef = c->d_coef1; a.x_init = x_t; a.eps_out = eps_out; a.tap_out = tap_out;
        a.B = B; a.T = 1; a.no_update = 1;
        HIP_TRY(launch_sample_dec(a, precision, st));
        return 0;
    }
    if (tap_out) return fail(AMUSE_EINVAL, "taps exist for the latent variants only");
    if (int e = stage_lengths(c, lengths, B, true, st)) return e;
    const size_t sd = AMUSE_POSE_STATE;
    const PoseRun run = pose_run_of(c, precision, B);
    if (int e = ensure_pose_ws(v, run.chunk, run.fused)) return e;
    return for_chunks(B, run.chunk, [&](int b0, int nb) {
        PoseStep p{};
        p.x_in = x_t + (size_t)b0 * sd; p.x_out = nullptr; p.eps_out = eps_out + (size_t)b0 * sd; p.coef = nullptr;
        p.ttok = ttok + (per_clip ? (size_t)b0 * kD : 0); p.ttok_stride = per_clip ? kD : 0;
        p.tkv = arch_dec(c->arch) ? v->tkv1 + (per_clip ? (size_t)b0 * kTkv : 0) : nullptr; p.tkv_clip_stride = per_clip ? kTkv : 0;
        p.cond_tok = c->cond_tok + (size_t)b0 * ncond * kD;
        p.ckv = v->ckv ? v->ckv + (size_t)b0 * ncond * kTkv : nullptr;
        p.lengths_dev = lengths ? c->d_lengths + b0 : nullptr;
        p.ncond = ncond; p.rows8 = run.rows8; p.fusedx = run.fusedx;
        return pose_step(c, p, nb, precision, run.fused, st);
    });
}
