// C ABI of libamuse_hip.so (include/amuse_hip.h): context, weight packing into MFMA-fragment
// streams, workspace, and the launch sequences.  Host code only - kernels live in k_*.hip.
#include "amuse_pack.hpp"
#include "amuse_variants.hpp"

namespace {
thread_local char g_err[512] = "";
}  // namespace
int amuse_failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// the same error slot for the library's other translation units (amuse_audio_api.hip)
__attribute__((visibility("hidden"))) int amuse_fail_msg(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}


namespace {
constexpr int kVaeChunk = 512;
constexpr int kEncRows = kFrames + 2;  // encoder sequence: 2 distribution tokens + 300 frames
constexpr size_t kVaeFloatsPerClip = (size_t)kEncRows * kD * (1 + 3 + 1 + 4) + 4 * kLayers * kD;  // x, qkv, o, skip, ca (train-mode decode: its four per-head partials) | stats

// The builders: which parameters, precision, front / back matrices and AMUSE_UPD_* class go into which stream.  The layouts themselves - the order inside
// a stream and the kernel that consumes it - are stated once each in amuse_pack.hpp.
int build_denoiser(amuse_ctx* c, const float* den, int what = AMUSE_UPD_ALL) {
    static const ParamIndex DI = denoiser_index();
    const Params D{DI, den};
    if (what & AMUSE_UPD_F32) {   // the 4-wave kernel (k_sampler.hip: the fp32 parity mode; every other mode samples on an 8-wave kernel), pack_ring4_stream
        std::vector<uint4> all;
        const auto pass = [&](std::vector<uint4>& s, int w) {
            for (int b = 0; b < 9; ++b) {
                const std::string p = blk_name("encoder", b);
                if (b >= 5) {
                    pack_skiplin(s, PREC_F32, D, "encoder", b - 5, w);
                    pad_units(s, skip_pad_units(PREC_F32));  // ring alignment
                }
                pack_qkv(s, PREC_F32, D.get(p + ".self_attn.in_proj_weight"), w, true);
                pack_outproj_ffn_quarters(s, PREC_F32, D, p, w);
            }
        };
        if (int e = pack_ring4_stream(all, &c->den_wave_units, pass)) return e;
        if (upload(c, &c->den_w, all.data(), all.size() * sizeof(uint4), PREC_F32, AMUSE_UPD_F32)) return AMUSE_EHIP;
    }
    // the 8-wave kernels (pack_sample8_streams): bf16 and fp16 share layout and unit counts, fp32x has its own A-wave order
    struct { int prec; uint4** slot; uint32_t* units; } const w8[3] = {
        {PREC_BF16, &c->den_w8, c->den_w8_units}, {PREC_F16, &c->den_w8h, c->den_w8_units}, {PREC_F16X2, &c->den_w8x, c->den_w8x_units}};
    for (const auto& t : w8) {
        if (!(what & kUpdBit[t.prec])) continue;   // amuse_update_weights: only the requested precisions are re-packed
        std::vector<uint4> all;
        if (int e = pack_sample8_streams(all, t.units, t.prec, D)) return e;
        if (upload(c, t.slot, all.data(), all.size() * sizeof(uint4), t.prec, kUpdBit[t.prec])) return AMUSE_EHIP;
    }
    {
        auto pv = build_pvec(D, "encoder", false);
        if (upload(c, &c->den_pvec, pv.data(), pv.size() * 4)) return AMUSE_EHIP;
        if (upload(c, &c->den_pe, D.get("query_pos.pe"), 500 * 128 * 4)) return AMUSE_EHIP;
        float fr[128];
        for (int k = 0; k < 128; ++k) fr[k] = expf(-logf(10000.f) * (float)k / 128.f);
        if (upload(c, &c->den_freqs, fr, sizeof(fr), PREC_F32, kImgConst)) return AMUSE_EHIP;
    }
    return upload_embeddings(c, D);
}

// block 0's hoisted constants belong to the decoder weights they were computed from
void invalidate_c1(amuse_ctx* c) { c->c1_bf16.valid = c->c1_f16.valid = c->c1_rows8.valid = c->c1_clip.valid = false; }

int build_prior(amuse_ctx* c, const float* pri, int what = AMUSE_UPD_ALL) {
    static const ParamIndex PI = prior_index();
    if (!g_capture) invalidate_c1(c);
    const Params Pp{PI, pri};
    // ---- decoder: final_layer behind stage 9; every stage on the row kernel without split-K
    if (int e = build_rownet_streams(c, c->dec, Pp, {"decoder", nullptr, Pp.get("final_layer.weight"), 0, 9, true, 0}, what)) return e;
    {
        auto pv = build_pvec(Pp, "decoder", true);
        if (upload(c, &c->dec.pvec, pv.data(), pv.size() * 4)) return AMUSE_EHIP;
        std::vector<float> fb(16 * kFeatTiles, 0.f);
        memcpy(fb.data(), Pp.get("final_layer.bias"), kFeats * 4);
        if (upload(c, &c->dec.final_bias, fb.data(), fb.size() * 4)) return AMUSE_EHIP;
        if (upload(c, &c->dec.pe, Pp.get("query_pos_decoder.pe"), 500 * 128 * 4)) return AMUSE_EHIP;
        std::vector<float> wv_t(9 * 128 * 128), wo_t(9 * 128 * 128), bv(9 * 128), bo(9 * 128);
        for (int b = 0; b < 9; ++b) {
            const std::string p = blk_name("decoder", b) + ".multihead_attn";
            auto t1 = transpose(Pp.get(p + ".in_proj_weight") + 256 * 128, 128, 128);
            auto t2 = transpose(Pp.get(p + ".out_proj.weight"), 128, 128);
            memcpy(wv_t.data() + (size_t)b * 128 * 128, t1.data(), 128 * 128 * 4);
            memcpy(wo_t.data() + (size_t)b * 128 * 128, t2.data(), 128 * 128 * 4);
            memcpy(bv.data() + b * 128, Pp.get(p + ".in_proj_bias") + 256, 512);
            memcpy(bo.data() + b * 128, Pp.get(p + ".out_proj.bias"), 512);
        }
        if (upload(c, &c->vae_wv_t, wv_t.data(), wv_t.size() * 4) || upload(c, &c->vae_wo_t, wo_t.data(), wo_t.size() * 4) ||
            upload(c, &c->vae_bv, bv.data(), bv.size() * 4) || upload(c, &c->vae_bo, bo.data(), bo.size() * 4))
            return AMUSE_EHIP;
    }
    // ---- encoder (streams: AMUSE_UPD_ENCODER): skel_embedding in front of stage 0 - that stage stays with k_vae_rows<f16x2, M_ENC>, stages 1..9 on the row kernel
    // without split-K - and nothing behind stage 9; no 16-bit per-clip kernel
    if (int e = build_rownet_streams(c, c->enc, Pp, {"encoder", Pp.get("skel_embedding.weight"), nullptr, 1, 9, false, AMUSE_UPD_ENCODER}, what)) return e;
    {
        auto pv = build_pvec(Pp, "encoder", false);
        if (upload(c, &c->enc.pvec, pv.data(), pv.size() * 4) ||
            upload(c, &c->enc.pe, Pp.get("query_pos_encoder.pe"), 500 * 128 * 4) ||
            upload(c, &c->vaee_tok, Pp.get("global_motion_token"), 2 * 128 * 4) ||
            upload(c, &c->enc.emb_bias, Pp.get("skel_embedding.bias"), 128 * 4))
            return AMUSE_EHIP;
    }
    return 0;
}

int build_ctx(amuse_ctx* c, const float* den, const float* pri) {
    if (int e = c->arch == AMUSE_ARCH_ENC ? build_denoiser(c, den) : variant_build(c, den, AMUSE_UPD_ALL)) return e;
    if (pri)
        if (int e = build_prior(c, pri)) return e;
    HIP_TRY(hipMalloc((void**)&c->d_timesteps, AMUSE_MAX_STEPS * sizeof(int)));
    HIP_TRY(hipMalloc((void**)&c->d_coef, AMUSE_MAX_STEPS * 8 * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->d_time_tok, AMUSE_MAX_STEPS * kD * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->d_ts1, sizeof(int)));
    HIP_TRY(hipMalloc((void**)&c->d_tt1, kD * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->d_coef1, 8 * sizeof(float)));
    HIP_TRY(hipMemset(c->d_coef1, 0, 8 * sizeof(float)));
    return 0;
}

int cond_tokens(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int* S_out, hipStream_t s) {
    CondArgs ca{};
    int n = 0;
    const float* zs[3] = {con, emo, sty};
    for (int i = 0; i < 3; ++i)
        if (zs[i]) { ca.z[n] = zs[i]; ca.wt[n] = c->cond_wt[i]; ca.bias[n] = c->cond_b[i]; ++n; }
    if (int e = ensure(&c->cond_tok, &c->cond_cap, (size_t)B * 3 * kD)) return e;
    ca.pe = c->den_pe; ca.out = c->cond_tok; ca.B = B; ca.ncond = n; ca.pe_base = 2;
    HIP_TRY(launch_cond_tokens(ca, s));
    *S_out = 2 + n;
    return 0;
}

// clips per workgroup tile: the pin (amuse_set_clips_per_group) or the plan's rule (amuse_host.hpp plan_clips_per_group).  A clip's arithmetic depends on its row offset
// inside the tile only through rounding (the softmax / PV accumulation order), so results are reproduced BITWISE by any launch that uses the same clips per tile and puts
// the clip in the same slot of its tile - i.e. by shards that start at multiples of g (amuse_amd/shard.py takes g from amuse_plan for the job's TOTAL clip count and aligns
// the shards) - and to rounding otherwise.
int pick_group(amuse_ctx* c, int B, int S) {
    const int gmax = 16 / S;
    int g = c->clips_per_group > 0 ? c->clips_per_group : plan_clips_per_group(AMUSE_ARCH_ENC, B, S);
    if (g > gmax) g = gmax;
    c->last_plan[0] = g;
    return g;
}

// kernel choice for one sampling launch: fp32 -> the 4-wave parity kernel (k_sampler.hip); fp32x / bf16 / fp16 -> the 8-wave kernels
bool use_sample8(int precision) { return precision != PREC_F32; }
void set_stream(const amuse_ctx* c, SampleArgs& a, int precision) {
    if (precision == PREC_F32) { a.wstream = c->den_w; a.wave_units = c->den_wave_units; }
    a.wave_units_a = c->den_w8_units[0]; a.wave_units_b = c->den_w8_units[1];
}
hipError_t dispatch_sample(amuse_ctx* c, SampleArgs& a, int precision, hipStream_t st) {
    if (use_sample8(precision)) {  // with prof_out: stamps come back as [8 waves][96] in the same 768-entry buffer
        if (precision == PREC_F16X2) {
            a.wstream = c->den_w8x; a.wave_units_a = c->den_w8x_units[0]; a.wave_units_b = c->den_w8x_units[1];
            return launch_sample8x(a, st);
        }
        if (precision == PREC_F16) {   // the same streams' layout and unit counts, fp16 weights
            a.wstream = c->den_w8h;
            return launch_sample8h(a, st);
        }
        a.wstream = c->den_w8;
        return launch_sample8(a, st);
    }
    return launch_sample(a, precision, st);
}

// decode / encode kernels of a call: the pin (amuse_set_decode_path) or the plan (amuse_host.hpp plan_decode_path / plan_encode_path), recorded for amuse_debug_last_plan
constexpr int kVaeFusedChunk = 4096;
int decode_path_of(amuse_ctx* c, int precision, int B) {
    int path = resolve_path(c->decode_path, plan_decode_path(precision, B), precision);
    if (path == AMUSE_DECODE_CLIP && !c->dec.fusedx) path = AMUSE_DECODE_FUSED;
    return c->last_plan[1] = path;
}
int encode_path_of(amuse_ctx* c, int precision, int B) {
    int path = precision == AMUSE_PREC_F32X ? resolve_path(c->decode_path, plan_encode_path(precision, B), precision) : AMUSE_DECODE_STAGED;
    if (path == AMUSE_DECODE_CLIP && !c->enc.fusedx) path = AMUSE_DECODE_FUSED;
    if (path == AMUSE_DECODE_FUSED && !c->enc.rows8) path = AMUSE_DECODE_STAGED;
    return c->last_plan[2] = path;
}

int ensure_vae_ws(amuse_ctx* c, int chunk) {   // (+ 1 KiB: k_vae_fusedx copies a clip's 4.5 KiB of ca in five 1 KiB pieces)
    return ensure(&c->vae_ws, &c->vae_cap, (size_t)chunk, (size_t)chunk * kVaeFloatsPerClip + 256);
}

// train-mode sampling (amuse_set_sample_dropout) of one amuse_sample / amuse_denoise_step / amuse_profile_sample call: refused where no kernel draws
// the masks (AMUSE_ARCH_ENC in fp32, bf16 and fp16 only), so that dropout is never silently dropped
int sample_dropout(const amuse_ctx* c, int precision, SampleArgs& a) {
    if (c->drop_thr == 0) return 0;
    if (c->arch != AMUSE_ARCH_ENC)
        return fail(AMUSE_ESTATE, "train-mode sampling (amuse_set_sample_dropout p > 0) exists for AMUSE_ARCH_ENC only, this context is arch %d", c->arch);
    if (precision == AMUSE_PREC_F32X)
        return fail(AMUSE_ESTATE, "train-mode sampling (amuse_set_sample_dropout p > 0) has no fp32x kernel: use fp32, bf16 or fp16");
    a.drop_thr = c->drop_thr; a.drop_scale = c->drop_scale; a.drop_seed = c->drop_seed;
    return 0;
}

// what every entry point on the shipped sampler's kernels puts into its launch: condition tokens, streams, parameters, tile geometry.  The caller has zeroed `a`
// (and, where the entry point has a train mode, run sample_dropout on it) and adds its time tokens, coefficients and inputs / outputs.
int sample_args(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int precision, hipStream_t st, SampleArgs& a) {
    int S = 0;
    if (int e = cond_tokens(c, con, emo, sty, B, &S, st)) return e;
    set_stream(c, a, precision);
    a.pvec = c->den_pvec; a.cond_tok = c->cond_tok; a.pe0 = c->den_pe;
    a.B = B; a.S = S; a.G = pick_group(c, B, S);
    return 0;
}

int check_common(amuse_ctx* c, const float* con, int B, int precision) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!con) return fail(AMUSE_EINVAL, "con is NULL (the content embedding is mandatory, denoiser.py:153-157)");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1, got %d", B);
    if (precision < AMUSE_PREC_F32 || precision > AMUSE_PREC_F16) return fail(AMUSE_EINVAL, "bad precision %d", precision);
    HIP_TRY(hipSetDevice(c->device));
    return 0;
}
}  // namespace

extern "C" {

int amuse_abi_version(void) { return AMUSE_ABI_VERSION; }
int amuse_debug_f16_split(const float* w, size_t n, uint16_t* hi, uint16_t* lo) {
    if (!w || !hi || !lo) return fail(AMUSE_EINVAL, "NULL argument");
    for (size_t i = 0; i < n; ++i) {
        hi[i] = f2h(w[i]);
        lo[i] = f2h(w[i] - h2f(hi[i]));
    }
    return 0;
}
const char* amuse_last_error(void) { return g_err; }

size_t amuse_denoiser_param_count(int arch) { return arch == AMUSE_ARCH_ENC ? (size_t)AMUSE_DENOISER_PARAMS : variant_param_count(arch); }
int amuse_arch(const amuse_ctx* c) { return c ? c->arch : AMUSE_EINVAL; }
size_t amuse_state_dim(const amuse_ctx* c) { return c ? variant_state_dim(c->arch) : 0; }

amuse_ctx* amuse_create(int device, const float* denoiser_params, size_t n_denoiser, const float* prior_params,
                        size_t n_prior) {
    if (!prior_params) { fail(AMUSE_EINVAL, "NULL parameter array"); return nullptr; }
    return amuse_create_arch(device, AMUSE_ARCH_ENC, denoiser_params, n_denoiser, prior_params, n_prior);
}

amuse_ctx* amuse_create_arch(int device, int arch, const float* denoiser_params, size_t n_denoiser, const float* prior_params,
                             size_t n_prior) {
    if (arch < AMUSE_ARCH_ENC || arch > AMUSE_ARCH_DEC_POSE) { fail(AMUSE_EINVAL, "unknown arch %d", arch); return nullptr; }
    const bool pose = (arch & 2) != 0;
    if (!denoiser_params || (!prior_params && !pose)) { fail(AMUSE_EINVAL, "NULL parameter array"); return nullptr; }
    if (n_denoiser != amuse_denoiser_param_count(arch) || (prior_params ? n_prior != AMUSE_PRIOR_PARAMS : n_prior != 0)) {
        fail(AMUSE_EINVAL, "parameter count mismatch: denoiser %zu (want %zu for arch %d), prior %zu (want %u)", n_denoiser,
             amuse_denoiser_param_count(arch), arch, n_prior, AMUSE_PRIOR_PARAMS);
        return nullptr;
    }
    if (denoiser_index().total != AMUSE_DENOISER_PARAMS || prior_index().total != AMUSE_PRIOR_PARAMS ||
        variant_param_count(AMUSE_ARCH_DEC) != AMUSE_DENOISER_PARAMS_DEC || variant_param_count(AMUSE_ARCH_ENC_POSE) != AMUSE_DENOISER_PARAMS_ENC_POSE ||
        variant_param_count(AMUSE_ARCH_DEC_POSE) != AMUSE_DENOISER_PARAMS_DEC_POSE) {
        fail(AMUSE_ESTATE, "internal: state-dict index does not add up");
        return nullptr;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { fail(AMUSE_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e)); return nullptr; }
    amuse_ctx* c = new amuse_ctx();
    c->device = device;
    c->arch = arch;
    c->has_prior = prior_params != nullptr;
    if (build_ctx(c, denoiser_params, prior_params) != 0) { amuse_destroy(c); return nullptr; }
    return c;
}

int amuse_update_weights(amuse_ctx* c, const float* denoiser_params, size_t n_denoiser, const float* prior_params,
                         size_t n_prior, int what, void* stream) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!denoiser_params && !prior_params) return fail(AMUSE_EINVAL, "nothing to update");
    if (what < 1 || what > AMUSE_UPD_ALL || !(what & (AMUSE_UPD_F32 | AMUSE_UPD_BF16 | AMUSE_UPD_F32X | AMUSE_UPD_F16))) return fail(AMUSE_EINVAL, "bad `what` mask %d", what);
    if (denoiser_params && n_denoiser != amuse_denoiser_param_count(c->arch))
        return fail(AMUSE_EINVAL, "denoiser parameter count %zu (want %zu)", n_denoiser, amuse_denoiser_param_count(c->arch));
    if (prior_params && n_prior != AMUSE_PRIOR_PARAMS)
        return fail(AMUSE_EINVAL, "prior parameter count %zu (want %u)", n_prior, AMUSE_PRIOR_PARAMS);
    if (prior_params && !c->has_prior) return fail(AMUSE_ESTATE, "this context was created without MotionPrior weights");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // kernels in flight still read the old streams
    if (denoiser_params) {
        if (int e = c->arch == AMUSE_ARCH_ENC ? build_denoiser(c, denoiser_params, what) : variant_build(c, denoiser_params, what)) return e;
        c->T = 0;   // the hoisted time-token table belongs to the old time-embedding weights: set the schedule again
    }
    if (prior_params)
        if (int e = build_prior(c, prior_params, what)) return e;
    return 0;
}

namespace {
// The gather maps.  Every image the builders upload is a permutation of parameters plus zero padding (the one exception,
// the timestep frequencies, is uploaded as kImgConst and never captured), so three builder runs on probe parameters - byte k
// of (index + 1), a value bf16 holds exactly - spell out, per image element, which parameter it carries.
int build_repack_maps(amuse_ctx* c) {
    struct Img { std::vector<int> map; bool prior; int kind, cls; };   // kind / cls: as the builder classified the image (upload, amuse_host.hpp)
    std::map<void**, Img> imgs;
    std::vector<float> den(AMUSE_DENOISER_PARAMS), pri(AMUSE_PRIOR_PARAMS);
    for (int k = 0; k < 3; ++k) {
        for (size_t i = 0; i < den.size(); ++i) den[i] = (float)(((i + 1) >> (8 * k)) & 255);
        for (size_t i = 0; i < pri.size(); ++i) pri[i] = (float)(((i + 1) >> (8 * k)) & 255);
        for (int which = 0; which < 2; ++which) {
            Capture cap;
            g_capture = &cap;
            g_probe_f16 = true;
            const int rc = which == 0 ? build_denoiser(c, den.data(), AMUSE_UPD_ALL) : build_prior(c, pri.data(), AMUSE_UPD_ALL);
            g_probe_f16 = false;
            g_capture = nullptr;
            if (rc) return rc;
            for (auto& kv : cap.bufs) {
                const std::vector<unsigned char>& bytes = kv.second.bytes;
                const int kind = kv.second.kind;
                const size_t n = bytes.size() / (kind ? 2 : 4);
                Img& im = imgs[kv.first];
                if (k == 0) { im.map.assign(n, 0); im.prior = which == 1; im.kind = kind; im.cls = kv.second.cls; }
                else if (im.map.size() != n) return fail(AMUSE_ESTATE, "internal: packed image changed size between probe runs");
                for (size_t j = 0; j < n; ++j) {
                    float v;
                    if (kind == 1) {
                        uint16_t h;
                        memcpy(&h, bytes.data() + 2 * j, 2);
                        const uint32_t u = (uint32_t)h << 16;
                        memcpy(&v, &u, 4);
                    } else if (kind == 2 || kind == 3) {
                        uint16_t h;
                        memcpy(&h, bytes.data() + 2 * j, 2);
                        v = h2f(h);
                    } else {
                        memcpy(&v, bytes.data() + 4 * j, 4);
                    }
                    if (!(v >= 0.f && v <= 255.f && v == (float)(int)v)) return fail(AMUSE_ESTATE, "internal: a packed image is not a gather of the parameters");
                    im.map[j] |= (int)v << (8 * k);
                }
            }
        }
    }
    for (auto& kv : imgs) {
        void** slot = kv.first;
        const size_t limit = kv.second.prior ? AMUSE_PRIOR_PARAMS : AMUSE_DENOISER_PARAMS;
        for (int m : kv.second.map)
            if (m < 0 || (size_t)m > limit) return fail(AMUSE_ESTATE, "internal: gather index out of range");
        int* dmap = nullptr;
        HIP_TRY(hipMalloc((void**)&dmap, kv.second.map.size() * sizeof(int)));
        c->owned.push_back(dmap);
        HIP_TRY(hipMemcpy(dmap, kv.second.map.data(), kv.second.map.size() * sizeof(int), hipMemcpyHostToDevice));
        c->repack.push_back({slot, dmap, kv.second.map.size(), kv.second.prior ? 1 : 0, kv.second.kind, kv.second.cls});
    }
    return 0;
}
}  // namespace

int amuse_update_weights_device(amuse_ctx* c, const float* denoiser_params_dev, const float* prior_params_dev, int what, void* stream) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!denoiser_params_dev && !prior_params_dev) return fail(AMUSE_EINVAL, "nothing to update");
    if (what < 1 || what > AMUSE_UPD_ALL || !(what & (AMUSE_UPD_F32 | AMUSE_UPD_BF16 | AMUSE_UPD_F32X | AMUSE_UPD_F16))) return fail(AMUSE_EINVAL, "bad `what` mask %d", what);
    if (c->arch != AMUSE_ARCH_ENC || !c->has_prior) return fail(AMUSE_ESTATE, "the device re-pack exists for the shipped configuration (AMUSE_ARCH_ENC) only; use amuse_update_weights");
    HIP_TRY(hipSetDevice(c->device));
    if (c->repack.empty())
        if (int e = build_repack_maps(c)) return e;
    if (prior_params_dev) invalidate_c1(c);
    for (const auto& r : c->repack) {
        const float* src = r.prior ? prior_params_dev : denoiser_params_dev;
        if (!src) continue;                             // (only one of the two parameter arrays given)
        if ((r.cls & what) != r.cls) continue;          // every bit the image needs must be requested
        HIP_TRY(launch_repack(src, r.map, *r.slot, r.n, r.kind, (hipStream_t)stream));
    }
    // the hoisted time-token table belongs to the old time-embedding weights: rebuilt here, stream-ordered, from the schedule's
    // timesteps (still on the device) - no host round trip, the schedule stays set
    if (denoiser_params_dev && c->T > 0)
        HIP_TRY(time_tokens(c, c->d_timesteps, c->T, c->den_pe + kD, c->d_time_tok, (hipStream_t)stream));
    return 0;
}

void amuse_destroy(amuse_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    variant_destroy(c);
    for (void* p : c->owned)
        if (p) (void)hipFree(p);
    // (the weight images are in `owned`: upload() put them there)  schedule buffers and workspaces:
    void* ptrs[] = {c->d_timesteps, c->d_coef, c->d_time_tok, c->d_ts1, c->d_tt1, c->d_coef1, c->cond_tok, c->lat_tmp, c->fwd_ws, c->vae_ws, c->d_lengths,
                    c->vae_skip, c->vae_ca_ws, c->c1_bf16.buf, c->c1_f16.buf, c->c1_rows8.buf, c->c1_clip.buf};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : {c->c1_bf16.event, c->c1_f16.event, c->c1_rows8.event, c->c1_clip.event})
        if (e) (void)hipEventDestroy(e);
    delete c;
}

int amuse_set_clips_per_group(amuse_ctx* c, int g) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (g < 0 || g > 5) return fail(AMUSE_EINVAL, "clips per group must be 0 (auto) .. 5, got %d", g);
    c->clips_per_group = g;
    return 0;
}

int amuse_set_sample_dropout(amuse_ctx* c, float p, uint64_t seed) {
    if (!(p >= 0.f) || p >= 1.f) return fail(AMUSE_EINVAL, "dropout probability %g outside [0, 1)", (double)p);
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    c->drop_thr = (uint32_t)(p * 16777216.0f);   // amuse_train.hip drop_args
    c->drop_scale = 1.0f / (1.0f - p);
    c->drop_seed = seed;
    return 0;
}

int amuse_set_decode_dropout(amuse_ctx* c, float p, uint64_t seed, uint64_t clip_index0) {
    if (!(p >= 0.f) || p >= 1.f) return fail(AMUSE_EINVAL, "dropout probability %g outside [0, 1)", (double)p);
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    c->dec_drop_thr = (uint32_t)(p * 16777216.0f);   // amuse_train.hip drop_args
    c->dec_drop_scale = 1.0f / (1.0f - p);
    c->dec_drop_seed = seed;
    c->dec_drop_clip0 = clip_index0;
    return 0;
}

int amuse_set_decode_path(amuse_ctx* c, int path) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (path != AMUSE_DECODE_AUTO && path != AMUSE_DECODE_STAGED && path != AMUSE_DECODE_FUSED && path != AMUSE_DECODE_CLIP)
        return fail(AMUSE_EINVAL, "bad decode path %d", path);
    c->decode_path = path;
    return 0;
}

int amuse_plan(int arch, int precision, int clips_total, int tokens, int* clips_per_group, int* decode_path, int* encode_path, int* step_path) {
    if (arch < AMUSE_ARCH_ENC || arch > AMUSE_ARCH_DEC_POSE) return fail(AMUSE_EINVAL, "bad arch %d", arch);
    if (precision < AMUSE_PREC_F32 || precision > AMUSE_PREC_F16) return fail(AMUSE_EINVAL, "bad precision %d", precision);
    if (clips_total < 1) return fail(AMUSE_EINVAL, "clips_total must be >= 1, got %d", clips_total);
    if (tokens < 3 || tokens > 5) return fail(AMUSE_EINVAL, "tokens must be 3..5 (latent + time + content [+ emotion] [+ style]), got %d", tokens);
    if (clips_per_group) *clips_per_group = plan_clips_per_group(arch, clips_total, tokens);
    if (decode_path) *decode_path = plan_decode_path(precision, clips_total);
    if (encode_path) *encode_path = plan_encode_path(precision, clips_total);
    if (step_path) *step_path = plan_step_path(arch, precision, clips_total);
    return 0;
}

int amuse_debug_last_plan(const amuse_ctx* c, int* clips_per_group, int* decode_path, int* encode_path, int* step_path) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (clips_per_group) *clips_per_group = c->last_plan[0];
    if (decode_path) *decode_path = c->last_plan[1];
    if (encode_path) *encode_path = c->last_plan[2];
    if (step_path) *step_path = c->last_plan[3];
    return 0;
}

int amuse_debug_set_decode_tap(amuse_ctx* c, float* tap_out) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    c->decode_tap = tap_out;
    return 0;
}

int amuse_debug_set_ablation(amuse_ctx* c, int mask) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (mask < 0 || mask > 1) return fail(AMUSE_EINVAL, "bad ablation mask %d", mask);
    c->ablate = mask;
    return 0;
}

int amuse_set_schedule(amuse_ctx* c, const amuse_schedule* s, void* stream) {
    if (!c || !s) return fail(AMUSE_EINVAL, "NULL argument");
    if (s->n_steps < 1 || s->n_steps > AMUSE_MAX_STEPS) return fail(AMUSE_EINVAL, "n_steps %d out of range", s->n_steps);
    if (!s->timesteps || !s->coef) return fail(AMUSE_EINVAL, "schedule tables are NULL");
    for (int i = 0; i < s->n_steps; ++i) {
        if (s->timesteps[i] < 0) return fail(AMUSE_EINVAL, "negative timestep at step %d", i);
        if (!(s->coef[i * 8 + 1] > 0.f)) return fail(AMUSE_EINVAL, "sqrt(alpha_bar) must be > 0 at step %d", i);
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(c->d_timesteps, s->timesteps, s->n_steps * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_coef, s->coef, (size_t)s->n_steps * 8 * sizeof(float), hipMemcpyHostToDevice));
    if (s->freqs) HIP_TRY(hipMemcpy(c->den_freqs, s->freqs, 128 * sizeof(float), hipMemcpyHostToDevice));
    c->T = s->n_steps;
    if (c->arch != AMUSE_ARCH_ENC) {
        if (int e = variant_set_schedule(c, st)) { c->T = 0; return e; }
    } else {
        HIP_TRY(time_tokens(c, c->d_timesteps, s->n_steps, c->den_pe + kD, c->d_time_tok, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int amuse_sample(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int precision,
                 uint64_t seed, uint64_t clip_index0, const float* x_init, const float* step_noise,
                 float* latents_out, float* traj_out, void* stream) {
    if (int e = check_common(c, con, B, precision)) return e;
    if (c->T < 1) return fail(AMUSE_ESTATE, "amuse_set_schedule has not been called");
    if (!latents_out) return fail(AMUSE_EINVAL, "latents_out is NULL");
    hipStream_t st = (hipStream_t)stream;
    SampleArgs a{};
    if (int e = sample_dropout(c, precision, a)) return e;
    if (c->arch != AMUSE_ARCH_ENC)
        return variant_sample(c, con, emo, sty, B, precision, seed, clip_index0, x_init, step_noise, latents_out, traj_out, st);
    if (int e = sample_args(c, con, emo, sty, B, precision, st, a)) return e;
    a.time_tok = c->d_time_tok; a.coef = c->d_coef; a.T = c->T;
    a.x_init = x_init; a.step_noise = step_noise; a.latents_out = latents_out; a.traj_out = traj_out;
    a.seed = seed; a.clip0 = clip_index0;
    HIP_TRY(dispatch_sample(c, a, precision, st));
    return 0;
}

int amuse_profile_sample(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int precision,
                         int prof_step, unsigned long long* stamps_out, void* stream) {
    if (int e = check_common(c, con, B, precision)) return e;
    if (c->T < 1) return fail(AMUSE_ESTATE, "amuse_set_schedule has not been called");
    if (!stamps_out || prof_step < 0 || prof_step >= c->T) return fail(AMUSE_EINVAL, "bad stamps_out / prof_step");
    if (c->arch != AMUSE_ARCH_ENC) return fail(AMUSE_ESTATE, "phase stamps exist for the AMUSE_ARCH_ENC sampling kernels only");
    hipStream_t st = (hipStream_t)stream;
    SampleArgs a{};
    if (int e = sample_dropout(c, precision, a)) return e;
    if (int e = sample_args(c, con, emo, sty, B, precision, st, a)) return e;
    if (int e = ensure(&c->lat_tmp, &c->lat_cap, (size_t)B * kD)) return e;
    HIP_TRY(hipMemsetAsync(stamps_out, 0, 4 * kProfStamps * sizeof(unsigned long long), st));
    a.time_tok = c->d_time_tok; a.coef = c->d_coef; a.T = c->T;
    a.latents_out = c->lat_tmp;
    a.seed = 1;
    a.prof_out = stamps_out; a.prof_step = prof_step;
    HIP_TRY(dispatch_sample(c, a, precision, st));
    return 0;
}

int amuse_denoise_step(amuse_ctx* c, const float* x_t, int timestep, const float* con, const float* emo,
                       const float* sty, int B, int precision, float* eps_out, float* tap_out, void* stream) {
    if (int e = check_common(c, con, B, precision)) return e;
    if (!x_t || !eps_out) return fail(AMUSE_EINVAL, "x_t / eps_out is NULL");
    if (timestep < 0) return fail(AMUSE_EINVAL, "negative timestep");
    hipStream_t st = (hipStream_t)stream;
    SampleArgs a{};
    if (int e = sample_dropout(c, precision, a)) return e;
    if (c->arch != AMUSE_ARCH_ENC) return variant_denoise(c, x_t, &timestep, false, con, emo, sty, nullptr, B, precision, eps_out, tap_out, st);
    HIP_TRY(hipMemcpyAsync(c->d_ts1, &timestep, sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // `timestep` lives on this call's stack
    HIP_TRY(time_tokens(c, c->d_ts1, 1, c->den_pe + kD, c->d_tt1, st));
    if (int e = sample_args(c, con, emo, sty, B, precision, st, a)) return e;
    a.time_tok = c->d_tt1; a.coef = c->d_coef1; a.T = 1; a.no_update = 1;
    a.x_init = x_t; a.eps_out = eps_out; a.tap_out = tap_out;
    HIP_TRY(dispatch_sample(c, a, precision, st));
    return 0;
}

int amuse_diffusion_forward(amuse_ctx* c, const float* z0, const float* noise, const int* timesteps, const float* sqrt_ab,
                            const float* sqrt_1m_ab, const float* con, const float* emo, const float* sty, int B,
                            int precision, float* noisy_out, float* noise_pred_out, void* stream) {
    if (int e = check_common(c, con, B, precision)) return e;
    if (!z0 || !noise || !timesteps || !sqrt_ab || !sqrt_1m_ab || !noise_pred_out) return fail(AMUSE_EINVAL, "NULL argument");
    for (int b = 0; b < B; ++b)
        if (timesteps[b] < 0) return fail(AMUSE_EINVAL, "timesteps[%d] = %d is negative", b, timesteps[b]);
    hipStream_t st = (hipStream_t)stream;
    if (c->arch != AMUSE_ARCH_ENC) {   // the same call on a variant's state ([B][state_dim]); its denoiser pass takes the per-clip timesteps
        const size_t sd = variant_state_dim(c->arch);
        if (int e = ensure(&c->fwd_ws, &c->fwd_cap, (size_t)B * (sd + 2))) return e;
        float* noisy_v = c->fwd_ws;
        float* sa_v = noisy_v + (size_t)B * sd;
        float* sb_v = sa_v + B;
        HIP_TRY(hipMemcpyAsync(sa_v, sqrt_ab, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sb_v, sqrt_1m_ab, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // the host arrays belong to the caller
        HIP_TRY(launch_add_noise(z0, noise, sa_v, sb_v, noisy_v, B, st, (int)sd));
        if (int e = variant_denoise(c, noisy_v, timesteps, true, con, emo, sty, nullptr, B, precision, noise_pred_out, nullptr, st)) return e;
        if (noisy_out) HIP_TRY(hipMemcpyAsync(noisy_out, noisy_v, (size_t)B * sd * sizeof(float), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    // per-clip scratch: noisy latents, time tokens, the two coefficient vectors and the timesteps
    if (int e = ensure(&c->fwd_ws, &c->fwd_cap, (size_t)B * (2 * kD + 3))) return e;
    float* noisy = c->fwd_ws;
    float* ttok = noisy + (size_t)B * kD;
    float* sa = ttok + (size_t)B * kD;
    float* sb = sa + B;
    int* ts = reinterpret_cast<int*>(sb + B);
    HIP_TRY(hipMemcpyAsync(ts, timesteps, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sa, sqrt_ab, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sb, sqrt_1m_ab, (size_t)B * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // the host arrays belong to the caller
    HIP_TRY(launch_add_noise(z0, noise, sa, sb, noisy, B, st));
    HIP_TRY(time_tokens(c, ts, B, c->den_pe + kD, ttok, st));
    SampleArgs a{};   // (eval: this entry point has no train mode)
    if (int e = sample_args(c, con, emo, sty, B, precision, st, a)) return e;
    a.time_tok = ttok; a.time_tok_clip = ttok; a.coef = c->d_coef1; a.T = 1; a.no_update = 1;
    a.x_init = noisy; a.eps_out = noise_pred_out;
    HIP_TRY(dispatch_sample(c, a, precision, st));
    if (noisy_out) HIP_TRY(hipMemcpyAsync(noisy_out, noisy, (size_t)B * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // extern "C"

namespace {
// Block 0's hoisted constant (HoistedC1, amuse_host.hpp) is produced on the stream of the decode that first needed it; the validity flag is host state.  A later decode
// on ANOTHER stream (the trainer's sampler stream beside the caller's) must not read it before those launches finish: an event marks the producer's place, and a
// consumer on a different stream waits on it.  Same stream: nothing to do (stream order).
template <typename F>
int produce_c1(HoistedC1& h, size_t floats, hipStream_t st, F&& launches) {   // runs `launches` (they fill h.buf) only if the constant is not valid
    if (h.valid) return 0;
    if (!h.buf) HIP_TRY(hipMalloc((void**)&h.buf, floats * sizeof(float)));
    if (int e = launches()) return e;
    if (!h.event) HIP_TRY(hipEventCreateWithFlags(&h.event, hipEventDisableTiming));
    h.stream = st;
    HIP_TRY(hipEventRecord(h.event, st));
    h.valid = true;
    return 0;
}
hipError_t consume_c1(const HoistedC1& h, hipStream_t st) {
    if (!h.event || h.stream == st) return hipSuccess;
    return hipStreamWaitEvent(st, h.event, 0);
}

// train-mode decode (amuse_set_decode_dropout p > 0) is refused where no kernel draws the masks, so that dropout is never silently dropped
int decode_dropout_refused(const amuse_ctx* c, int precision) {
    if (c->dec_drop_thr == 0) return 0;
    if (!c->has_prior) return fail(AMUSE_ESTATE, "this context was created without MotionPrior weights");
    if (precision == AMUSE_PREC_F32X)
        return fail(AMUSE_ESTATE, "train-mode decode (amuse_set_decode_dropout p > 0) has no fp32x kernel: use fp32, bf16 or fp16");
    return 0;
}

// one decode call as its kernel families see it; clip0 = global index of clip 0 (the dropout masks of train-mode decode; unused in eval)
struct DecodeCall {
    const float* z; const int* lengths; int B, precision, quat_mode;
    float *feats_out, *poses_out, *trans_out;
    hipStream_t st; uint64_t clip0;
};
template <typename T>
T* at_clip(T* p, int b0, size_t per_clip) { return p ? p + (size_t)b0 * per_clip : nullptr; }
hipError_t decode_ca(const amuse_ctx* c, const float* z, bool bias, float* ca, int nb, hipStream_t st) {   // (no bias: the per-head form of train-mode decode)
    return launch_vae_ca(z, c->vae_wv_t, c->vae_bv, c->vae_wo_t, bias ? c->vae_bo : nullptr, ca, nb, st);
}

// bf16 / fp16 throughput modes from kFusedMinClips clips up: one persistent workgroup per clip (k_vae_fused.hip)
int decode_fused16(amuse_ctx* c, const DecodeCall& d) {
    const bool f16 = d.precision == PREC_F16;
    const auto launch = f16 ? launch_vae_fusedh : launch_vae_fused;
    const int chunk = d.B < kVaeFusedChunk ? d.B : kVaeFusedChunk;
    if (int e = ensure(&c->vae_skip, &c->vae_skip_cap, (size_t)chunk, (size_t)chunk * (kVaeFusedSkipBytesPerClip / sizeof(uint4)))) return e;
    if (int e = ensure(&c->vae_ca_ws, &c->vae_ca_cap, (size_t)chunk * kLayers * kD + 256)) return e;   // + the DMA's overrun
    VaeFusedArgs base{};
    base.wstream = c->dec.fused16[f16]; base.pvec = c->dec.pvec; base.final_bias = c->dec.final_bias; base.pe = c->dec.pe;
    base.ca = c->vae_ca_ws; base.skip = c->vae_skip; base.quat_mode = d.quat_mode; base.ablate_attention = c->ablate & 1;
    // Block 0's self-attention half does not depend on the latent (k_vae_fused.hip / amuse_fused.hpp decoder_block, c1): computed once
    // per weight set by the kernel's own tapped instantiation on one clip, stream-ordered in front of the first decode that uses it
    // (the same bits as recomputing block 0 per clip: profiles/r04_decode_hoist_ab.txt).
    HoistedC1& h = f16 ? c->c1_f16 : c->c1_bf16;
    constexpr size_t kC1Floats = (size_t)kFrames * kD, kTapFloats = 11 * kC1Floats;
    if (!c->decode_tap && !(c->ablate & 1))
        if (int e = produce_c1(h, kC1Floats + kTapFloats, d.st, [&]() -> int {
                float* tap = h.buf + kC1Floats;
                HIP_TRY(decode_ca(c, d.z, true, c->vae_ca_ws, 1, d.st));
                VaeFusedArgs fa = base;
                fa.B = 1; fa.tap_out = tap;
                HIP_TRY(launch(fa, d.st));
                HIP_TRY(hipMemcpyAsync(h.buf, tap + 10 * kC1Floats, kC1Floats * sizeof(float), hipMemcpyDeviceToDevice, d.st));
                return 0;
            }))
            return e;
    if (h.valid) HIP_TRY(consume_c1(h, d.st));
    return for_chunks(d.B, chunk, [&](int b0, int nb) -> int {
        HIP_TRY(decode_ca(c, d.z + (size_t)b0 * kD, true, c->vae_ca_ws, nb, d.st));
        VaeFusedArgs fa = base;
        fa.lengths = d.lengths ? c->d_lengths + b0 : nullptr;
        fa.feats_out = at_clip(d.feats_out, b0, kFrames * kFeats);
        fa.poses_out = at_clip(d.poses_out, b0, kFrames * kJoints * 3);
        fa.trans_out = at_clip(d.trans_out, b0, kFrames * 3);
        fa.B = nb;
        fa.tap_out = b0 == 0 ? c->decode_tap : nullptr;   // (amuse_debug_set_decode_tap: tests)
        fa.c1 = (h.valid && !fa.tap_out) ? h.buf : nullptr;
        HIP_TRY(launch(fa, d.st));
        return 0;
    });
}

// the staged kernels' arguments of clips [b0, b0 + nb) of a decode: the decoder's streams, the workspace carved for nb clips (the cross-attention constant in its
// tail), this chunk's lengths and outputs
StageArgs decode_stage_args(const amuse_ctx* c, const DecodeCall& d, int b0, int nb, const StageWs& w) {
    StageArgs a = stage_args(c->dec, d.precision, w, nb);
    a.rows.ca = w.tail;
    a.rows.lengths = a.attn.lengths = d.lengths ? c->d_lengths + b0 : nullptr;
    a.rows.feats_out = at_clip(d.feats_out, b0, kFrames * kFeats);
    a.rows.poses_out = at_clip(d.poses_out, b0, kFrames * kJoints * 3);
    a.rows.trans_out = at_clip(d.trans_out, b0, kFrames * 3);
    a.rows.quat_mode = d.quat_mode;
    return a;
}

// the fp32x decode as ONE persistent workgroup per clip (k_vae_fusedx.hip; CLIP) where the call's clips fill rounds of the chip; its scratch arrays are the staged
// path's attn_o and skip
int decode_clipx(amuse_ctx* c, const DecodeCall& d) {
    const int chunk = d.B < kVaeChunk ? d.B : kVaeChunk;
    if (int e = ensure_vae_ws(c, chunk)) return e;
    // block 0's self-attention half is one [300][128] constant per weight set for full-length clips (the decoder's queries are the positional table): computed
    // once by THIS kernel on one clip (c1_out: the same instruction stream, the same bits), then every full-length clip starts behind norm1 and the kernel's
    // weight stream behind block 0's sixteen attention stages.  Explicit lengths take the full path.
    const bool hoist = !d.lengths && !c->decode_tap;
    return for_chunks(d.B, chunk, [&](int b0, int nb) -> int {
        const StageWs w = carve_stage_ws(c->vae_ws, (size_t)nb * kFrames);
        const VaeRowsArgs ra = decode_stage_args(c, d, b0, nb, w).rows;
        HIP_TRY(decode_ca(c, d.z + (size_t)b0 * kD, true, w.tail, nb, d.st));
        VaeFusedXArgs fx{};
        fx.wstream = c->dec.fusedx; fx.pvec = ra.pvec; fx.final_bias = ra.final_bias; fx.pe = ra.pe; fx.ca = w.tail;
        fx.skip = w.skip; fx.obuf = w.attn_o; fx.quat_mode = d.quat_mode;
        if (hoist) {
            if (int e = produce_c1(c->c1_clip, (size_t)kFrames * kD, d.st, [&]() -> int {
                    VaeFusedXArgs px = fx;
                    px.B = 1; px.c1_out = c->c1_clip.buf;
                    HIP_TRY(launch_vae_fusedx(px, d.st));
                    return 0;
                }))
                return e;
            HIP_TRY(consume_c1(c->c1_clip, d.st));
            fx.c1 = c->c1_clip.buf;
        }
        fx.lengths = ra.lengths; fx.feats_out = ra.feats_out; fx.poses_out = ra.poses_out; fx.trans_out = ra.trans_out;
        fx.tap_out = b0 == 0 ? c->decode_tap : nullptr;
        fx.B = nb;
        HIP_TRY(launch_vae_fusedx(fx, d.st));
        return 0;
    });
}

// the row / attention launches.  fp32x: the row stages without split-K (k_vae_rows8.hip; FUSED) or the split-K row kernel k_vae_rows<f16x2> (STAGED), chosen from the
// clips of the CALL (not of the chunk: a job's last chunk must not change kernels) or as amuse_set_decode_path pins it, so that a job-level choice (amuse_plan) keeps
// fp32x shards bitwise too.  Train-mode decode: the six dropout sites of every block live - per-head cross-attention partials, the dropout instantiations of the row
// and attention kernels
int decode_staged(amuse_ctx* c, const DecodeCall& d, bool rows8, bool drop) {
    const int chunk = d.B < kVaeChunk ? d.B : kVaeChunk;
    if (int e = ensure_vae_ws(c, chunk)) return e;
    // fp32x row stages, all clips full length: block 0's self-attention half is one [300][128] constant per weight set (see decode_fused16) - computed once by these
    // kernels themselves on one clip (a tile's arithmetic does not depend on its launch: same bits), then every decode starts at stage 1 behind norm1.  Explicit
    // lengths (even all 300) take the full path.
    const bool hoist = rows8 && !d.lengths;
    return for_chunks(d.B, chunk, [&](int b0, int nb) -> int {
        const StageWs w = carve_stage_ws(c->vae_ws, (size_t)nb * kFrames);
        StageArgs a = decode_stage_args(c, d, b0, nb, w);
        HIP_TRY(decode_ca(c, d.z + (size_t)b0 * kD, !drop, w.tail, nb, d.st));
        if (drop) {   // clip b of this chunk is global clip clip0 + b0 + b
            VaeDropArgs da{};
            da.drop_thr = c->dec_drop_thr; da.drop_scale = c->dec_drop_scale; da.drop_seed = c->dec_drop_seed;
            da.drop_clip0 = (uint32_t)(d.clip0 + (uint64_t)b0);
            a.rows.drop = a.attn.drop = da;
            a.rows.ca_bias = c->vae_bo;
            return run_stages(a, d.precision, {VAE_MODE_DEC_DROP, 0, 1, 0, VAE_MODE_DEC, false}, d.st);
        }
        twin_rows8(a, c->dec, rows8);
        if (hoist) {
            if (int e = produce_c1(c->c1_rows8, (size_t)kFrames * kD, d.st, [&]() -> int {
                    VaeRowsArgs p8 = a.rows8;
                    p8.B = 1; p8.lengths = nullptr; p8.feats_out = p8.poses_out = p8.trans_out = nullptr;
                    VaeAttnArgs pa = a.attn;
                    pa.B = 1; pa.lengths = nullptr;
                    p8.stage = 0;
                    HIP_TRY(launch_vae_rows8x(p8, d.st));
                    HIP_TRY(launch_vae_attn(pa, d.precision, VAE_MODE_DEC, d.st));
                    p8.stage = 1; p8.c1_out = c->c1_rows8.buf;
                    HIP_TRY(launch_vae_rows8x(p8, d.st));
                    return 0;
                }))
                return e;
            HIP_TRY(consume_c1(c->c1_rows8, d.st));
            a.rows8.c1 = c->c1_rows8.buf;
        }
        return run_stages(a, d.precision, {VAE_MODE_DEC, hoist ? 1 : 0, rows8 ? 0 : 1, rows8 ? 9 : 0, VAE_MODE_DEC, false}, d.st);
    });
}

// amuse_vae_decode: the checks and the choice of kernel family
int vae_decode(amuse_ctx* c, const float* z, const int* lengths, int B, int precision, int quat_mode,
               float* feats_out, float* poses_out, float* trans_out, void* stream, uint64_t clip0) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!c->has_prior) return fail(AMUSE_ESTATE, "this context was created without MotionPrior weights");
    if (!z) return fail(AMUSE_EINVAL, "z is NULL");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1, got %d", B);
    if (precision < AMUSE_PREC_F32 || precision > AMUSE_PREC_F16) return fail(AMUSE_EINVAL, "bad precision %d", precision);
    if (quat_mode != AMUSE_QUAT_P3D && quat_mode != AMUSE_QUAT_LEGACY) return fail(AMUSE_EINVAL, "bad quat_mode %d", quat_mode);
    if (int e = decode_dropout_refused(c, precision)) return e;
    HIP_TRY(hipSetDevice(c->device));
    const DecodeCall d{z, lengths, B, precision, quat_mode, feats_out, poses_out, trans_out, (hipStream_t)stream, clip0};
    if (int e = stage_lengths(c, lengths, B, false, d.st)) return e;
    // train-mode decode runs on the staged family at every clip count, whatever the pin says: the fused kernels and block 0's hoisted constant are eval-only
    const bool drop = c->dec_drop_thr > 0;
    const int path = drop ? (c->last_plan[1] = AMUSE_DECODE_STAGED) : decode_path_of(c, precision, B);
    if (is_op16(precision) && path != AMUSE_DECODE_STAGED) return decode_fused16(c, d);
    if (precision == PREC_F16X2 && path == AMUSE_DECODE_CLIP) return decode_clipx(c, d);
    return decode_staged(c, d, precision == PREC_F16X2 && path != AMUSE_DECODE_STAGED, drop);
}
}  // namespace

extern "C" {

int amuse_vae_decode(amuse_ctx* c, const float* z, const int* lengths, int B, int precision, int quat_mode,
                     float* feats_out, float* poses_out, float* trans_out, void* stream) {
    return vae_decode(c, z, lengths, B, precision, quat_mode, feats_out, poses_out, trans_out, stream, c ? c->dec_drop_clip0 : 0);
}

int amuse_vae_encode(amuse_ctx* c, const float* feats, const int* lengths, int B, int precision, const float* eps,
                     float* mu_out, float* std_out, float* latent_out, void* stream) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!c->has_prior) return fail(AMUSE_ESTATE, "this context was created without MotionPrior weights");
    if (!feats) return fail(AMUSE_EINVAL, "feats is NULL");
    if (!mu_out && !std_out && !latent_out) return fail(AMUSE_EINVAL, "no output requested");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1, got %d", B);
    if (precision < AMUSE_PREC_F32 || precision > AMUSE_PREC_F16) return fail(AMUSE_EINVAL, "bad precision %d", precision);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (int e = stage_lengths(c, lengths, B, false, st)) return e;
    const int chunk = B < kVaeChunk ? B : kVaeChunk;
    if (int e = ensure_vae_ws(c, chunk)) return e;
    // fp32x from kFusedMinClips clips of the call (or as amuse_set_decode_path pins it - the decode's rule): stages 1..9 on the row kernel without split-K (FUSED), or the
    // whole encoder as one persistent workgroup per clip (CLIP)
    const int epath = encode_path_of(c, precision, B);
    const bool rows8 = epath != AMUSE_DECODE_STAGED;
    return for_chunks(B, chunk, [&](int b0, int nb) -> int {
        const StageWs w = carve_stage_ws(c->vae_ws, (size_t)nb * kEncRows);
        StageArgs a = stage_args(c->enc, precision, w, nb);
        VaeRowsArgs& ra = a.rows;
        ra.tok = c->vaee_tok;
        ra.stats_out = w.tail;  // [nb][2][128] <= the decoder's [nb][9][128] cross-attention slot
        ra.lengths = a.attn.lengths = lengths ? c->d_lengths + b0 : nullptr;
        ra.enc_feats = feats + (size_t)b0 * kFrames * kFeats;
        if (epath == AMUSE_DECODE_CLIP) {
            DenFusedXArgs fx{};
            fx.wstream = c->enc.fusedx; fx.pvec = ra.pvec; fx.emb_bias = ra.emb_bias; fx.pe = ra.pe; fx.ttok = ra.tok;
            fx.x_in = ra.enc_feats; fx.eps_out = ra.stats_out; fx.lengths = ra.lengths; fx.obuf = w.attn_o; fx.skip = w.skip;
            fx.B = nb; fx.S = kEncRows; fx.npre = 2; fx.encode = 1;
            HIP_TRY(launch_den_fusedx(fx, st));
        } else {
            twin_rows8(a, c->enc, rows8);
            if (int e = run_stages(a, precision, {VAE_MODE_ENC, 0, 1, rows8 ? 9 : 0, VAE_MODE_ENC, true}, st)) return e;
        }
        HIP_TRY(launch_vae_latent(ra.stats_out, at_clip(eps, b0, kD), at_clip(mu_out, b0, kD), at_clip(std_out, b0, kD), at_clip(latent_out, b0, kD), nb, st));
        return 0;
    });
}

int amuse_smplx_to_feats(amuse_ctx* c, const float* poses, const float* trans, int B, float* feats_out, void* stream) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!poses || !trans || !feats_out) return fail(AMUSE_EINVAL, "NULL argument");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1, got %d", B);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_smplx_to_feats(poses, trans, (size_t)B * kFrames, feats_out, (hipStream_t)stream));
    return 0;
}

int amuse_diffusion_backward(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int precision,
                             int quat_mode, uint64_t seed, uint64_t clip_index0, const float* x_init,
                             const float* step_noise, float* latents_out, float* poses_out, float* trans_out,
                             void* stream) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!poses_out || !trans_out) return fail(AMUSE_EINVAL, "poses_out / trans_out is NULL");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1, got %d", B);
    if (!(c->arch & 2))   // (a latent-space context decodes: refuse a train-mode decode that cannot run before anything is launched)
        if (int e = decode_dropout_refused(c, precision)) return e;
    float* lat = latents_out;
    if (!lat) {
        HIP_TRY(hipSetDevice(c->device));
        if (int e = ensure(&c->lat_tmp, &c->lat_cap, (size_t)B * variant_state_dim(c->arch))) return e;
        lat = c->lat_tmp;
    }
    if (int e = amuse_sample(c, con, emo, sty, B, precision, seed, clip_index0, x_init, step_noise, lat, nullptr, stream))
        return e;
    // diffusion_only: the sampled state IS the feature sequence - no decode (infer_ldm.py:165), only the conversion of :168-173
    if (c->arch & 2) return amuse_feats_to_smplx(c, lat, B, quat_mode, poses_out, trans_out, stream);
    // (train-mode decode: the masks follow the sampler's clips - this call's clip_index0, not the setter's)
    return vae_decode(c, lat, nullptr, B, precision, quat_mode, nullptr, poses_out, trans_out, stream, clip_index0);
}

int amuse_counter_normal(amuse_ctx* c, uint64_t seed, uint64_t clip_index0, int B, int step, int rng_stream,
                         float* out, void* stream) {
    if (!c || !out) return fail(AMUSE_EINVAL, "NULL argument");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_counter_normal(seed, clip_index0, B, step, rng_stream, out, (hipStream_t)stream, (int)variant_state_dim(c->arch)));
    return 0;
}

int amuse_denoise_step_pose(amuse_ctx* c, const float* x_t, int timestep, const float* con, const float* emo, const float* sty,
                            const int* lengths, int B, int precision, float* eps_out, void* stream) {
    if (int e = check_common(c, con, B, precision)) return e;
    if (!(c->arch & 2)) return fail(AMUSE_ESTATE, "amuse_denoise_step_pose needs a pose-space variant (AMUSE_ARCH_ENC_POSE / _DEC_POSE)");
    if (!x_t || !eps_out) return fail(AMUSE_EINVAL, "x_t / eps_out is NULL");
    if (timestep < 0) return fail(AMUSE_EINVAL, "negative timestep");
    SampleArgs a{};
    if (int e = sample_dropout(c, precision, a)) return e;   // (always refused: a pose-space variant)
    return variant_denoise(c, x_t, &timestep, false, con, emo, sty, lengths, B, precision, eps_out, nullptr, (hipStream_t)stream);
}

int amuse_feats_to_smplx(amuse_ctx* c, const float* feats, int B, int quat_mode, float* poses_out, float* trans_out, void* stream) {
    if (!c) return fail(AMUSE_EINVAL, "ctx is NULL");
    if (!feats || (!poses_out && !trans_out)) return fail(AMUSE_EINVAL, "NULL argument");
    if (B < 1) return fail(AMUSE_EINVAL, "B must be >= 1, got %d", B);
    if (quat_mode != AMUSE_QUAT_P3D && quat_mode != AMUSE_QUAT_LEGACY) return fail(AMUSE_EINVAL, "bad quat_mode %d", quat_mode);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_feats_to_smplx(feats, (size_t)B * kFrames, quat_mode, poses_out, trans_out, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
