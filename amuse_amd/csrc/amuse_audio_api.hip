// C ABI of the audio front-end (include/amuse_hip.h, "Audio front-end"): the context, and the bf16 mode of the AST encoder described in amuse_audio_enc.hpp -
// what it uploads for a parameter and how an operand becomes the arguments of the kernels of k_audio.hip / k_audio_gemm.hip.  Host code only.
#include <hip/hip_runtime.h>

#include <vector>

#include "amuse_audio_enc.hpp"
#include "amuse_audio_tail.hpp"
#include "amuse_audio_x.hpp"

using namespace amuse;

// The parity mode (AMUSE_PREC_F32X) lives in amuse_audio_x.hip and is reached through this WEAK reference only: where that unit is not linked (the host-only
// build of tests/host_asan, whose stub defines the bf16 launchers alone) the address is null and amuse_audio_set_precision refuses the mode.
extern "C" const amuse::AudioModeOps* amuse_audio_x_ops(void) __attribute__((weak));
// AST_EVP's tail (classifier heads, fusion, decoder: amuse_audio_tail.hip) is reached the same way: without that unit amuse_audio_set_tail, amuse_audio_reconstruct
// and the labels of amuse_audio_encode_labels return AMUSE_ESTATE.
extern "C" const amuse::AudioTailOps* amuse_audio_tail_ops(void) __attribute__((weak));

#define HIP_TRY(expr) HIP_TRY_P("", expr)   // (this unit's messages carry no prefix)

namespace {

// torch Linear weight [N][K] fp32 -> the GEMM's fragment order (amuse_audio.hpp GemmArgs::W), bf16
void pack_w(const float* W, int N, int K, unsigned short* out) {
    for_each_fragment_lane(N, K, [&](size_t u, int lane, size_t s) {
        for (int e = 0; e < 8; ++e) out[(u * 64 + lane) * 8 + e] = f2bf(W[s + e]);
    });
}

struct Bf16Mode {
    static constexpr int planes = 1;
    static constexpr const char* err_prefix = "";
    struct Scratch { std::vector<unsigned short> img; };
    // GEMM weights fragment-packed bf16, the feature head's weight plain bf16 [256][768]
    static int put(AstState<Bf16Mode>* c, void* slot, const float* src, const AstParam& p) {
        const size_t n = (size_t)p.rows * p.cols;
        if (p.kind == PK_F32) return c->up.up(slot, src, n * 4);
        std::vector<unsigned short>& h = c->scratch.img;
        h.resize(n);
        if (p.kind == PK_GEMM_W) pack_w(src, p.rows, p.cols, h.data());
        else for (size_t i = 0; i < n; ++i) h[i] = f2bf(src[i]);
        return c->up.up(slot, h.data(), n * 2);
    }
    static hipError_t im2col(const float* fbank, Operand P, int nb, hipStream_t st) { return launch_im2col(fbank, P.hi, nb, st); }
    static hipError_t ln(const float* X, const float* gamma, const float* beta, float eps, Operand out, int M, hipStream_t st) {
        return launch_ln_bf16(X, gamma, beta, eps, out.hi, M, st);
    }
    static hipError_t gemm(int epi, Operand A, const unsigned short* W, const float* bias, int M, int N, int K, Operand out, float* out_f32, const float* pos, Operand vt,
                           hipStream_t st) {
        GemmArgs g{};
        g.A = A.hi; g.W = W; g.bias = bias; g.M = M; g.N = N; g.K = K; g.out_bf16 = out.hi; g.out_f32 = out_f32; g.pos = pos; g.vt = vt.hi;
        return launch_gemm(g, epi, st);
    }
    static hipError_t attn(Operand QK, Operand Vt, Operand O, int nb, hipStream_t st) { return launch_ast_attn(QK.hi, Vt.hi, O.hi, nb, st); }
    static hipError_t head(const float* pooled, int frame_based, const Encoder& E, float* out, int nb, hipStream_t st) {
        return launch_ast_head(pooled, frame_based, E.fh_ln_w, E.fh_ln_b, static_cast<const unsigned short*>(E.fh_w), E.fh_b, out, nb, st);
    }
};

constexpr int kChunk = 32;   // clips per pass over the network (about 22 MB of workspace per clip)
// One mode of the encoders: its functions and what they built.  [0] bf16, built by amuse_audio_create; [1] fp32x, built on the first switch to AMUSE_PREC_F32X
struct ModeSlot {
    const AudioModeOps* ops = nullptr;
    void* state = nullptr;
};

}  // namespace

struct amuse_audio_ctx {
    int device = 0;
    int frame_based = 1;
    float norm_mean = 0.f, norm_std = 1.f;
    float *melw = nullptr, *window = nullptr;   // melw: the mel filter bank TRANSPOSED, [257 bins][128 filters]
    int* mel_range = nullptr;                   // [128][2]: first / end bin of each filter's support
    Uploader consts;             // owns melw, window, mel_range
    ModeSlot mode[2];
    const ModeSlot& cur() const { return mode[precision == AMUSE_PREC_F32X]; }   // the mode of `precision`
    float* fbank = nullptr;      // fbanks of one chunk
    int fbank_cap = 0;
    hipStream_t side[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    // amuse_audio_set_precision: the mode and, until the parity mode is built, a host copy of the three parameter arrays to build it from (the device holds
    // bf16 images only)
    int precision = AMUSE_PREC_BF16;
    std::vector<float> host_params[3];
    // amuse_audio_set_tail: the tail's state (amuse_audio_tail.hip) and the second pooling buffer of amuse_audio_encode_labels ((cls + dist) row sums of a chunk)
    void* tail = nullptr;
    float* pooled2 = nullptr;
    int pooled2_cap = 0;
};

namespace {

int ensure_fbank(amuse_audio_ctx* c, int nb) {
    if (c->fbank_cap >= nb) return 0;
    if (c->fbank) HIP_TRY(hipFree(c->fbank));
    c->fbank = nullptr; c->fbank_cap = 0;
    HIP_TRY(hipMalloc((void**)&c->fbank, (size_t)nb * kAstFrames * kAstMel * 4));
    c->fbank_cap = nb;
    return 0;
}
int ensure_side_streams(amuse_audio_ctx* c) {
    if (c->ev_fork) return 0;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    return 0;
}

int ensure_pooled2(amuse_audio_ctx* c, int nb) {
    if (c->pooled2_cap >= nb) return 0;
    if (c->pooled2) HIP_TRY(hipFree(c->pooled2));
    c->pooled2 = nullptr; c->pooled2_cap = 0;
    HIP_TRY(hipMalloc((void**)&c->pooled2, (size_t)nb * kAstPoolSplit * kAstDim * 4));
    c->pooled2_cap = nb;
    return 0;
}

}  // namespace

extern "C" {

amuse_audio_ctx* amuse_audio_create(int device, const float* con_params, const float* emo_params, const float* sty_params,
                                    size_t n_each, const float* mel_banks, const float* window, float norm_mean,
                                    float norm_std, int frame_based_feats) {
    if (!con_params || !emo_params || !sty_params || !mel_banks || !window) {
        failf(AMUSE_EINVAL, "NULL argument%s");
        return nullptr;
    }
    if (n_each != AMUSE_AST_PARAMS) {
        failf(AMUSE_EINVAL, "%sparameter count mismatch: %ld per encoder (want %ld)", "", (long)n_each, (long)AMUSE_AST_PARAMS);
        return nullptr;
    }
    if (!(norm_std > 0.f)) {
        failf(AMUSE_EINVAL, "norm_std must be positive%s");
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        failf(AMUSE_EHIP, "hipSetDevice(%s%ld) failed", "", device);
        return nullptr;
    }
    amuse_audio_ctx* c = new amuse_audio_ctx();
    c->device = device;
    c->frame_based = frame_based_feats ? 1 : 0;
    c->norm_mean = norm_mean;
    c->norm_std = norm_std;
    const float* ps[3] = {con_params, emo_params, sty_params};
    // device image of the filter bank: transposed (a bin's 128 weights contiguous) + each filter's support
    std::vector<float> mel_t((size_t)257 * kAstMel);
    std::vector<int> mel_rng(2 * kAstMel);
    for (int m = 0; m < kAstMel; ++m) {
        int k0 = 257, k1 = 0;
        for (int k = 0; k < 257; ++k) {
            const float w = mel_banks[(size_t)m * 257 + k];
            mel_t[(size_t)k * kAstMel + m] = w;
            if (w != 0.f) { if (k < k0) k0 = k; k1 = k + 1; }
        }
        mel_rng[2 * m] = k0 < k1 ? k0 : 0;
        mel_rng[2 * m + 1] = k0 < k1 ? k1 : 0;
    }
    c->mode[0].ops = &kAudioModeOps<Bf16Mode>;
    int rc = c->consts.up(&c->melw, mel_t.data(), mel_t.size() * 4) || c->consts.up(&c->window, window, 400 * 4) ||
             c->consts.up(&c->mel_range, mel_rng.data(), mel_rng.size() * 4) || c->mode[0].ops->create(&c->mode[0].state, ps);
    if (!rc && amuse_audio_x_ops)   // (a link without the parity mode never needs them)
        for (int e = 0; e < 3; ++e) c->host_params[e].assign(ps[e], ps[e] + n_each);
    if (rc) {
        amuse_audio_destroy(c);
        return nullptr;
    }
    return c;
}

void amuse_audio_destroy(amuse_audio_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    c->consts.free_all();
    for (ModeSlot& m : c->mode)
        if (m.state) m.ops->destroy(m.state);
    if (c->tail) amuse_audio_tail_ops()->destroy(c->tail);
    if (c->pooled2) (void)hipFree(c->pooled2);
    if (c->fbank) (void)hipFree(c->fbank);
    for (int i = 0; i < 2; ++i) {
        if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    delete c;
}

int amuse_audio_fbank(amuse_audio_ctx* c, const float* waves, int n_samples, int B, float* fbank_out, void* stream) {
    if (!c || !waves || !fbank_out) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (B < 1 || n_samples < 1) return failf(AMUSE_EINVAL, "%sB and n_samples must be >= 1 (got %ld, %ld)", "", B, n_samples);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_fbank(waves, n_samples, B, c->window, c->melw, c->mel_range, c->norm_mean, c->norm_std, fbank_out, (hipStream_t)stream));
    return 0;
}

int amuse_audio_encode(amuse_audio_ctx* c, int which, const float* fbank, int B, float* feat_out, float* hidden_out,
                       int tap_block, void* stream) {
    if (!c || !fbank || !feat_out) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (which < 0 || which > 2) return failf(AMUSE_EINVAL, "%sencoder index %ld not in 0..2", "", which);
    if (B < 1) return failf(AMUSE_EINVAL, "%sB must be >= 1, got %ld", "", B);
    if (hidden_out && (tap_block < 0 || tap_block >= kAstLayers)) return failf(AMUSE_EINVAL, "%stap_block %ld not in 0..11", "", tap_block);
    HIP_TRY(hipSetDevice(c->device));
    const ModeSlot& m = c->cur();
    const int chunk = B < kChunk ? B : kChunk;
    if (int e = m.ops->ensure_ws(m.state, 0, chunk)) return e;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0) < chunk ? (B - b0) : chunk;
        if (int e = m.ops->run_encoder(m.state, 0, which, c->frame_based, fbank + (size_t)b0 * kAstFrames * kAstMel, nb, feat_out + (size_t)b0 * kAstFeat,
                                hidden_out ? hidden_out + (size_t)b0 * kAstTokens * kAstDim : nullptr, tap_block, (hipStream_t)stream))
            return e;
    }
    return 0;
}

// amuse_audio_features runs the three encoders (independent networks over the same fbank) concurrently, each on its own
// stream and workspace: at small batches one encoder's launches leave most of the chip idle (10 row tiles of 128 tokens per
// clip against 512 persistent workgroup slots), at large ones the other encoders' work fills the tail of every launch.
int amuse_audio_features(amuse_audio_ctx* c, const float* waves, int n_samples, int B, float* con_out, float* emo_out,
                         float* sty_out, void* stream) {
    if (!c || !waves) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (B < 1 || n_samples < 1) return failf(AMUSE_EINVAL, "%sB and n_samples must be >= 1 (got %ld, %ld)", "", B, n_samples);
    HIP_TRY(hipSetDevice(c->device));
    const ModeSlot& m = c->cur();
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < kChunk ? B : kChunk;
    float* outs[3] = {con_out, emo_out, sty_out};
    if (int e = ensure_fbank(c, chunk)) return e;
    if (int e = ensure_side_streams(c)) return e;
    for (int e = 0; e < 3; ++e)
        if (outs[e])
            if (int rc = m.ops->ensure_ws(m.state, e, chunk)) return rc;
    // per chunk: fbank on `st`, then a fork-join over two side streams (stream-ordered with `st` through events, so the
    // call stays asynchronous and capturable): encoder e on stream e with workspace e
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0) < chunk ? (B - b0) : chunk;
        HIP_TRY(launch_fbank(waves + (size_t)b0 * n_samples, n_samples, nb, c->window, c->melw, c->mel_range, c->norm_mean, c->norm_std, c->fbank, st));
        HIP_TRY(hipEventRecord(c->ev_fork, st));
        for (int e = 1; e < 3; ++e) {
            if (!outs[e]) continue;
            HIP_TRY(hipStreamWaitEvent(c->side[e - 1], c->ev_fork, 0));
            if (int rc = m.ops->run_encoder(m.state, e, e, c->frame_based, c->fbank, nb, outs[e] + (size_t)b0 * kAstFeat, nullptr, 0, c->side[e - 1])) return rc;
            HIP_TRY(hipEventRecord(c->ev_join[e - 1], c->side[e - 1]));
        }
        if (outs[0])
            if (int rc = m.ops->run_encoder(m.state, 0, 0, c->frame_based, c->fbank, nb, outs[0] + (size_t)b0 * kAstFeat, nullptr, 0, st)) return rc;
        for (int e = 1; e < 3; ++e)
            if (outs[e]) HIP_TRY(hipStreamWaitEvent(st, c->ev_join[e - 1], 0));   // (also: the next chunk's fbank overwrites c->fbank)
    }
    return 0;
}

int amuse_audio_set_tail(amuse_audio_ctx* c, const float* tail_params, size_t n) {
    if (!c || !tail_params) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (n != AMUSE_AST_TAIL_PARAMS) return failf(AMUSE_EINVAL, "%stail parameter count mismatch: %ld (want %ld)", "", (long)n, (long)AMUSE_AST_TAIL_PARAMS);
    if (!amuse_audio_tail_ops) return failf(AMUSE_ESTATE, "the audio model's tail (amuse_audio_tail) is not linked into this build%s");
    HIP_TRY(hipSetDevice(c->device));
    void* fresh = nullptr;
    if (int e = amuse_audio_tail_ops()->create(&fresh, tail_params)) return e;
    if (c->tail) amuse_audio_tail_ops()->destroy(c->tail);
    c->tail = fresh;
    return 0;
}

int amuse_audio_encode_labels(amuse_audio_ctx* c, int which, int frame_based, const float* fbank, int B, float* feat_out, float* logits_out, void* stream) {
    if (!c || !fbank || !feat_out) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (which < 0 || which > 2) return failf(AMUSE_EINVAL, "%sencoder index %ld not in 0..2", "", which);
    if (B < 1) return failf(AMUSE_EINVAL, "%sB must be >= 1, got %ld", "", B);
    if (logits_out && which == AMUSE_AUDIO_CON) return failf(AMUSE_EINVAL, "the content encoder has no classifier head (label_dim 0): logits_out must be NULL%s");
    if (logits_out && !amuse_audio_tail_ops) return failf(AMUSE_ESTATE, "the audio model's tail (amuse_audio_tail) is not linked into this build%s");
    if (logits_out && !c->tail) return failf(AMUSE_ESTATE, "no tail set: call amuse_audio_set_tail before asking for labels%s");
    const int fb = frame_based < 0 ? c->frame_based : (frame_based ? 1 : 0);
    const int L = which == AMUSE_AUDIO_EMO ? kTailLabelsEmo : kTailLabelsSty;
    HIP_TRY(hipSetDevice(c->device));
    const ModeSlot& m = c->cur();
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < kChunk ? B : kChunk;
    if (int e = m.ops->ensure_ws(m.state, 0, chunk)) return e;
    if (logits_out && fb)
        if (int e = ensure_pooled2(c, chunk)) return e;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0) < chunk ? (B - b0) : chunk;
        float* feat = feat_out + (size_t)b0 * kAstFeat;
        if (int e = m.ops->run_encoder(m.state, 0, which, fb, fbank + (size_t)b0 * kAstFrames * kAstMel, nb, feat, nullptr, 0, st)) return e;
        if (!logits_out) continue;
        // frame-based: the labels come from (cls + dist) / 2 of the final norm - the pooling the features did NOT take: v.norm and k_ast_pool (frame_based 0) again,
        // over the residual stream run_encoder left in the workspace, into a second buffer
        if (fb)
            if (int e = m.ops->pool(m.state, 0, which, 0, c->pooled2, nb, st)) return e;
        if (int e = amuse_audio_tail_ops()->labels(c->tail, which, fb, fb ? c->pooled2 : feat, nb, logits_out + (size_t)b0 * L, st)) return e;
    }
    return 0;
}

namespace {
int reconstruct_checked(amuse_audio_ctx* c, const float* con, const float* emo, const float* sty, int B, int group, float* fbank_out, float* hidden_out, void* stream) {
    if (!c || !con || !emo || !sty || (!fbank_out && !hidden_out)) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (B < 1 || group < 1 || group > kTailMaxGroup || B % group)
        return failf(AMUSE_EINVAL, "%sgroup must be in 1..16 and divide B (B %ld, group %ld)", "", B, group);
    if (!amuse_audio_tail_ops) return failf(AMUSE_ESTATE, "the audio model's tail (amuse_audio_tail) is not linked into this build%s");
    if (!c->tail) return failf(AMUSE_ESTATE, "no tail set: call amuse_audio_set_tail first%s");
    HIP_TRY(hipSetDevice(c->device));
    return amuse_audio_tail_ops()->reconstruct(c->tail, c->precision, con, emo, sty, B, group, fbank_out, hidden_out, (hipStream_t)stream);
}
}  // namespace

int amuse_audio_reconstruct(amuse_audio_ctx* c, const float* con, const float* emo, const float* sty, int B, int group, float* fbank_out, void* stream) {
    if (!fbank_out) return failf(AMUSE_EINVAL, "NULL argument%s");
    return reconstruct_checked(c, con, emo, sty, B, group, fbank_out, nullptr, stream);
}
int amuse_debug_tail_hidden(amuse_audio_ctx* c, const float* con, const float* emo, const float* sty, int B, int group, float* hidden_out, void* stream) {
    if (!hidden_out) return failf(AMUSE_EINVAL, "NULL argument%s");
    return reconstruct_checked(c, con, emo, sty, B, group, nullptr, hidden_out, stream);
}

int amuse_audio_set_precision(amuse_audio_ctx* c, int precision) {
    if (!c) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (precision != AMUSE_PREC_BF16 && precision != AMUSE_PREC_F32X)
        return failf(AMUSE_EINVAL, "%saudio precision %ld is neither AMUSE_PREC_BF16 nor AMUSE_PREC_F32X", "", precision);
    ModeSlot& x = c->mode[1];
    if (precision == AMUSE_PREC_F32X && !x.state) {
        if (!amuse_audio_x_ops)
            return failf(AMUSE_ESTATE, "the audio front-end's AMUSE_PREC_F32X mode (amuse_audio_x) is not linked into this build%s");
        HIP_TRY(hipSetDevice(c->device));
        const float* const ps[3] = {c->host_params[0].data(), c->host_params[1].data(), c->host_params[2].data()};
        if (int e = amuse_audio_x_ops()->create(&x.state, ps)) return e;
        x.ops = amuse_audio_x_ops();
        for (std::vector<float>& v : c->host_params) std::vector<float>().swap(v);   // the images are built once: the host copy is done
    }
    c->precision = precision;
    return 0;
}
int amuse_audio_precision(const amuse_audio_ctx* c) { return c ? c->precision : AMUSE_EINVAL; }

// GEMM in isolation (tools/gpu_gemm_bench.py, tests): C = A . W^T + bias with epilogue 0 (bf16 out) or 3 (fp32 out);
// A dev bf16 TILE-MAJOR [M padded to 128][K] (amuse_debug_tile), W dev bf16 in the kernel's packed fragment order
// (GemmArgs::W), out tile-major [M padded to 128][N]
int amuse_debug_gemm(const void* A, const void* W, const float* bias, int M, int N, int K, int epi, void* out, void* stream) {
    if (!A || !W || !bias || !out) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (M < 1 || N % kGemmTN || K % 64 || (epi != EPI_BF16 && epi != EPI_F32)) return failf(AMUSE_EINVAL, "%sbad GEMM shape / epilogue (N %ld K %ld)", "", N, K);
    GemmArgs g{};
    g.A = (const unsigned short*)A; g.W = (const unsigned short*)W; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.out_bf16 = (unsigned short*)out; g.out_f32 = (float*)out;
    HIP_TRY(launch_gemm(g, epi, (hipStream_t)stream));
    return 0;
}

// what 0: bf16 row-major [M][F] -> tile-major [M padded to 128][F] (pad rows zeroed); 1: bf16 tile-major -> row-major [M][F];
// 2: fp32 tile-major -> row-major [M][F]
int amuse_debug_tile(const void* src, void* dst, int M, int F, int what, void* stream) {
    if (!src || !dst) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (M < 1 || F < 32 || F % 32 || what < 0 || what > 2) return failf(AMUSE_EINVAL, "%sbad shape / direction (F %ld what %ld)", "", F, what);
    hipStream_t st = (hipStream_t)stream;
    if (what == 0) HIP_TRY(launch_tile_bf16((const unsigned short*)src, (unsigned short*)dst, M, F, st));
    else if (what == 1) HIP_TRY(launch_untile_bf16((const unsigned short*)src, (unsigned short*)dst, M, F, st));
    else HIP_TRY(launch_untile_f32((const float*)src, (float*)dst, M, F, M, M, st));
    return 0;
}

}  // extern "C"
