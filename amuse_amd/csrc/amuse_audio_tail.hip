// Host side of AST_EVP's tail (include/amuse_hip.h "Audio model metrics": amuse_audio_set_tail / amuse_audio_reconstruct / the labels of
// amuse_audio_encode_labels): the device images of the classifier heads, FusionBlock and DecoderBlock, the packer of the last Linear's weight stream and the
// launch sequence on the kernels of k_audio_tail.hip.  A translation unit of its own, reached from amuse_audio_api.hip through amuse_audio_tail_ops() only
// (amuse_audio_tail.hpp): a link without it has the encoders and refuses the tail's calls.  Error reporting (failf, HIP_TRY_P) and f2bf are those of
// amuse_audio_enc.hpp, shared with the encoders' units.  Host code only.
#include <hip/hip_runtime.h>

#include <vector>

#include "amuse_audio_enc.hpp"
#include "amuse_audio_tail.hpp"

using namespace amuse;

#define HIP_TRY(expr) HIP_TRY_P("audio tail: ", expr)

namespace {

// torch Linear weight [N][K] fp32 -> the skinny GEMM's unit order (amuse_audio_tail.hpp tail_pack_index / tail_pack_index_x); out: N * K (bf16) or 2 * N * K (hi | lo) x 16 bit
int pack_tail(const float* W, int N, int K, int precision, unsigned short* out) {
    const int KS = K / 32;
    if (precision == AMUSE_PREC_BF16) {
        for (int ft = 0; ft < N / 16; ++ft)
            for (int ks = 0; ks < KS; ++ks) {
                unsigned short* u = out + ((size_t)ft * KS + ks) * 512;
                for (int lane = 0; lane < 64; ++lane) {
                    const float* src = W + (size_t)(16 * ft + (lane & 15)) * K + 32 * ks + 8 * (lane >> 4);
                    for (int e = 0; e < 8; ++e) u[8 * lane + e] = f2bf(src[e]);
                }
            }
        return 0;
    }
    // the library's one fp32 -> (hi, lo) splitter, a feature tile (16 rows of W, contiguous) at a time
    std::vector<uint16_t> hi((size_t)16 * K), lo((size_t)16 * K);
    for (int ft = 0; ft < N / 16; ++ft) {
        if (int e = amuse_debug_f16_split(W + (size_t)16 * ft * K, (size_t)16 * K, hi.data(), lo.data())) return e;
        for (int ks = 0; ks < KS; ++ks) {
            unsigned short* u = out + ((size_t)ft * KS + ks) * 1024;
            for (int lane = 0; lane < 64; ++lane) {
                const size_t s = (size_t)(lane & 15) * K + 32 * ks + 8 * (lane >> 4);
                memcpy(u + 8 * lane, &hi[s], 16);
                memcpy(u + 512 + 8 * lane, &lo[s], 16);
            }
        }
    }
    return 0;
}

struct LayerT {   // nn.TransformerEncoderLayer, offsets into the trunk blob
    const float *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_w, *n1_b, *n2_w, *n2_b;
};
struct HeadT {
    const float *ln_w, *ln_b, *w, *b;
};
struct StateT {
    float* trunk = nullptr;                 // every parameter in front of decode.projection.2.weight, fp32, in the order of the flat array
    HeadT head[2][2];                       // [emo | sty][mlp_head | mlp_head_featbased]
    LayerT fus[kTailFusionLayers], dec[kTailDecodeLayers];
    const float *fus_nw, *fus_nb, *fus_fw, *fus_fb, *dec_nw, *dec_nb, *p0_w, *p0_b;
    float* p2_b = nullptr;                  // decode.projection.2.bias
    unsigned short *p2_bf16 = nullptr, *p2_x = nullptr;   // its weight stream: bf16 image (built by create), hi | lo image (built on the first use in AMUSE_PREC_F32X)
    std::vector<float> p2_host;             // until then: the host copy to build it from
    float *x = nullptr, *y = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr, *hid = nullptr;   // workspace of one pass over kTailRows rows
};

void t_destroy(void* state) {
    StateT* c = static_cast<StateT*>(state);
    if (!c) return;
    void* all[] = {c->trunk, c->p2_b, c->p2_bf16, c->p2_x, c->x, c->y, c->qkv, c->att, c->ff, c->hid};
    for (void* p : all)
        if (p) (void)hipFree(p);
    delete c;
}

int build(StateT* c, const float* params) {
    const size_t n_w2 = (size_t)kTailOut * kTailHidden, n_trunk = (size_t)AMUSE_AST_TAIL_PARAMS - n_w2 - kTailOut;
    HIP_TRY(hipMalloc((void**)&c->trunk, n_trunk * 4));
    HIP_TRY(hipMemcpy(c->trunk, params, n_trunk * 4, hipMemcpyHostToDevice));
    const float* p = c->trunk;
    auto take = [&](size_t n) { const float* q = p; p += n; return q; };
    const int labels[2] = {kTailLabelsEmo, kTailLabelsSty}, dims[2] = {kAstFeat, kAstDim};
    for (int e = 0; e < 2; ++e)
        for (int h = 0; h < 2; ++h) {
            HeadT& H = c->head[e][h];
            H.ln_w = take(dims[h]); H.ln_b = take(dims[h]); H.w = take((size_t)labels[e] * dims[h]); H.b = take(labels[e]);
        }
    auto layer = [&](LayerT& L, size_t D) {
        L.in_w = take(3 * D * D); L.in_b = take(3 * D); L.out_w = take(D * D); L.out_b = take(D);
        L.l1_w = take(kTailFF * D); L.l1_b = take(kTailFF); L.l2_w = take(D * kTailFF); L.l2_b = take(D);
        L.n1_w = take(D); L.n1_b = take(D); L.n2_w = take(D); L.n2_b = take(D);
    };
    for (LayerT& L : c->fus) layer(L, kTailFusionDim);
    c->fus_nw = take(kTailFusionDim); c->fus_nb = take(kTailFusionDim);
    c->fus_fw = take((size_t)kTailLatent * kTailFusionDim); c->fus_fb = take(kTailLatent);
    for (LayerT& L : c->dec) layer(L, kTailLatent);
    c->dec_nw = take(kTailLatent); c->dec_nb = take(kTailLatent);
    c->p0_w = take((size_t)kTailHidden * kTailLatent); c->p0_b = take(kTailHidden);
    if ((size_t)(p - c->trunk) != n_trunk) return failf(AMUSE_EINVAL, "audio tail: parameter walk ends at %s%ld, not %ld", "", (long)(p - c->trunk), (long)n_trunk);
    const float* w2 = params + n_trunk;
    HIP_TRY(hipMalloc((void**)&c->p2_b, (size_t)kTailOut * 4));
    HIP_TRY(hipMemcpy(c->p2_b, w2 + n_w2, (size_t)kTailOut * 4, hipMemcpyHostToDevice));
    {
        std::vector<unsigned short> img(n_w2);
        if (int e = pack_tail(w2, kTailOut, kTailHidden, AMUSE_PREC_BF16, img.data())) return e;
        HIP_TRY(hipMalloc((void**)&c->p2_bf16, n_w2 * 2));
        HIP_TRY(hipMemcpy(c->p2_bf16, img.data(), n_w2 * 2, hipMemcpyHostToDevice));
    }
    c->p2_host.assign(w2, w2 + n_w2);
    HIP_TRY(hipMalloc((void**)&c->x, (size_t)kTailRows * kTailFusionDim * 4));
    HIP_TRY(hipMalloc((void**)&c->y, (size_t)kTailRows * kTailFusionDim * 4));
    HIP_TRY(hipMalloc((void**)&c->qkv, (size_t)kTailRows * 3 * kTailFusionDim * 4));
    HIP_TRY(hipMalloc((void**)&c->att, (size_t)kTailRows * kTailFusionDim * 4));
    HIP_TRY(hipMalloc((void**)&c->ff, (size_t)kTailRows * kTailFF * 4));
    HIP_TRY(hipMalloc((void**)&c->hid, (size_t)kTailRows * kTailHidden * 4));
    return 0;
}
int t_create(void** state, const float* params) {
    StateT* c = new StateT();
    if (int e = build(c, params)) {
        t_destroy(c);
        return e;
    }
    *state = c;
    return 0;
}

// the hi | lo image of the last Linear, once (537 MB); the host copy is done after it
int ensure_x_image(StateT* c) {
    if (c->p2_x) return 0;
    const size_t n_w2 = (size_t)kTailOut * kTailHidden;
    if (c->p2_host.size() != n_w2) return failf(AMUSE_ESTATE, "audio tail: no host copy to build the AMUSE_PREC_F32X image from%s");
    std::vector<unsigned short> img(2 * n_w2);
    if (int e = pack_tail(c->p2_host.data(), kTailOut, kTailHidden, AMUSE_PREC_F32X, img.data())) return e;
    HIP_TRY(hipMalloc((void**)&c->p2_x, img.size() * 2));
    HIP_TRY(hipMemcpy(c->p2_x, img.data(), img.size() * 2, hipMemcpyHostToDevice));
    std::vector<float>().swap(c->p2_host);
    return 0;
}

// one post-norm nn.TransformerEncoderLayer over nb rows in groups of S: c->x -> c->x
int run_layer(const StateT* c, const LayerT& L, int nb, int S, int D, hipStream_t st) {
    HIP_TRY(launch_tail_linear(c->x, L.in_w, L.in_b, nb, 3 * D, D, 0, c->qkv, st));
    HIP_TRY(launch_tail_attn(c->qkv, nb, S, D, c->att, st));
    HIP_TRY(launch_tail_linear(c->att, L.out_w, L.out_b, nb, D, D, 0, c->y, st));
    HIP_TRY(launch_tail_add_ln(c->x, c->y, L.n1_w, L.n1_b, nb, D, c->x, st));
    HIP_TRY(launch_tail_linear(c->x, L.l1_w, L.l1_b, nb, kTailFF, D, 1, c->ff, st));
    HIP_TRY(launch_tail_linear(c->ff, L.l2_w, L.l2_b, nb, D, kTailFF, 0, c->y, st));
    HIP_TRY(launch_tail_add_ln(c->x, c->y, L.n2_w, L.n2_b, nb, D, c->x, st));
    return 0;
}

int t_reconstruct(void* state, int precision, const float* con, const float* emo, const float* sty, int B, int group, float* fbank_out, float* hidden_out,
                  hipStream_t st) {
    StateT* c = static_cast<StateT*>(state);
    if (fbank_out && precision == AMUSE_PREC_F32X)
        if (int e = ensure_x_image(c)) return e;
    const int chunk = kTailRows / group * group;   // whole groups only: a row's bits depend on its group alone
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0) < chunk ? (B - b0) : chunk;
        const size_t o = (size_t)b0 * kAstFeat;
        HIP_TRY(launch_tail_cat(emo + o, sty + o, con + o, nb, c->x, st));
        for (const LayerT& L : c->fus)
            if (int e = run_layer(c, L, nb, group, kTailFusionDim, st)) return e;
        HIP_TRY(launch_tail_add_ln(c->x, nullptr, c->fus_nw, c->fus_nb, nb, kTailFusionDim, c->y, st));
        HIP_TRY(launch_tail_linear(c->y, c->fus_fw, c->fus_fb, nb, kTailLatent, kTailFusionDim, 0, c->x, st));
        for (const LayerT& L : c->dec)
            if (int e = run_layer(c, L, nb, group, kTailLatent, st)) return e;
        HIP_TRY(launch_tail_add_ln(c->x, nullptr, c->dec_nw, c->dec_nb, nb, kTailLatent, c->y, st));
        float* hid = hidden_out ? hidden_out + (size_t)b0 * kTailHidden : c->hid;
        HIP_TRY(launch_tail_linear(c->y, c->p0_w, c->p0_b, nb, kTailHidden, kTailLatent, 1, hid, st));
        if (fbank_out) {
            TailGemmArgs g{};
            g.A = hid; g.W = precision == AMUSE_PREC_F32X ? c->p2_x : c->p2_bf16; g.bias = c->p2_b; g.B = nb; g.N = kTailOut; g.K = kTailHidden;
            g.out = fbank_out + (size_t)b0 * kTailOut;
            HIP_TRY(launch_tail_gemm(g, precision, st));
        }
    }
    return 0;
}

int t_labels(void* state, int which, int frame_based, const float* in, int B, float* logits, hipStream_t st) {
    const StateT* c = static_cast<StateT*>(state);
    const int e = which == AMUSE_AUDIO_EMO ? 0 : 1, L = e ? kTailLabelsSty : kTailLabelsEmo;
    const HeadT& H = c->head[e][frame_based ? 1 : 0];
    if (frame_based) HIP_TRY(launch_tail_head(in, kAstPoolSplit, 0.5f, kAstDim, H.ln_w, H.ln_b, H.w, H.b, L, logits, B, st));
    else HIP_TRY(launch_tail_head(in, 0, 1.0f, kAstFeat, H.ln_w, H.ln_b, H.w, H.b, L, logits, B, st));
    return 0;
}

const AudioTailOps kOps = {t_create, t_destroy, t_reconstruct, t_labels};

bool bad_gemm_shape(int N, int K) { return N < kTailSpan || N % kTailSpan || K < 64 || K % 64 || K > kTailMaxK; }

}  // namespace

extern "C" {

const amuse::AudioTailOps* amuse_audio_tail_ops(void) { return &kOps; }

int amuse_debug_tail_pack(const float* W, int N, int K, int precision, void* out) {
    if (!W || !out) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (bad_gemm_shape(N, K)) return failf(AMUSE_EINVAL, "%sbad tail GEMM shape (N %ld K %ld): N %% 256 == 0, K %% 64 == 0, 64 <= K <= 1024", "", N, K);
    if (precision != AMUSE_PREC_BF16 && precision != AMUSE_PREC_F32X) return failf(AMUSE_EINVAL, "%sprecision %ld is neither AMUSE_PREC_BF16 nor AMUSE_PREC_F32X", "", precision);
    return pack_tail(W, N, K, precision, static_cast<unsigned short*>(out));
}

int amuse_debug_tail_gemm(const float* A, const void* W_packed, const float* bias, int B, int N, int K, int precision, float* out, void* stream) {
    if (!A || !W_packed || !bias || !out) return failf(AMUSE_EINVAL, "NULL argument%s");
    if (B < 1 || bad_gemm_shape(N, K)) return failf(AMUSE_EINVAL, "%sbad tail GEMM shape (N %ld K %ld): B >= 1, N %% 256 == 0, K %% 64 == 0, 64 <= K <= 1024", "", N, K);
    if (precision != AMUSE_PREC_BF16 && precision != AMUSE_PREC_F32X) return failf(AMUSE_EINVAL, "%sprecision %ld is neither AMUSE_PREC_BF16 nor AMUSE_PREC_F32X", "", precision);
    for (int b0 = 0; b0 < B; b0 += kTailRows) {
        TailGemmArgs g{};
        g.A = A + (size_t)b0 * K; g.W = W_packed; g.bias = bias; g.B = (B - b0) < kTailRows ? (B - b0) : kTailRows; g.N = N; g.K = K;
        g.out = out + (size_t)b0 * N;
        HIP_TRY(launch_tail_gemm(g, precision, (hipStream_t)stream));
    }
    return 0;
}

}  // extern "C"
