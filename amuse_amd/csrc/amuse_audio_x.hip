// Host side of the audio front-end's parity mode (include/amuse_hip.h amuse_audio_set_precision, AMUSE_PREC_F32X): the split-fp16 weight
// images, the doubled activation workspace and the launch sequence of one AST encoder on the kernels of k_audio_gemm_x.hip / k_audio_x.hip.
// A translation unit of its own, reached from amuse_audio_api.hip through amuse_audio_x_ops() only (amuse_audio_x.hpp): a link without it
// has the bf16 mode and refuses this one.  Host code only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_audio_x.hpp"

using namespace amuse;

int amuse_fail_msg(int code, const char* msg);   // amuse_api.hip: the library's thread-local error slot

namespace {

int failf(int code, const char* fmt, const char* a = "", long b = 0) {
    char buf[400];
    snprintf(buf, sizeof(buf), fmt, a, b);
    return amuse_fail_msg(code, buf);
}
#define HIP_TRY(expr)                                                                                               \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) return failf(AMUSE_EHIP, "audio fp32x: %s (line %ld)", hipGetErrorString(e_), __LINE__); \
    } while (0)

struct BlockX {
    float *n1w, *n1b, *n2w, *n2b, *qkv_b, *proj_b, *fc1_b, *fc2_b;
    unsigned short *qkv_w, *proj_w, *fc1_w, *fc2_w;   // hi | lo unit pairs
};
struct EncoderX {
    float *cls, *dist, *pos, *patch_b, *norm_w, *norm_b, *fh_ln_w, *fh_ln_b, *fh_b, *fh_wt;   // fh_wt: feature_head weight transposed [768][256], fp32
    unsigned short* patch_w;
    BlockX blk[kAstLayers];
};
// activations of one encoder pass over `cap` clips; an operand matrix is two planes: lo = hi + (its element count)
struct WorkspaceX {
    int cap = 0;
    float *X = nullptr, *pooled = nullptr;
    unsigned short *H = nullptr, *QK = nullptr, *Vt = nullptr, *O = nullptr, *F = nullptr, *P = nullptr;
    size_t nH = 0, nQK = 0, nVt = 0, nF = 0, nP = 0;   // elements per plane (O as H)
};
struct StateX {
    EncoderX enc[3];
    std::vector<void*> owned;
    WorkspaceX ws[3];
};

int up_f32(StateX* c, float** dst, const float* src, size_t n) {
    HIP_TRY(hipMalloc((void**)dst, n * sizeof(float)));
    c->owned.push_back(*dst);
    HIP_TRY(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
// torch Linear weight [N][K] fp32 -> the fragment order of amuse_audio_api.hip pack_w with every unit [64 lanes][8] doubled: hi, then lo.
// The split is amuse_debug_f16_split's (the library's one fp32 -> (hi, lo) splitter), taken over the whole matrix before the permutation.
int up_packed_x(StateX* c, unsigned short** dst, const float* W, int N, int K, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo,
                std::vector<unsigned short>& img) {
    const size_t n = (size_t)N * K;
    hi.resize(n);
    lo.resize(n);
    img.resize(2 * n);
    if (int e = amuse_debug_f16_split(W, n, hi.data(), lo.data())) return e;
    size_t o = 0;
    for (int sp = 0; sp < N / 64; ++sp)
        for (int x = 0; x < 4; ++x)
            for (int ks = 0; ks < K / 32; ++ks) {
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15;
                    const int f = 64 * sp + 32 * (x >> 1) + 8 * (i >> 2) + 4 * (x & 1) + (i & 3);
                    const size_t s = (size_t)f * K + 32 * ks + 8 * g;
                    memcpy(&img[o + 8 * lane], &hi[s], 16);
                    memcpy(&img[o + 512 + 8 * lane], &lo[s], 16);
                }
                o += 1024;
            }
    HIP_TRY(hipMalloc((void**)dst, img.size() * 2));
    c->owned.push_back(*dst);
    HIP_TRY(hipMemcpy(*dst, img.data(), img.size() * 2, hipMemcpyHostToDevice));
    return 0;
}

// the parameter order of amuse_audio_api.hip build_encoder (amuse_amd/audio_weights.py ast_param_spec)
int build_encoder_x(StateX* c, EncoderX& E, const float* p) {
    const size_t D = kAstDim;
    std::vector<uint16_t> hi, lo;
    std::vector<unsigned short> img;
    auto take = [&](size_t n) { const float* q = p; p += n; return q; };
    auto packed = [&](unsigned short** dst, const float* W, int N, int K) { return up_packed_x(c, dst, W, N, K, hi, lo, img); };
    if (up_f32(c, &E.cls, take(D), D) || up_f32(c, &E.dist, take(D), D) ||
        up_f32(c, &E.pos, take((size_t)kAstTokens * D), (size_t)kAstTokens * D) ||
        packed(&E.patch_w, take(D * 256), (int)D, 256) || up_f32(c, &E.patch_b, take(D), D))
        return AMUSE_EHIP;
    for (int l = 0; l < kAstLayers; ++l) {
        BlockX& b = E.blk[l];
        if (up_f32(c, &b.n1w, take(D), D) || up_f32(c, &b.n1b, take(D), D) ||
            packed(&b.qkv_w, take(3 * D * D), (int)(3 * D), (int)D) || up_f32(c, &b.qkv_b, take(3 * D), 3 * D) ||
            packed(&b.proj_w, take(D * D), (int)D, (int)D) || up_f32(c, &b.proj_b, take(D), D) ||
            up_f32(c, &b.n2w, take(D), D) || up_f32(c, &b.n2b, take(D), D) ||
            packed(&b.fc1_w, take((size_t)kAstMlp * D), kAstMlp, (int)D) || up_f32(c, &b.fc1_b, take(kAstMlp), kAstMlp) ||
            packed(&b.fc2_w, take(D * kAstMlp), (int)D, kAstMlp) || up_f32(c, &b.fc2_b, take(D), D))
            return AMUSE_EHIP;
    }
    if (up_f32(c, &E.norm_w, take(D), D) || up_f32(c, &E.norm_b, take(D), D) || up_f32(c, &E.fh_ln_w, take(D), D) || up_f32(c, &E.fh_ln_b, take(D), D))
        return AMUSE_EHIP;
    const float* fw = take((size_t)kAstFeat * D);
    std::vector<float> wt((size_t)kAstFeat * D);
    for (int f = 0; f < kAstFeat; ++f)
        for (size_t k = 0; k < D; ++k) wt[k * kAstFeat + f] = fw[(size_t)f * D + k];
    if (up_f32(c, &E.fh_wt, wt.data(), wt.size()) || up_f32(c, &E.fh_b, take(kAstFeat), kAstFeat)) return AMUSE_EHIP;
    return 0;
}

size_t pad128(size_t m) { return (m + 127) / 128 * 128; }

void free_ws(WorkspaceX& w) {
    void* old[] = {w.X, w.pooled, w.H, w.QK, w.Vt, w.O, w.F, w.P};
    for (void* p : old)
        if (p) (void)hipFree(p);
    w = WorkspaceX{};
}
int x_ensure_ws(void* state, int slot, int nb) {
    WorkspaceX& w = static_cast<StateX*>(state)->ws[slot];
    if (w.cap >= nb) return 0;
    free_ws(w);
    const size_t Mp = pad128((size_t)nb * kAstRows);
    w.nH = Mp * kAstDim; w.nQK = Mp * 2 * kAstDim; w.nVt = (size_t)nb * kAstDim * kAstKeysPad; w.nF = Mp * kAstMlp;
    w.nP = pad128((size_t)nb * kAstPatches) * 256;
    HIP_TRY(hipMalloc((void**)&w.X, Mp * kAstDim * 4));
    HIP_TRY(hipMalloc((void**)&w.pooled, (size_t)nb * kAstPoolSplit * kAstDim * 4));
    HIP_TRY(hipMalloc((void**)&w.H, w.nH * 4));
    HIP_TRY(hipMalloc((void**)&w.QK, w.nQK * 4));
    HIP_TRY(hipMalloc((void**)&w.Vt, w.nVt * 4));
    HIP_TRY(hipMalloc((void**)&w.O, w.nH * 4));
    HIP_TRY(hipMalloc((void**)&w.F, w.nF * 4));
    HIP_TRY(hipMalloc((void**)&w.P, w.nP * 4));
    // pad rows / pad key slots are read (GEMM tiles, LayerNorm, masked attention keys) and only have to be finite (amuse_audio_api.hip ensure_ws)
    HIP_TRY(hipMemset(w.X, 0, Mp * kAstDim * 4));
    HIP_TRY(hipMemset(w.H, 0, w.nH * 4));
    HIP_TRY(hipMemset(w.QK, 0, w.nQK * 4));
    HIP_TRY(hipMemset(w.Vt, 0, w.nVt * 4));
    HIP_TRY(hipMemset(w.O, 0, w.nH * 4));
    HIP_TRY(hipMemset(w.F, 0, w.nF * 4));
    HIP_TRY(hipMemset(w.P, 0, w.nP * 4));
    w.cap = nb;
    return 0;
}

int x_run_encoder(void* state, int slot, int which, int frame_based, const float* fbank, int nb, float* feat_out, float* hidden_out, int tap_block,
                  hipStream_t st) {
    StateX* c = static_cast<StateX*>(state);
    const WorkspaceX& w = c->ws[slot];
    const EncoderX& E = c->enc[which];
    if (nb < 1 || nb > w.cap) return failf(AMUSE_ESTATE, "audio fp32x: workspace holds %s%ld clips", "", w.cap);
    const int M = nb * kAstRows;   // a clip owns 1216 rows: 1214 tokens + 2 pad rows
    HIP_TRY(launch_im2col_x(fbank, w.P, w.P + w.nP, nb, st));
    GemmXArgs g{};
    g.A_hi = w.P; g.A_lo = w.P + w.nP; g.W = E.patch_w; g.bias = E.patch_b; g.M = nb * kAstPatches; g.N = kAstDim; g.K = 256;
    g.out_f32 = w.X; g.pos = E.pos;
    HIP_TRY(launch_gemm_x(g, EPI_PATCH, st));
    HIP_TRY(launch_ast_tokens(E.cls, E.dist, E.pos, w.X, nb, st));
    for (int l = 0; l < kAstLayers; ++l) {
        const BlockX& b = E.blk[l];
        HIP_TRY(launch_ln_x(w.X, b.n1w, b.n1b, 1e-6f, w.H, w.H + w.nH, M, st));
        g = GemmXArgs{};
        g.A_hi = w.H; g.A_lo = w.H + w.nH; g.W = b.qkv_w; g.bias = b.qkv_b; g.M = M; g.N = 3 * kAstDim; g.K = kAstDim;
        g.out_hi = w.QK; g.out_lo = w.QK + w.nQK; g.vt_hi = w.Vt; g.vt_lo = w.Vt + w.nVt;
        HIP_TRY(launch_gemm_x(g, EPI_QKV, st));
        HIP_TRY(launch_ast_attn_x(w.QK, w.QK + w.nQK, w.Vt, w.Vt + w.nVt, w.O, w.O + w.nH, nb, st));
        g = GemmXArgs{};
        g.A_hi = w.O; g.A_lo = w.O + w.nH; g.W = b.proj_w; g.bias = b.proj_b; g.M = M; g.N = kAstDim; g.K = kAstDim; g.out_f32 = w.X;
        HIP_TRY(launch_gemm_x(g, EPI_RESID_F32, st));
        HIP_TRY(launch_ln_x(w.X, b.n2w, b.n2b, 1e-6f, w.H, w.H + w.nH, M, st));
        g = GemmXArgs{};
        g.A_hi = w.H; g.A_lo = w.H + w.nH; g.W = b.fc1_w; g.bias = b.fc1_b; g.M = M; g.N = kAstMlp; g.K = kAstDim; g.out_hi = w.F; g.out_lo = w.F + w.nF;
        HIP_TRY(launch_gemm_x(g, EPI_GELU_BF16, st));
        g = GemmXArgs{};
        g.A_hi = w.F; g.A_lo = w.F + w.nF; g.W = b.fc2_w; g.bias = b.fc2_b; g.M = M; g.N = kAstDim; g.K = kAstMlp; g.out_f32 = w.X;
        HIP_TRY(launch_gemm_x(g, EPI_RESID_F32, st));
        if (hidden_out && l == tap_block) HIP_TRY(launch_untile_f32(w.X, hidden_out, M, kAstDim, kAstRows, kAstTokens, st));
    }
    HIP_TRY(launch_ast_pool(w.X, E.norm_w, E.norm_b, frame_based, w.pooled, nb, st));
    HIP_TRY(launch_ast_head_x(w.pooled, frame_based, E.fh_ln_w, E.fh_ln_b, E.fh_wt, E.fh_b, feat_out, nb, st));
    return 0;
}

int x_pool(void* state, int slot, int which, int frame_based, float* pooled, int nb, hipStream_t st) {
    StateX* c = static_cast<StateX*>(state);
    const WorkspaceX& w = c->ws[slot];
    if (nb < 1 || nb > w.cap) return failf(AMUSE_ESTATE, "audio fp32x: workspace holds %s%ld clips", "", w.cap);
    HIP_TRY(launch_ast_pool(w.X, c->enc[which].norm_w, c->enc[which].norm_b, frame_based, pooled, nb, st));
    return 0;
}

void x_destroy(void* state) {
    StateX* c = static_cast<StateX*>(state);
    if (!c) return;
    for (void* p : c->owned) (void)hipFree(p);
    for (WorkspaceX& w : c->ws) free_ws(w);
    delete c;
}
int x_create(void** state, const float* const params[3]) {
    StateX* c = new StateX();
    for (int e = 0; e < 3; ++e)
        if (int rc = build_encoder_x(c, c->enc[e], params[e])) {
            x_destroy(c);
            return rc;
        }
    *state = c;
    return 0;
}

const AudioXOps kOps = {x_create, x_destroy, x_ensure_ws, x_run_encoder, x_pool};

}  // namespace

extern "C" const amuse::AudioXOps* amuse_audio_x_ops(void) { return &kOps; }
