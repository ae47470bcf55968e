// Host code shared by the audio front-end's translation units (amuse_audio_api.hip: bf16 mode + C ABI; amuse_audio_x.hip: the AMUSE_PREC_F32X parity mode;
// amuse_audio_tail.hip: the error plumbing only): error reporting, the owning uploader, and ONE description of an AST encoder - its parameter order, the GEMM's
// weight-fragment order, its device image, its activation workspace and its launch sequence - written against a small MODE (a struct of static functions: what
// it uploads for a parameter kind, how an operand becomes its kernels' arguments), plus the table of functions through which the C ABI reaches a mode.
// The two modes differ in their kernels and in the number of 16-bit PLANES of an operand matrix (bf16: 1; fp32x: 2, hi and lo): a buffer of n elements is
// 2 * planes * n bytes and the low plane sits at hi + n.  Host code only - no kernel includes this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_audio.hpp"

int amuse_fail_msg(int code, const char* msg);   // amuse_api.hip: the library's thread-local error slot

namespace amuse {

// ---- error plumbing.  HIP_TRY_P(prefix, call): `prefix` names the unit in the message ("", "audio fp32x: ", "audio tail: ")
inline int failf(int code, const char* fmt, const char* a = "", long b = 0, long c = 0) {
    char buf[400];
    snprintf(buf, sizeof(buf), fmt, a, b, c);
    return amuse_fail_msg(code, buf);
}
inline int fail_hip(const char* prefix, hipError_t e, long line) {
    char buf[400];
    snprintf(buf, sizeof(buf), "%s%s (line %ld)", prefix, hipGetErrorString(e), line);
    return amuse_fail_msg(AMUSE_EHIP, buf);
}
#define HIP_TRY_P(prefix, expr)                                               \
    do {                                                                      \
        hipError_t e_ = (expr);                                               \
        if (e_ != hipSuccess) return fail_hip(prefix, e_, __LINE__);          \
    } while (0)

inline unsigned short f2bf(float f) {  // round-to-nearest-even, as v_cvt_pk_bf16_f32
    uint32_t x;
    memcpy(&x, &f, 4);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((x >> 16) | 0x40);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (unsigned short)(x >> 16);
}
inline size_t pad128(size_t m) { return (m + 127) / 128 * 128; }

// device blocks it allocated and filled, in order; freed in that order
struct Uploader {
    const char* err_prefix = "";
    std::vector<void*> owned;
    int up(void* slot, const void* src, size_t bytes) {   // slot: the address of a device pointer of any type
        void* d = nullptr;
        HIP_TRY_P(err_prefix, hipMalloc(&d, bytes));
        owned.push_back(d);
        memcpy(slot, &d, sizeof(d));
        HIP_TRY_P(err_prefix, hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    void free_all() {
        for (void* p : owned) (void)hipFree(p);
        owned.clear();
    }
};

// ---- the encoder's device image.  GEMM weights and the feature head's weight are in the mode's format (Mode::put, below)
struct Block {
    float *n1w, *n1b, *n2w, *n2b, *qkv_b, *proj_b, *fc1_b, *fc2_b;
    unsigned short *qkv_w, *proj_w, *fc1_w, *fc2_w;
};
struct Encoder {
    float *cls, *dist, *pos, *patch_b, *norm_w, *norm_b, *fh_ln_w, *fh_ln_b, *fh_b;
    unsigned short* patch_w;
    void* fh_w;
    Block blk[kAstLayers];
};

// ---- the order of the flat parameter array (include/amuse_hip.h AMUSE_AST_PARAMS; amuse_amd/audio_weights.py ast_param_spec): front, 12 x block, back
enum ParamKind { PK_F32, PK_GEMM_W, PK_HEAD_W };   // fp32 vector | Linear weight [rows][cols] of a GEMM | feature_head.1.weight [rows][cols]
struct AstParam { size_t slot; int rows, cols; ParamKind kind; };   // slot: offset of the device pointer in Encoder / Block
#define ENC_(f, rows, cols, kind) {offsetof(Encoder, f), rows, cols, kind}
#define BLK_(f, rows, cols, kind) {offsetof(Block, f), rows, cols, kind}
constexpr AstParam kAstFront[] = {ENC_(cls, 1, kAstDim, PK_F32), ENC_(dist, 1, kAstDim, PK_F32), ENC_(pos, kAstTokens, kAstDim, PK_F32),
                                  ENC_(patch_w, kAstDim, 256, PK_GEMM_W), ENC_(patch_b, 1, kAstDim, PK_F32)};
constexpr AstParam kAstBlock[] = {BLK_(n1w, 1, kAstDim, PK_F32), BLK_(n1b, 1, kAstDim, PK_F32), BLK_(qkv_w, 3 * kAstDim, kAstDim, PK_GEMM_W),
                                  BLK_(qkv_b, 1, 3 * kAstDim, PK_F32), BLK_(proj_w, kAstDim, kAstDim, PK_GEMM_W), BLK_(proj_b, 1, kAstDim, PK_F32),
                                  BLK_(n2w, 1, kAstDim, PK_F32), BLK_(n2b, 1, kAstDim, PK_F32), BLK_(fc1_w, kAstMlp, kAstDim, PK_GEMM_W),
                                  BLK_(fc1_b, 1, kAstMlp, PK_F32), BLK_(fc2_w, kAstDim, kAstMlp, PK_GEMM_W), BLK_(fc2_b, 1, kAstDim, PK_F32)};
constexpr AstParam kAstBack[] = {ENC_(norm_w, 1, kAstDim, PK_F32), ENC_(norm_b, 1, kAstDim, PK_F32), ENC_(fh_ln_w, 1, kAstDim, PK_F32),
                                 ENC_(fh_ln_b, 1, kAstDim, PK_F32), ENC_(fh_w, kAstFeat, kAstDim, PK_HEAD_W), ENC_(fh_b, 1, kAstFeat, PK_F32)};
#undef ENC_
#undef BLK_

// the GEMM's weight-fragment order (amuse_audio.hpp GemmArgs::W) of a Linear weight [N][K]: for unit u = ((64-feature span sp, fragment x), k-step ks) and lane
// (g, i), the 8 consecutive source elements from offset s are the lane's 8 elements of the unit.  put(u, lane, s) writes them in the mode's element format.
template <class Put>
void for_each_fragment_lane(int N, int K, Put&& put) {
    size_t u = 0;
    for (int sp = 0; sp < N / 64; ++sp)
        for (int x = 0; x < 4; ++x)
            for (int ks = 0; ks < K / 32; ++ks, ++u)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15;
                    const int f = 64 * sp + 32 * (x >> 1) + 8 * (i >> 2) + 4 * (x & 1) + (i & 3);
                    put(u, lane, (size_t)f * K + 32 * ks + 8 * g);
                }
}

// ---- activations of one encoder pass over `cap` clips.  n*: elements per plane of the operand matrices (O as H)
struct Workspace {
    int cap = 0;
    float *X = nullptr, *pooled = nullptr;
    unsigned short *H = nullptr, *QK = nullptr, *Vt = nullptr, *O = nullptr, *F = nullptr, *P = nullptr;
    size_t nH = 0, nQK = 0, nVt = 0, nF = 0, nP = 0;
};
struct Operand { unsigned short* hi; size_t n; };   // a matrix the mode's GEMM / attention reads or writes: planes of n elements from hi

// what the C ABI holds of a mode: its three encoders' images and one workspace per encoder stream (amuse_audio_encode uses [0])
template <class Mode>
struct AstState {
    Encoder enc[3];
    Uploader up{Mode::err_prefix, {}};
    Workspace ws[3];
    typename Mode::Scratch scratch;   // host buffers of the packers, reused from weight to weight
};

// A Mode supplies:  planes, err_prefix, Scratch;  put(state, slot, src, param) -> AMUSE_* (upload one parameter in the mode's format);
// im2col / ln / gemm / attn / head -> hipError_t (the mode's launchers on Operands).  All static.
template <class Mode>
struct AstOps {
    using State = AstState<Mode>;

    static int build_encoder(State* c, Encoder& E, const float* p) {
        auto walk = [&](void* base, const AstParam* t, size_t n) {
            for (size_t i = 0; i < n; ++i) {
                if (Mode::put(c, static_cast<char*>(base) + t[i].slot, p, t[i])) return (int)AMUSE_EHIP;
                p += (size_t)t[i].rows * t[i].cols;
            }
            return 0;
        };
        if (walk(&E, kAstFront, std::size(kAstFront))) return AMUSE_EHIP;
        for (Block& b : E.blk)
            if (walk(&b, kAstBlock, std::size(kAstBlock))) return AMUSE_EHIP;
        return walk(&E, kAstBack, std::size(kAstBack));
    }
    static void destroy(void* state) {
        State* c = static_cast<State*>(state);
        if (!c) return;
        c->up.free_all();
        for (Workspace& w : c->ws) free_ws(w);
        delete c;
    }
    // the device images from the flat fp32 parameter arrays of amuse_audio_create (host memory)
    static int create(void** state, const float* const params[3]) {
        State* c = new State();
        for (int e = 0; e < 3; ++e)
            if (int rc = build_encoder(c, c->enc[e], params[e])) {
                destroy(c);
                return rc;
            }
        c->scratch = typename Mode::Scratch{};
        *state = c;
        return 0;
    }

    static void free_ws(Workspace& w) {
        void* old[] = {w.X, w.pooled, w.H, w.QK, w.Vt, w.O, w.F, w.P};
        for (void* p : old)
            if (p) (void)hipFree(p);
        w = Workspace{};
    }
    static int ensure_ws(void* state, int slot, int nb) {
        Workspace& w = static_cast<State*>(state)->ws[slot];
        if (w.cap >= nb) return 0;
        free_ws(w);
        const size_t Mp = pad128((size_t)nb * kAstRows), el = 2 * Mode::planes;   // bytes per operand element
        w.nH = Mp * kAstDim; w.nQK = Mp * 2 * kAstDim; w.nVt = (size_t)nb * kAstDim * kAstKeysPad; w.nF = Mp * kAstMlp;
        w.nP = pad128((size_t)nb * kAstPatches) * 256;
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.X, Mp * kAstDim * 4));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.pooled, (size_t)nb * kAstPoolSplit * kAstDim * 4));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.H, w.nH * el));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.QK, w.nQK * el));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.Vt, w.nVt * el));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.O, w.nH * el));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.F, w.nF * el));
        HIP_TRY_P(Mode::err_prefix, hipMalloc((void**)&w.P, w.nP * el));
        // every activation is tile-major (amuse_audio.hpp), rows padded to the GEMM's 128-token tile.  Pad rows are read by the GEMM
        // tiles and the LayerNorm (their results stay in pad rows) and the V^T pad columns by the attention (masked): they only
        // have to be finite
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.X, 0, Mp * kAstDim * 4));
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.H, 0, w.nH * el));
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.O, 0, w.nH * el));
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.F, 0, w.nF * el));
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.P, 0, w.nP * el));
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.Vt, 0, w.nVt * el));
        HIP_TRY_P(Mode::err_prefix, hipMemset(w.QK, 0, w.nQK * el));
        w.cap = nb;
        return 0;
    }

    // encoder `which` over nb <= capacity clips whose fbanks are at `fbank`, on workspace `slot`
    static int run_encoder(void* state, int slot, int which, int frame_based, const float* fbank, int nb, float* feat_out, float* hidden_out, int tap_block,
                           hipStream_t st) {
        const State* c = static_cast<State*>(state);
        const Workspace& w = c->ws[slot];
        const Encoder& E = c->enc[which];
        if (nb < 1 || nb > w.cap) return failf(AMUSE_ESTATE, "%sworkspace holds %ld clips", Mode::err_prefix, w.cap);
        const Operand H{w.H, w.nH}, QK{w.QK, w.nQK}, Vt{w.Vt, w.nVt}, O{w.O, w.nH}, F{w.F, w.nF}, P{w.P, w.nP}, none{nullptr, 0};
        const int M = nb * kAstRows, D = kAstDim;   // a clip owns 1216 rows: 1214 tokens + 2 pad rows
        HIP_TRY_P(Mode::err_prefix, Mode::im2col(fbank, P, nb, st));
        HIP_TRY_P(Mode::err_prefix, Mode::gemm(EPI_PATCH, P, E.patch_w, E.patch_b, nb * kAstPatches, D, 256, none, w.X, E.pos, none, st));
        HIP_TRY_P(Mode::err_prefix, launch_ast_tokens(E.cls, E.dist, E.pos, w.X, nb, st));
        for (int l = 0; l < kAstLayers; ++l) {
            const Block& b = E.blk[l];
            HIP_TRY_P(Mode::err_prefix, Mode::ln(w.X, b.n1w, b.n1b, 1e-6f, H, M, st));
            HIP_TRY_P(Mode::err_prefix, Mode::gemm(EPI_QKV, H, b.qkv_w, b.qkv_b, M, 3 * D, D, QK, nullptr, nullptr, Vt, st));
            HIP_TRY_P(Mode::err_prefix, Mode::attn(QK, Vt, O, nb, st));
            HIP_TRY_P(Mode::err_prefix, Mode::gemm(EPI_RESID_F32, O, b.proj_w, b.proj_b, M, D, D, none, w.X, nullptr, none, st));
            HIP_TRY_P(Mode::err_prefix, Mode::ln(w.X, b.n2w, b.n2b, 1e-6f, H, M, st));
            HIP_TRY_P(Mode::err_prefix, Mode::gemm(EPI_GELU_BF16, H, b.fc1_w, b.fc1_b, M, kAstMlp, D, F, nullptr, nullptr, none, st));
            HIP_TRY_P(Mode::err_prefix, Mode::gemm(EPI_RESID_F32, F, b.fc2_w, b.fc2_b, M, D, kAstMlp, none, w.X, nullptr, none, st));
            if (hidden_out && l == tap_block) HIP_TRY_P(Mode::err_prefix, launch_untile_f32(w.X, hidden_out, M, D, kAstRows, kAstTokens, st));
        }
        HIP_TRY_P(Mode::err_prefix, launch_ast_pool(w.X, E.norm_w, E.norm_b, frame_based, w.pooled, nb, st));
        HIP_TRY_P(Mode::err_prefix, Mode::head(w.pooled, frame_based, E, feat_out, nb, st));
        return 0;
    }
    // v.norm + k_ast_pool with the given pooling over the residual stream the last run_encoder left in workspace `slot`, into `pooled` [nb][kAstPoolSplit][768]
    // (amuse_audio_encode_labels: the labels' pooling where it differs from the features')
    static int pool(void* state, int slot, int which, int frame_based, float* pooled, int nb, hipStream_t st) {
        const State* c = static_cast<State*>(state);
        const Workspace& w = c->ws[slot];
        if (nb < 1 || nb > w.cap) return failf(AMUSE_ESTATE, "%sworkspace holds %ld clips", Mode::err_prefix, w.cap);
        HIP_TRY_P(Mode::err_prefix, launch_ast_pool(w.X, c->enc[which].norm_w, c->enc[which].norm_b, frame_based, pooled, nb, st));
        return 0;
    }
};

// ---- a mode as the C ABI sees it (amuse_audio_api.hip): AstOps<Mode>'s functions.  All return an AMUSE_* code and leave the message in amuse_last_error.
struct AudioModeOps {
    int (*create)(void** state, const float* const params[3]);
    void (*destroy)(void* state);
    int (*ensure_ws)(void* state, int slot, int nb);   // workspace `slot` (0..2) holds at least nb clips
    int (*run_encoder)(void* state, int slot, int which, int frame_based, const float* fbank, int nb, float* feat_out, float* hidden_out, int tap_block, hipStream_t st);
    int (*pool)(void* state, int slot, int which, int frame_based, float* pooled, int nb, hipStream_t st);
};
template <class Mode>
constexpr AudioModeOps kAudioModeOps = {AstOps<Mode>::create, AstOps<Mode>::destroy, AstOps<Mode>::ensure_ws, AstOps<Mode>::run_encoder, AstOps<Mode>::pool};

}  // namespace amuse
