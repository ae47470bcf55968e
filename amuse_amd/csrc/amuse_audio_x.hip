// Host side of the audio front-end's parity mode (include/amuse_hip.h amuse_audio_set_precision, AMUSE_PREC_F32X): the mode of the AST encoder described in
// amuse_audio_enc.hpp on two operand planes - split-fp16 weight images, the transposed fp32 feature head, and the kernels of k_audio_gemm_x.hip / k_audio_x.hip.
// A translation unit of its own, reached from amuse_audio_api.hip through amuse_audio_x_ops() only (amuse_audio_x.hpp): a link without it
// has the bf16 mode and refuses this one.  Host code only.
#include <hip/hip_runtime.h>

#include <vector>

#include "amuse_audio_enc.hpp"
#include "amuse_audio_x.hpp"

using namespace amuse;

namespace {

struct XMode {
    static constexpr int planes = 2;   // hi, lo = hi + (the plane's element count)
    static constexpr const char* err_prefix = "audio fp32x: ";
    struct Scratch {
        std::vector<uint16_t> hi, lo;
        std::vector<unsigned short> img;
    };
    // GEMM weights: the fragment order with every unit [64 lanes][8] doubled, hi then lo; the split is amuse_debug_f16_split's (the library's one fp32 -> (hi, lo)
    // splitter), taken over the whole matrix before the permutation.  The feature head's weight: fp32, transposed to [768][256]
    static int put(AstState<XMode>* c, void* slot, const float* src, const AstParam& p) {
        const size_t n = (size_t)p.rows * p.cols;
        if (p.kind == PK_F32) return c->up.up(slot, src, n * 4);
        if (p.kind == PK_HEAD_W) {
            std::vector<float> wt(n);
            for (int f = 0; f < p.rows; ++f)
                for (int k = 0; k < p.cols; ++k) wt[(size_t)k * p.rows + f] = src[(size_t)f * p.cols + k];
            return c->up.up(slot, wt.data(), n * 4);
        }
        Scratch& s = c->scratch;
        s.hi.resize(n);
        s.lo.resize(n);
        s.img.resize(2 * n);
        if (int e = amuse_debug_f16_split(src, n, s.hi.data(), s.lo.data())) return e;
        for_each_fragment_lane(p.rows, p.cols, [&](size_t u, int lane, size_t at) {
            memcpy(&s.img[u * 1024 + 8 * lane], &s.hi[at], 16);
            memcpy(&s.img[u * 1024 + 512 + 8 * lane], &s.lo[at], 16);
        });
        return c->up.up(slot, s.img.data(), s.img.size() * 2);
    }
    static hipError_t im2col(const float* fbank, Operand P, int nb, hipStream_t st) { return launch_im2col_x(fbank, P.hi, P.hi + P.n, nb, st); }
    static hipError_t ln(const float* X, const float* gamma, const float* beta, float eps, Operand out, int M, hipStream_t st) {
        return launch_ln_x(X, gamma, beta, eps, out.hi, out.hi + out.n, M, st);
    }
    static hipError_t gemm(int epi, Operand A, const unsigned short* W, const float* bias, int M, int N, int K, Operand out, float* out_f32, const float* pos, Operand vt,
                           hipStream_t st) {
        GemmXArgs g{};
        g.A_hi = A.hi; g.A_lo = A.hi + A.n; g.W = W; g.bias = bias; g.M = M; g.N = N; g.K = K; g.out_f32 = out_f32; g.pos = pos;
        g.out_hi = out.hi; g.out_lo = out.hi + out.n; g.vt_hi = vt.hi; g.vt_lo = vt.hi + vt.n;   // (an operand the epilogue does not write is {null, 0})
        return launch_gemm_x(g, epi, st);
    }
    static hipError_t attn(Operand QK, Operand Vt, Operand O, int nb, hipStream_t st) {
        return launch_ast_attn_x(QK.hi, QK.hi + QK.n, Vt.hi, Vt.hi + Vt.n, O.hi, O.hi + O.n, nb, st);
    }
    static hipError_t head(const float* pooled, int frame_based, const Encoder& E, float* out, int nb, hipStream_t st) {
        return launch_ast_head_x(pooled, frame_based, E.fh_ln_w, E.fh_ln_b, static_cast<const float*>(E.fh_w), E.fh_b, out, nb, st);
    }
};

}  // namespace

extern "C" const amuse::AudioModeOps* amuse_audio_x_ops(void) { return &kAudioModeOps<XMode>; }
