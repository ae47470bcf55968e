// The tail of AST_EVP behind the three encoders (include/amuse_hip.h, "Audio model metrics"): classifier heads, FusionBlock, DecoderBlock.  Argument blocks +
// launchers of its kernels (k_audio_tail.hip) and the table through which amuse_audio_api.hip reaches its host side (amuse_audio_tail.hip).
//
// amuse_audio_api.hip holds only a WEAK reference to amuse_audio_tail_ops, as it does to amuse_audio_x_ops: a link without amuse_audio_tail.o (the host-only
// build of tests/host_asan, whose runtime stub knows none of the launchers below) still links, and the tail's calls return AMUSE_ESTATE there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amuse {

constexpr int kTailLabelsEmo = 8, kTailLabelsSty = 30;
constexpr int kTailFusionDim = 768, kTailFusionLayers = 2, kTailLatent = 512, kTailDecodeLayers = 4, kTailHeads = 4, kTailFF = 2048;
constexpr int kTailHidden = 1024, kTailOut = 1024 * 128;
constexpr int kTailMaxGroup = 16;   // rows of one reconstruct sequence
constexpr int kTailRows = 32;       // rows per pass over the network (two 16-row MFMA tiles)

// ---- The skinny GEMM of the last Linear: out[B][N] = A[B][K] . W[N][K]^T + bias, B <= 32, N % 256 == 0, K % 64 == 0, 64 <= K <= 1024.
// W is PACKED (amuse_debug_tail_pack) as 1 KiB units [64 lanes][8 x 16 bit] = one MFMA A-operand fragment of 16 features x 32 k, the units of a 16-feature tile
// consecutive, tiles ascending: element (f, k) of a 16-bit plane sits at tail_pack_index(f, k, K).  AMUSE_PREC_BF16: one plane (bf16, round-to-nearest-even);
// AMUSE_PREC_F32X: every unit doubled - the hi unit (rn16(w), fp16), then the lo unit (rn16(w - hi)) - so a tile's units are 2 KiB apart.
constexpr int kTailSpan = 256;      // features per span: a workgroup takes a contiguous run of spans, its 8 waves contiguous runs of that run's 16-feature tiles
constexpr int kTailMaxK = 1024;     // the activation tile lives in LDS: 2 row tiles x K x 2 B (x 2 planes in the split mode) <= 128 KiB
__host__ __device__ inline size_t tail_pack_index(int f, int k, int K) {
    return ((size_t)(f >> 4) * (size_t)(K >> 5) + (size_t)(k >> 5)) * 512 + ((((k & 31) >> 3) << 4) + (f & 15)) * 8 + (k & 7);
}
__host__ __device__ inline size_t tail_pack_index_x(int f, int k, int K, int plane /*0 hi, 1 lo*/) {
    return ((size_t)(f >> 4) * (size_t)(K >> 5) + (size_t)(k >> 5)) * 1024 + (size_t)plane * 512 + ((((k & 31) >> 3) << 4) + (f & 15)) * 8 + (k & 7);
}
struct TailGemmArgs {
    const float* A;        // [B][K] fp32 row-major
    const void* W;         // packed as above
    const float* bias;     // [N]
    int B, N, K;
    float* out;            // [B][N] fp32 row-major
};
// precision: AMUSE_PREC_BF16 or AMUSE_PREC_F32X
hipError_t launch_tail_gemm(const TailGemmArgs& a, int precision, hipStream_t s);

// ---- The trunk's row-wise fp32 stages (fp32 weights as torch stores them, fp32 FMAs, a row's result independent of every other row but the attention's group)
// out[b][n] = act(A[b] . W[n] + bias[n]), K % 256 == 0, K <= 2048, N % 4 == 0; relu: act = max(., 0)
hipError_t launch_tail_linear(const float* A, const float* W, const float* bias, int B, int N, int K, int relu, float* out, hipStream_t s);
// nn.MultiheadAttention's core over groups of S consecutive rows (S <= 16, 4 heads): qkv [B][3 D] -> out [B][D] (before out_proj); q scaled by head_dim ** -0.5
hipError_t launch_tail_attn(const float* qkv, int B, int S, int D, float* out, hipStream_t s);
// out[b] = LayerNorm(x[b] + y[b]) (y nullable), two passes, eps 1e-5; D <= 768
hipError_t launch_tail_add_ln(const float* x, const float* y, const float* gamma, const float* beta, int B, int D, float* out, hipStream_t s);
// out[b] = emo[b] | sty[b] | con[b]  ([B][768])
hipError_t launch_tail_cat(const float* emo, const float* sty, const float* con, int B, float* out, hipStream_t s);
// A classifier head: LayerNorm(D, eps 1e-5) -> Linear(D -> L).  slices == 0: in [B][D]; slices > 0: in [B][slices][D] partial row sums (k_ast_pool's output),
// added in slice order and multiplied by `scale` first
hipError_t launch_tail_head(const float* in, int slices, float scale, int D, const float* gamma, const float* beta, const float* W, const float* bias, int L,
                            float* out, int B, hipStream_t s);

// ---- host side (amuse_audio_tail.hip), as amuse_audio_api.hip sees it.  All functions return an AMUSE_* code and leave the message in amuse_last_error.
struct AudioTailOps {
    // device images from the flat fp32 parameter array of amuse_audio_set_tail (host memory, AMUSE_AST_TAIL_PARAMS floats)
    int (*create)(void** state, const float* params);
    void (*destroy)(void* state);
    // rows of S = group consecutive clips form one sequence; fbank_out [B][131072] and / or hidden_out [B][1024] (the last Linear's input), either nullable
    int (*reconstruct)(void* state, int precision, const float* con, const float* emo, const float* sty, int B, int group, float* fbank_out, float* hidden_out,
                       hipStream_t st);
    // which = AMUSE_AUDIO_EMO | _STY.  frame_based: `in` = k_ast_pool's (cls + dist) row sums [B][kAstPoolSplit][768] -> mlp_head_featbased;
    // otherwise `in` = the features [B][256] -> mlp_head.  logits [B][8 | 30]
    int (*labels)(void* state, int which, int frame_based, const float* in, int B, float* logits, hipStream_t st);
};

}  // namespace amuse

extern "C" const amuse::AudioTailOps* amuse_audio_tail_ops(void);
