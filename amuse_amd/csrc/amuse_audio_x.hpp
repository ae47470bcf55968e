// Parity mode of the audio front-end (include/amuse_hip.h amuse_audio_set_precision, AMUSE_PREC_F32X): argument blocks + launchers of its
// kernels (k_audio_gemm_x.hip, k_audio_x.hip) and the function through which amuse_audio_api.hip reaches its host side (amuse_audio_x.hip).
//
// amuse_audio_api.hip holds only a WEAK reference to amuse_audio_x_ops: a link without amuse_audio_x.o (the host-only build of
// tests/host_asan, whose runtime stub defines the bf16 launchers and nothing else) still links, and amuse_audio_set_precision refuses the
// mode there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "amuse_audio.hpp"

namespace amuse {

// ---- Split operands.  A matrix the parity GEMM reads is TWO fp16 planes, hi = rn16(x) and lo = rn16(x - hi), each laid out exactly as the
// bf16 matrix of the throughput mode (tile-major, amuse_audio.hpp tm_bf16): a tile of a plane is one MFMA fragment and one 1 KiB LDS-DMA
// instruction.  Weights are packed as hi | lo UNIT PAIRS in the fragment order of pack_w: fragment row (64-feature span, fragment x),
// k-step ks -> 2 KiB: unit hi, then unit lo.
constexpr int kGemmXTM = 128, kGemmXTN = 128;   // output tile of k_gemm_x: tokens x features

struct GemmXArgs {
    const unsigned short *A_hi, *A_lo;     // fp16 planes, tile-major [M padded to 128][K]
    const unsigned short* W;               // packed hi | lo unit pairs
    const float* bias;                     // [N]
    int M, N, K;                           // N % 128 == 0, K % 64 == 0
    unsigned short *out_hi, *out_lo;       // EPI_GELU_BF16 (here: exact-erf GELU -> operand planes): [M padded][N]; EPI_QKV: q (pre-scaled) | k planes [M padded][1536]
    float* out_f32;                        // EPI_RESID_F32 (+=): tile-major [M padded][N]; EPI_PATCH: the token matrix [B * 1216 padded][768]
    const float* pos;                      // EPI_PATCH: pos_embed [1214][768]
    unsigned short *vt_hi, *vt_lo;         // EPI_QKV: V^T planes, tile-major [B * 768 rows][1216 key slots] (row / slot order: k_audio.hip k_ast_attn)
};
// epi: EPI_GELU_BF16, EPI_RESID_F32, EPI_PATCH or EPI_QKV (the enum of amuse_audio.hpp; the "BF16" of the GELU epilogue names the slot, the output is the two fp16 planes)
hipError_t launch_gemm_x(const GemmXArgs& a, int epi, hipStream_t s);
hipError_t launch_im2col_x(const float* fbank, unsigned short* p_hi, unsigned short* p_lo, int B, hipStream_t s);
hipError_t launch_ln_x(const float* X, const float* gamma, const float* beta, float eps, unsigned short* out_hi, unsigned short* out_lo, int M, hipStream_t s);
hipError_t launch_ast_attn_x(const unsigned short* qk_hi, const unsigned short* qk_lo, const unsigned short* vt_hi, const unsigned short* vt_lo,
                             unsigned short* o_hi, unsigned short* o_lo, int B, hipStream_t s);
// feature_head in fp32: LayerNorm(768, eps 1e-5) -> Linear(768 -> 256) on plain fp32 FMAs; Wt = the weight TRANSPOSED, [768][256]
hipError_t launch_ast_head_x(const float* pooled, int frame_based, const float* gamma, const float* beta, const float* Wt, const float* bias, float* out,
                             int B, hipStream_t s);

// ---- host side of the mode (amuse_audio_x.hip), as amuse_audio_api.hip sees it: the table of amuse_audio_enc.hpp that the bf16 mode fills too
struct AudioModeOps;

}  // namespace amuse

extern "C" const amuse::AudioModeOps* amuse_audio_x_ops(void);
