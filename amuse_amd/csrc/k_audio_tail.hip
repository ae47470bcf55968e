// Kernels of AST_EVP's tail (amuse_audio_tail.hpp; include/amuse_hip.h "Audio model metrics"), gfx950.
//
//   k_tail_gemm    the last Linear (1024 -> 131072): a weight stream of 268 MB (bf16) / 537 MB (split fp16) against at most 32 rows of activations.
//                  HBM-bound: the floor is the stream's bytes over the sweep rate.  Each wave owns a contiguous run of 16-feature tiles, i.e. ONE contiguous
//                  byte range of the packed image, and walks it in chunks of UN k-steps: global -> VGPR, a lane's 16 B inside a wave-contiguous 1 KiB, non-temporal
//                  (the stream exceeds the Infinity Cache), the next chunk's loads in flight while the current one feeds the MFMAs - also across tile boundaries.
//                  No LDS staging of weights (no two waves share one).  The activation rows are rounded (bf16) or split (fp16 hi / lo) ONCE into LDS as MFMA
//                  B-operand fragments; the weights are the 16-feature A operand, so a lane's four accumulators are four consecutive features of one row:
//                  a 16 x 16 accumulator leaves as 16 row segments of 64 B (four lanes x 16 B).  Both row tiles of the call are fed from one pass over the weights.
//   k_tail_linear / k_tail_attn / k_tail_add_ln / k_tail_cat / k_tail_head
//                  the trunk (24 M parameters, off the hot path) and the classifier heads as row-wise fp32 launches: fp32 weights in torch's layout,
//                  plain FMAs, two-pass LayerNorm, softmax over at most 16 keys.
#include <hip/hip_runtime.h>

#include "../../include/amuse_hip.h"
#include "amuse_audio_tail.hpp"
#include "amuse_dev.hpp"
#include "amuse_kernels.hpp"   // DeviceOnce

namespace amuse {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------- the skinny GEMM
template <int UN, int PL>
__device__ __forceinline__ void tail_load(u32x4 (&dst)[UN * PL], const u32x4* p) {
#pragma unroll
    for (int j = 0; j < UN * PL; ++j) dst[j] = __builtin_nontemporal_load(p + j * 64);
}

// UN: k-steps (32 k) per chunk, K / 32 % UN == 0; NRT: 16-row activation tiles; X: split fp16 (three MFMAs per product, lo.lo dropped) instead of bf16
template <int UN, int NRT, bool X>
__global__ __launch_bounds__(512) void k_tail_gemm(TailGemmArgs a) {
    extern __shared__ u32x4 xs[];   // [plane][row tile][k-step][64 lanes] x 16 B: B-operand fragments, lane (g, i) = row i, k 8 g .. 8 g + 7
    constexpr int PL = X ? 2 : 1;
    const int KS = a.K >> 5;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int units = NRT * KS;
    for (int u = wave; u < units; u += 8) {
        const int rt = u / KS, ks = u - rt * KS;
        const int row = 16 * rt + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
        f32x4 v0 = splat4(0.f), v1 = splat4(0.f);
        if (row < a.B) {
            v0 = ld4(a.A + (size_t)row * a.K + k0);
            v1 = ld4(a.A + (size_t)row * a.K + k0 + 4);
        }
        if constexpr (X) {
            const F16Pair p = split_f16(v0, v1);
            xs[u * 64 + lane] = __builtin_bit_cast(u32x4, p.hi);
            xs[(units + u) * 64 + lane] = __builtin_bit_cast(u32x4, p.lo);
        } else {
            xs[u * 64 + lane] = __builtin_bit_cast(u32x4, pack_bf16(v0, v1));
        }
    }
    __syncthreads();

    // contiguous spans per workgroup, contiguous tiles per wave (16 tiles per span, 8 waves: 2 per span and wave)
    const int spans = a.N / kTailSpan;
    const int s0 = (int)((long long)blockIdx.x * spans / gridDim.x), s1 = (int)((long long)(blockIdx.x + 1) * spans / gridDim.x);
    const int tiles_w = (s1 - s0) * (kTailSpan / 16 / 8);
    int tile = s0 * (kTailSpan / 16) + wave * tiles_w;
    const int cpt = KS / UN;   // chunks per tile
    const long long nchunks = (long long)tiles_w * cpt;
    if (nchunks == 0) return;
    const u32x4* wp = reinterpret_cast<const u32x4*>(a.W) + (size_t)tile * KS * PL * 64 + lane;
    const int g = lane >> 4, i = lane & 15;

    f32x4 acc[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc[rt] = splat4(0.f);
    int c_in = 0;
    // one chunk: UN k-steps of the current tile from registers; at the tile's last chunk lane (g, i) holds features 16 tile + 4 g .. + 3 of row 16 rt + i
    auto step = [&](const u32x4(&w)[UN * PL]) {
        const int ks0 = c_in * UN;
#pragma unroll
        for (int j = 0; j < UN; ++j)
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                const u32x4 xh = xs[(rt * KS + ks0 + j) * 64 + lane];
                if constexpr (X) {
                    const u32x4 xl = xs[(units + rt * KS + ks0 + j) * 64 + lane];
                    const f16x8 wh = __builtin_bit_cast(f16x8, w[2 * j]), wl = __builtin_bit_cast(f16x8, w[2 * j + 1]);
                    acc[rt] = mfma_f16(wl, __builtin_bit_cast(f16x8, xh), acc[rt]);
                    acc[rt] = mfma_f16(wh, __builtin_bit_cast(f16x8, xl), acc[rt]);
                    acc[rt] = mfma_f16(wh, __builtin_bit_cast(f16x8, xh), acc[rt]);
                } else {
                    acc[rt] = mfma_bf16(__builtin_bit_cast(bf16x8, w[j]), __builtin_bit_cast(bf16x8, xh), acc[rt]);
                }
            }
        if (++c_in == cpt) {
            const int f = 16 * tile + 4 * g;
            const f32x4 bv = ld4(a.bias + f);
#pragma unroll
            for (int rt = 0; rt < NRT; ++rt) {
                const int row = 16 * rt + i;
                if (row < a.B) st4(a.out + (size_t)row * a.N + f, acc[rt] + bv);
                acc[rt] = splat4(0.f);
            }
            ++tile;
            c_in = 0;
        }
    };
    // two register buffers, no copies: while one feeds the MFMAs the other's loads are in flight.  The prefetch is UNCONDITIONAL (behind the wave's last chunk it
    // fetches that chunk again: 8 KiB of a 128 KiB run, in bounds), so that the wait in front of a chunk's MFMAs is vmcnt(loads of the other buffer), never 0
    constexpr int kStep = UN * PL * 64;
    const u32x4* const wlast = wp + (nchunks - 1) * kStep;
    u32x4 b0[UN * PL], b1[UN * PL];
    tail_load<UN, PL>(b0, wp);
    for (long long c = 0; c < nchunks; c += 2) {
        wp = wp + kStep < wlast ? wp + kStep : wlast;
        tail_load<UN, PL>(b1, wp);
        step(b0);
        if (c + 1 >= nchunks) break;
        wp = wp + kStep < wlast ? wp + kStep : wlast;
        tail_load<UN, PL>(b0, wp);
        step(b1);
    }
}

template <int UN, int NRT, bool X>
hipError_t launch_tail_gemm_t(const TailGemmArgs& a, hipStream_t s) {
    static DeviceOnce once;
    int dev_;
    if (!once.done(&dev_)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tail_gemm<UN, NRT, X>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (X ? 2 : 1) * NRT * (kTailMaxK / 32) * 1024);
        if (e != hipSuccess) return e;
        once.set(dev_);
    }
    const int spans = a.N / kTailSpan;
    const int resident = 256;   // one workgroup per CU, 256 CUs
    const size_t lds = (size_t)(X ? 2 : 1) * NRT * (a.K / 32) * 1024;
    hipLaunchKernelGGL((k_tail_gemm<UN, NRT, X>), dim3(spans < resident ? spans : resident), dim3(512), lds, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the trunk, fp32
// one wave per output feature, every row of the call: lane l holds W[n][256 j + 4 l .. + 3]; a dot product is each lane's FMAs in k order, then a butterfly
__global__ __launch_bounds__(256) void k_tail_linear(const float* __restrict__ A, const float* __restrict__ W, const float* __restrict__ bias, int B, int N, int K,
                                                      int relu, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int KJ = K >> 8;
    f32x4 w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = j < KJ ? ld4(W + (size_t)n * K + 256 * j + 4 * lane) : splat4(0.f);
    const float bn = bias[n];
    for (int b = 0; b < B; ++b) {
        const float* x = A + (size_t)b * K + 4 * lane;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < KJ) {
                const f32x4 v = ld4(x + 256 * j);
                s = fmaf(w[j][0], v[0], s);
                s = fmaf(w[j][1], v[1], s);
                s = fmaf(w[j][2], v[2], s);
                s = fmaf(w[j][3], v[3], s);
            }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        s += bn;
        if (relu) s = fmaxf(s, 0.f);
        if (lane == 0) out[(size_t)b * N + n] = s;
    }
}

// grid (groups, heads): S <= 16 rows of one group, one head of width hd = D / 4 <= 192
constexpr int kTailHdMax = 192, kTailHdPad = kTailHdMax + 1;
__global__ __launch_bounds__(256) void k_tail_attn(const float* __restrict__ qkv, int S, int D, float* __restrict__ out) {
    __shared__ float q[kTailMaxGroup][kTailHdPad], k[kTailMaxGroup][kTailHdPad], v[kTailMaxGroup][kTailHdPad];
    __shared__ float sc[kTailMaxGroup][kTailMaxGroup + 1];
    const int t = threadIdx.x, hd = D / kTailHeads, h = blockIdx.y;
    const size_t row0 = (size_t)blockIdx.x * S;
    const float scale = 1.0f / sqrtf((float)hd);
    for (int e = t; e < S * hd; e += 256) {
        const int i = e / hd, d = e - i * hd;
        const float* r = qkv + (row0 + i) * 3 * D + h * hd + d;
        q[i][d] = r[0] * scale;
        k[i][d] = r[D];
        v[i][d] = r[2 * D];
    }
    __syncthreads();
    for (int p = t; p < S * S; p += 256) {
        const int i = p / S, j = p - i * S;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s = fmaf(q[i][d], k[j][d], s);
        sc[i][j] = s;
    }
    __syncthreads();
    if (t < S) {
        float m = sc[t][0];
        for (int j = 1; j < S; ++j) m = fmaxf(m, sc[t][j]);
        float sum = 0.f;
        for (int j = 0; j < S; ++j) {
            const float e = expf(sc[t][j] - m);
            sc[t][j] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        for (int j = 0; j < S; ++j) sc[t][j] *= inv;
    }
    __syncthreads();
    for (int e = t; e < S * hd; e += 256) {
        const int i = e / hd, d = e - i * hd;
        float o = 0.f;
        for (int j = 0; j < S; ++j) o = fmaf(sc[i][j], v[j][d], o);
        out[(row0 + i) * D + h * hd + d] = o;
    }
}

// LayerNorm statistics of a row held as v[3] per thread (feature t + 256 i, D <= 768), two passes: -> (mean, rstd)
__device__ __forceinline__ void tail_row_stats(const float (&v)[3], int D, float eps, float (&red)[2][4], float& mean, float& rstd) {
    const int t = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (t + 256 * i < D) s += v[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((t & 63) == 0) red[0][t >> 6] = s;
    __syncthreads();
    mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    float qq = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (t + 256 * i < D) { const float d = v[i] - mean; qq += d * d; }
    for (int o = 32; o > 0; o >>= 1) qq += __shfl_xor(qq, o);
    if ((t & 63) == 0) red[1][t >> 6] = qq;
    __syncthreads();
    rstd = 1.0f / sqrtf(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D + eps);
}

__global__ __launch_bounds__(256) void k_tail_add_ln(const float* x, const float* __restrict__ y, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int D, float* out /*may be x: a thread reads and writes its own features*/) {
    __shared__ float red[2][4];
    const int t = threadIdx.x;
    const size_t r = (size_t)blockIdx.x * D;
    float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = t + 256 * i;
        if (c < D) v[i] = y ? x[r + c] + y[r + c] : x[r + c];
    }
    float mean, rstd;
    tail_row_stats(v, D, 1e-5f, red, mean, rstd);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = t + 256 * i;
        if (c < D) out[r + c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
    }
}

__global__ __launch_bounds__(256) void k_tail_cat(const float* __restrict__ emo, const float* __restrict__ sty, const float* __restrict__ con, float* __restrict__ out) {
    const int t = threadIdx.x;
    const size_t b = blockIdx.x;
    out[b * 768 + t] = emo[b * 256 + t];
    out[b * 768 + 256 + t] = sty[b * 256 + t];
    out[b * 768 + 512 + t] = con[b * 256 + t];
}

__global__ __launch_bounds__(256) void k_tail_head(const float* __restrict__ in, int slices, float scale, int D, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ W, const float* __restrict__ bias, int L,
                                                    float* __restrict__ out) {
    __shared__ float red[2][4];
    __shared__ float h[768];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t b = blockIdx.x;
    float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = t + 256 * i;
        if (c < D) {
            if (slices > 0) {
                float s = 0.f;
                for (int y = 0; y < slices; ++y) s += in[(b * slices + y) * D + c];
                v[i] = s * scale;
            } else {
                v[i] = in[b * D + c];
            }
        }
    }
    float mean, rstd;
    tail_row_stats(v, D, 1e-5f, red, mean, rstd);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = t + 256 * i;
        if (c < D) h[c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
    }
    __syncthreads();
    for (int l = wave; l < L; l += 4) {
        float s = 0.f;
        for (int c = lane; c < D; c += 64) s = fmaf(W[(size_t)l * D + c], h[c], s);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) out[b * L + l] = s + bias[l];
    }
}

}  // namespace

hipError_t launch_tail_gemm(const TailGemmArgs& a, int precision, hipStream_t s) {
    if (a.B < 1 || a.B > kTailRows || a.N < kTailSpan || a.N % kTailSpan || a.K < 64 || a.K % 64 || a.K > kTailMaxK) return hipErrorInvalidValue;
    const bool x = precision == AMUSE_PREC_F32X;
    if (!x && precision != AMUSE_PREC_BF16) return hipErrorInvalidValue;
    // chunk depth: 16 KiB of weights per wave and register buffer where K allows it (K % 512 == 0: 16 k-steps of bf16, 8 of hi | lo pairs), 2 k-steps otherwise
    const bool wide = a.K % 512 == 0, two = a.B > 16;
    if (x) {
        if (wide) return two ? launch_tail_gemm_t<8, 2, true>(a, s) : launch_tail_gemm_t<8, 1, true>(a, s);
        return two ? launch_tail_gemm_t<2, 2, true>(a, s) : launch_tail_gemm_t<2, 1, true>(a, s);
    }
    if (wide) return two ? launch_tail_gemm_t<16, 2, false>(a, s) : launch_tail_gemm_t<16, 1, false>(a, s);
    return two ? launch_tail_gemm_t<2, 2, false>(a, s) : launch_tail_gemm_t<2, 1, false>(a, s);
}

hipError_t launch_tail_linear(const float* A, const float* W, const float* bias, int B, int N, int K, int relu, float* out, hipStream_t s) {
    if (B < 1 || N < 4 || N % 4 || K < 256 || K % 256 || K > 2048) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tail_linear, dim3(N / 4), dim3(256), 0, s, A, W, bias, B, N, K, relu, out);
    return hipGetLastError();
}
hipError_t launch_tail_attn(const float* qkv, int B, int S, int D, float* out, hipStream_t s) {
    if (S < 1 || S > kTailMaxGroup || B < 1 || B % S || D % kTailHeads || D / kTailHeads > kTailHdMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tail_attn, dim3(B / S, kTailHeads), dim3(256), 0, s, qkv, S, D, out);
    return hipGetLastError();
}
hipError_t launch_tail_add_ln(const float* x, const float* y, const float* gamma, const float* beta, int B, int D, float* out, hipStream_t s) {
    if (B < 1 || D < 1 || D > 768) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tail_add_ln, dim3(B), dim3(256), 0, s, x, y, gamma, beta, D, out);
    return hipGetLastError();
}
hipError_t launch_tail_cat(const float* emo, const float* sty, const float* con, int B, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_tail_cat, dim3(B), dim3(256), 0, s, emo, sty, con, out);
    return hipGetLastError();
}
hipError_t launch_tail_head(const float* in, int slices, float scale, int D, const float* gamma, const float* beta, const float* W, const float* bias, int L,
                            float* out, int B, hipStream_t s) {
    if (B < 1 || D < 1 || D > 768 || L < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tail_head, dim3(B), dim3(256), 0, s, in, slices, scale, D, gamma, beta, W, bias, L, out);
    return hipGetLastError();
}

}  // namespace amuse
