// Audio front-end, parity mode (amuse_audio_set_precision AMUSE_PREC_F32X): the kernels around k_gemm_x (k_audio_gemm_x.hip) that produce
// or consume SPLIT fp16 operands - x = hi + lo, hi = rn16(x), lo = rn16(x - hi), two planes each laid out as the bf16 matrix of the
// throughput mode (amuse_audio_x.hpp) - with everything else in fp32:
//   k_im2col_x     16 x 16 stride-10 patches of the spectrogram -> two planes (K = 256)
//   k_ln_x         LayerNorm of the fp32 residual stream (fp32 statistics, two passes) -> two planes
//   k_ast_attn_x   flash attention, S = 1214, d = 64: S^T = Kl.Qh + Kh.Ql + Kh.Qh and O^T the same with the split P, on
//                  v_mfma_f32_16x16x32_f16; softmax in exp2 units and fp32 with the running-maximum rule of the fp32x decode attention
//                  (k_vae_fusedx.hip attend_x): lazy rescaling by kAttnTau, so p <= 2^6; row sums of the split P in fp32
//   k_ast_head_x   feature_head on plain fp32 FMAs (LayerNorm eps 1e-5, Linear 768 -> 256 from fp32 weights)
// The residual stream, the token rows, the final LayerNorm + pooling and the hidden-state tap are the fp32 kernels of k_audio.hip, unchanged.
#include <cstdlib>

#include "amuse_dev.hpp"
#include "amuse_audio_x.hpp"
#include "amuse_kernels.hpp"   // DeviceOnce

namespace amuse {
namespace {

typedef unsigned short f16raw;
// LDS-DMA: 64 lanes x 16 B from (wave-uniform base + 32-bit lane offset) to LDS [dst, dst + 1 KiB), lane-linear (k_audio_gemm.hip)
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}

// ---------------------------------------------------------------------------------------------- im2col
// patches[b * 1212 + fh * 101 + tw][kh * 16 + kw] = fbank[b][10 tw + kw][10 fh + kh] (k_audio.hip k_im2col), as two planes
__global__ __launch_bounds__(256) void k_im2col_x(const float* __restrict__ fbank, f16raw* __restrict__ p_hi, f16raw* __restrict__ p_lo, int B) {
    const size_t row = (size_t)blockIdx.x;           // b * 1212 + p
    const int b = (int)(row / kAstPatches), p = (int)(row - (size_t)b * kAstPatches);
    const int fh = p / kAstT, tw = p - fh * kAstT;
    const int kh = threadIdx.x >> 4, kw = threadIdx.x & 15;
    const float v = fbank[((size_t)b * kAstFrames + 10 * tw + kw) * kAstMel + 10 * fh + kh];
    const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
    const size_t o = tm_bf16(row, threadIdx.x, 256);
    p_hi[o] = __builtin_bit_cast(f16raw, hi);
    p_lo[o] = __builtin_bit_cast(f16raw, lo);
}

// ---------------------------------------------------------------------------------------------- LayerNorm rows
// fp32 tile-major in -> two fp16 planes, tile-major.  The thread mapping and the order of every sum are those of k_ln_bf16 (k_audio.hip): one
// workgroup per 16-row tile row, wave w owns the feature tiles 6 w .. 6 w + 5; a row's result does not depend on where in the batch it sits.
__global__ __launch_bounds__(256) void k_ln_x(const float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                              f16raw* __restrict__ out_hi, f16raw* __restrict__ out_lo) {
    __shared__ float red[2][4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
    const size_t tile0 = (size_t)blockIdx.x * (kAstDim / 32) + 6 * wave;
    const float* x = X + tile0 * 512 + lane * 4;
    f32x4 v[6][2];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        v[t][0] = ld4(x + t * 512);
        v[t][1] = ld4(x + t * 512 + 256);
        s += ((v[t][0][0] + v[t][0][1]) + (v[t][0][2] + v[t][0][3])) + ((v[t][1][0] + v[t][1][1]) + (v[t][1][2] + v[t][1][3]));
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0) red[0][wave][j] = s;
    __syncthreads();
    const float mean = ((red[0][0][j] + red[0][1][j]) + (red[0][2][j] + red[0][3][j])) * (1.0f / kAstDim);
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float d = v[t][h][m] - mean;
                q += d * d;
            }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    if (g == 0) red[1][wave][j] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf(((red[1][0][j] + red[1][1][j]) + (red[1][2][j] + red[1][3][j])) * (1.0f / kAstDim) + eps);
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int f = 32 * (6 * wave + t) + 8 * g;
        f32x4 y[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 ga = ld4(gamma + f + 4 * h), be = ld4(beta + f + 4 * h);
#pragma unroll
            for (int m = 0; m < 4; ++m) y[h][m] = (v[t][h][m] - mean) * rstd * ga[m] + be[m];
        }
        const F16Pair pr = split_f16(y[0], y[1]);
        const size_t o = (tile0 + t) * 512 + lane * 8;
        *reinterpret_cast<uint4*>(out_hi + o) = __builtin_bit_cast(uint4, pr.hi);
        *reinterpret_cast<uint4*>(out_lo + o) = __builtin_bit_cast(uint4, pr.lo);
    }
}

// ---------------------------------------------------------------------------------------------- attention
// The operand layouts of k_ast_attn (k_audio.hip), as two planes each: Q, K tiles of QK [B * 1216][1536] (q pre-scaled by the qkv epilogue
// before its split), V^T tiles of Vt [B * 768][1216 key slots].  Workgroup = 128 queries of one head (8 waves x ONE query tile, at every
// clip count: a query's bits cannot depend on the batch); keys in chunks of 64 - 8 K tiles + 8 V^T tiles, hi and lo: 32 KiB - through a
// ring of three LDS stages by DMA, two chunks in flight, one barrier per chunk.  Per chunk and wave: 24 score MFMAs, 24 for P.V, 4 for
// the row sums (the ones fragment of k_ast_attn against P's hi and lo pieces: the sum of the split P the product uses, in fp32).
// max of three.  Built with -fno-honor-nans (Makefile), NOT inline asm: k_audio.hip max3 has the reasons.
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
constexpr int kAttnXQ = 128;
constexpr int kAttnXStage = 32 * 1024;   // K hi (u, s) at 2 u + s | K lo at 8 + 2 u + s | V^T hi (td, pr) at 16 + 2 td + pr | V^T lo at 24 + 2 td + pr
constexpr int kAttnXLds = 3 * kAttnXStage;   // 96 KiB: one workgroup per CU, two waves per SIMD (256 registers each)
constexpr int kAttnChunks = kAstRows / 64;   // 19
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_ast_attn_x(const f16raw* __restrict__ QKh, const f16raw* __restrict__ QKl,
                                                                                              const f16raw* __restrict__ Vth, const f16raw* __restrict__ Vtl,
                                                                                              f16raw* __restrict__ Oh, f16raw* __restrict__ Ol) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = lane >> 4;
    const int qb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    constexpr int kRowTiles = kAstRows / 16, kQkTiles = 2 * kAstDim / 32, kSlotTiles = kAstRows / 32;   // 76, 48, 38
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)smem;
    const unsigned voff = lane * 16;
    // this wave's four DMA pieces of chunk c: waves 0..3 the K tiles of key tile 4 c + wave (k-steps 0, 1; hi, lo), waves 4..7 the V^T tiles
    // of row tile 4 h + wave - 4 (slot tiles 2 c, 2 c + 1; hi, lo)
    const bool kwave = wave < 4;
    const size_t soff = kwave ? (((size_t)b * kRowTiles + wave) * kQkTiles + kAstDim / 32 + 2 * h) * 1024
                              : ((size_t)b * (kAstDim / 16) + 4 * h + wave - 4) * kSlotTiles * 1024;
    const char* src_h = reinterpret_cast<const char*>(kwave ? QKh : Vth) + soff;
    const char* src_l = reinterpret_cast<const char*>(kwave ? QKl : Vtl) + soff;
    const size_t cstep = kwave ? (size_t)4 * kQkTiles * 1024 : (size_t)2 * 1024;
    const unsigned dsth = (kwave ? 2 * wave : 16 + 2 * (wave - 4)) * 1024, dstl = dsth + 8 * 1024;
    auto fetch = [&](int c, int slot) {
        c = c < kAttnChunks ? c : kAttnChunks - 1;   // past the end: the last chunk again (lands in a free slot, never read)
        const unsigned d = lds0 + slot * kAttnXStage;
        glds16s(src_h + c * cstep, voff, d + dsth);
        glds16s(src_h + c * cstep + 1024, voff, d + dsth + 1024);
        glds16s(src_l + c * cstep, voff, d + dstl);
        glds16s(src_l + c * cstep + 1024, voff, d + dstl + 1024);
    };
    fetch(0, 0);
    fetch(1, 1);
    const int qt = 8 * qb + wave;        // this wave's query tile of the clip's 76
    f16x8 qh[2], ql[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        uint4 uh = uint4{0, 0, 0, 0}, ul = uint4{0, 0, 0, 0};
        if (qt < kRowTiles) {
            const size_t o = (((size_t)b * kRowTiles + qt) * kQkTiles + 2 * h + s) * 1024 + voff;
            uh = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(QKh) + o);
            ul = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(QKl) + o);
        }
        qh[s] = __builtin_bit_cast(f16x8, uh);
        ql[s] = __builtin_bit_cast(f16x8, ul);
    }
    // the q fragments are waited for HERE (k_ast_attn): from here on only DMA is counted
#pragma unroll
    for (int s = 0; s < 2; ++s) asm volatile("" : "+v"(qh[s]), "+v"(ql[s]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // Scores arrive in the log2 domain and RELATIVE to the row's running maximum (the score MFMAs start from C = -m_run); the maximum moves only
    // when some score of the wave exceeds its row's by more than kAttnTau (lazy rescaling, amuse_dev.hpp): p <= 2^kAttnTau = 64
    const f16x8 ones = __builtin_bit_cast(f16x8, (lane & 15) == 0 ? uint4{0x3c003c00u, 0x3c003c00u, 0x3c003c00u, 0x3c003c00u} : uint4{0u, 0u, 0u, 0u});
    float m_run = 0.f;
    f32x4 os = splat4(0.f);
    f32x4 o[4];
#pragma unroll
    for (int td = 0; td < 4; ++td) o[td] = splat4(0.f);
    int slot = 0, fslot = 2;
#pragma unroll 1
    for (int c = 0; c < kAttnChunks; ++c) {
        // this wave's pieces of chunk c have landed (chunk c + 1 may still fly), its reads of chunk c - 1 are done; behind the
        // barrier chunk c is complete and the slot of chunk c - 1 is free for chunk c + 2
        if (c == 0) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        fetch(c + 2, fslot);
        fslot = fslot == 2 ? 0 : fslot + 1;
        const char* sl = smem + slot * kAttnXStage + lane * 16;
        slot = slot == 2 ? 0 : slot + 1;
        f32x4 st[4];
        const f32x4 c0 = splat4(-m_run);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f16x8 kh0 = *reinterpret_cast<const f16x8*>(sl + (2 * u) * 1024), kh1 = *reinterpret_cast<const f16x8*>(sl + (2 * u + 1) * 1024);
            const f16x8 kl0 = *reinterpret_cast<const f16x8*>(sl + (8 + 2 * u) * 1024), kl1 = *reinterpret_cast<const f16x8*>(sl + (8 + 2 * u + 1) * 1024);
            st[u] = mfma_f16(kl0, qh[0], c0);
            st[u] = mfma_f16(kl1, qh[1], st[u]);
            st[u] = mfma_f16(kh0, ql[0], st[u]);
            st[u] = mfma_f16(kh1, ql[1], st[u]);
            st[u] = mfma_f16(kh0, qh[0], st[u]);
            st[u] = mfma_f16(kh1, qh[1], st[u]);
        }
        // lane (g, query j): log2-domain S[j][key = 64 c + 16 u + 4 g + m] - m_run[j]
        if (c == kAttnChunks - 1) {   // keys 1214, 1215 are the clip's pad rows
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (64 * c + 16 * u + 4 * g + m >= kAstTokens) st[u][m] = -INFINITY;
        }
        float mx = max3(max3(st[0][0], st[0][1], st[0][2]), max3(st[0][3], st[1][0], st[1][1]), max3(st[1][2], st[1][3], st[2][0]));
        mx = max3(mx, max3(st[2][1], st[2][2], st[2][3]), max3(st[3][0], st[3][1], st[3][2]));
        mx = fmaxf(mx, st[3][3]);   // this lane's 16 scores; every chunk holds a valid key
        if (c == 0 || __builtin_amdgcn_ballot_w64(mx > kAttnTau) != 0) {   // (wave-uniform)
            mx = allreduce_g_max(mx);   // the same in the four lanes of a row
            const float d = c == 0 ? mx : fmaxf(mx, 0.f);
#pragma unroll
            for (int u = 0; u < 4; ++u) st[u] -= splat4(d);
            const float alpha = c == 0 ? 0.f : __builtin_amdgcn_exp2f(-d);   // (chunk 0: o = l = 0, and exp2(-d) may overflow)
            os *= alpha;
#pragma unroll
            for (int td = 0; td < 4; ++td) o[td] *= alpha;
            m_run += d;
        }
        f32x4 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int m = 0; m < 4; ++m) p[u][m] = __builtin_amdgcn_exp2f(st[u][m]);   // masked keys: exp2(-inf) = 0
        // k-slots (g, e) of key group pr: e < 4 -> tile 2 pr key 4 g + e, else tile 2 pr + 1 key 4 g + e - 4: the V^T slot order
        F16Pair pp[2];
        pp[0] = split_f16(p[0], p[1]);
        pp[1] = split_f16(p[2], p[3]);
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            f16x8 vh[4], vl[4];
#pragma unroll
            for (int td = 0; td < 4; ++td) {
                vh[td] = *reinterpret_cast<const f16x8*>(sl + (16 + 2 * td + pr) * 1024);
                vl[td] = *reinterpret_cast<const f16x8*>(sl + (24 + 2 * td + pr) * 1024);
            }
#pragma unroll
            for (int td = 0; td < 4; ++td) o[td] = mfma_f16(vl[td], pp[pr].hi, o[td]);
#pragma unroll
            for (int td = 0; td < 4; ++td) o[td] = mfma_f16(vh[td], pp[pr].lo, o[td]);
#pragma unroll
            for (int td = 0; td < 4; ++td) o[td] = mfma_f16(vh[td], pp[pr].hi, o[td]);
        }
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            os = mfma_f16(ones, pp[pr].lo, os);
            os = mfma_f16(ones, pp[pr].hi, os);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the surplus fetches must not outlive the workgroup's LDS
    // o[td][m] = O[query j][feature 64 h + 32 (td >> 1) + 8 g + 4 (td & 1) + m]: the pair td = 2 t, 2 t + 1 is this lane's slot of tile 2 h + t
    if (qt >= kRowTiles) return;
    const float inv = 1.0f / allreduce_g_sum(os[0]);
    const size_t dst = (((size_t)b * kRowTiles + qt) * (kAstDim / 32) + 2 * h) * 1024 + voff;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const F16Pair ov = split_f16(o[2 * tt] * inv, o[2 * tt + 1] * inv);
        *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Oh) + dst + tt * 1024) = __builtin_bit_cast(uint4, ov.hi);
        *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Ol) + dst + tt * 1024) = __builtin_bit_cast(uint4, ov.lo);
    }
}

// ---------------------------------------------------------------------------------------------- head
// feature_head: LayerNorm(768, eps 1e-5) -> Linear(768 -> 256), all fp32: the input of k_ast_head (k_audio.hip), its statistics and their
// order; the product on fp32 FMAs over k in ascending order, weights TRANSPOSED [768][256] so that a k-step is one contiguous row
__global__ __launch_bounds__(256) void k_ast_head_x(const float* __restrict__ pooled /*[B][kAstPoolSplit][768] row sums*/, float inv_rows,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ Wt /*[768][256]*/,
                                                    const float* __restrict__ bias, float* __restrict__ out /*[B][256]*/) {
    __shared__ float h[kAstDim];
    __shared__ float red[2][4];
    const int t = threadIdx.x, b = blockIdx.x;
    const float* x = pooled + (size_t)b * kAstPoolSplit * kAstDim;
    float v[3], s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // mean over the pooled rows: the slices of k_ast_pool, added in slice order
        float a = 0.f;
        for (int y = 0; y < kAstPoolSplit; ++y) a += x[y * kAstDim + t + 256 * i];
        v[i] = a * inv_rows;
        s += v[i];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((t & 63) == 0) red[0][t >> 6] = s;
    __syncthreads();
    const float mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * (1.0f / kAstDim);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float d = v[i] - mean; q += d * d; }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if ((t & 63) == 0) red[1][t >> 6] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * (1.0f / kAstDim) + 1e-5f);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = t + 256 * i;
        h[c] = (v[i] - mean) * rstd * gamma[c] + beta[c];
    }
    __syncthreads();
    float acc = 0.f;
    for (int c = 0; c < kAstDim; ++c) acc = fmaf(Wt[(size_t)c * kAstFeat + t], h[c], acc);
    out[(size_t)b * kAstFeat + t] = acc + bias[t];
}

}  // namespace

hipError_t launch_im2col_x(const float* fbank, unsigned short* p_hi, unsigned short* p_lo, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_im2col_x, dim3(B * kAstPatches), dim3(256), 0, s, fbank, p_hi, p_lo, B);
    return hipGetLastError();
}
hipError_t launch_ln_x(const float* X, const float* gamma, const float* beta, float eps, unsigned short* out_hi, unsigned short* out_lo, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_ln_x, dim3((M + 15) / 16), dim3(256), 0, s, X, gamma, beta, eps, out_hi, out_lo);
    return hipGetLastError();
}
hipError_t launch_ast_attn_x(const unsigned short* qk_hi, const unsigned short* qk_lo, const unsigned short* vt_hi, const unsigned short* vt_lo,
                             unsigned short* o_hi, unsigned short* o_lo, int B, hipStream_t s) {
    static DeviceOnce once;
    int dev_;
    if (!once.done(&dev_)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ast_attn_x), hipFuncAttributeMaxDynamicSharedMemorySize, kAttnXLds);
        if (e != hipSuccess) return e;
        once.set(dev_);
    }
    hipLaunchKernelGGL(k_ast_attn_x, dim3((kAstRows + kAttnXQ - 1) / kAttnXQ, kAstHeads, B), dim3(512), kAttnXLds, s, qk_hi, qk_lo, vt_hi, vt_lo, o_hi, o_lo);
    return hipGetLastError();
}
hipError_t launch_ast_head_x(const float* pooled, int frame_based, const float* gamma, const float* beta, const float* Wt, const float* bias, float* out,
                             int B, hipStream_t s) {
    const float inv_rows = 1.0f / (float)(frame_based ? kAstTokens - 2 : 2);
    hipLaunchKernelGGL(k_ast_head_x, dim3(B), dim3(256), 0, s, pooled, inv_rows, gamma, beta, Wt, bias, out);
    return hipGetLastError();
}

}  // namespace amuse
