// The audio front-end's GEMM in the parity mode (amuse_audio_set_precision AMUSE_PREC_F32X): C = A . W^T + bias with a fused epilogue on
// SPLIT fp16 operands - x = hi + lo, hi = rn16(x), lo = rn16(x - hi) - and fp32 accumulation: per fragment pair three
// v_mfma_f32_16x16x32_f16, Wl.xh + Wh.xl + Wh.xh (small terms first; the lo.lo term, 2^-22 relative, is dropped).
//
// The same tile-major discipline as k_gemm_tm (k_audio_gemm.hip, whose header has the reasons): both operands travel global -> LDS by
// LDS-DMA, 1 KiB of whole cache lines per instruction straight into fragment order; an activation is two fp16 planes each laid out as
// the bf16 matrix of the throughput mode, the weights are hi | lo unit pairs in the fragment order of pack_w (amuse_audio_x.hpp).
//   * 128 features x 128 tokens per workgroup, k-steps of 32: a stage is 8 W fragments x (hi, lo) + 8 X fragments x (hi, lo) = 32 KiB -
//     operand bytes per tile double against the bf16 kernel, so the tile is its narrow shape; a ring of FOUR stages (128 KiB + the bias
//     tile: ONE workgroup per CU, which may hold all 160 KiB), three stages in flight.  ONE shape for every launch: a row's bits
//     cannot depend on the clip count.
//   * four waves of 64 features x 64 tokens: 64 accumulator registers, 16 fragment reads per 48 MFMAs.  The fragments of stage s + 1
//     are read into registers while stage s is multiplied; one barrier per stage; the eight DMA instructions of a stage are issued two
//     per MFMA group.  The three MFMAs of a product go out term-major over the token fragments, so consecutive MFMAs never hit the
//     same accumulator.
//   * epilogue in registers (a lane holds 8 consecutive features of a token row).  An epilogue that writes an operand splits in
//     registers and writes both planes, one whole tile per wave instruction.  Every stage waits strictly (vmcnt counts the epilogue's
//     stores too: they only make a wait longer).
// GELU here is the exact erf form (amuse_dev.hpp gelu_erf_bf, fp32 rounding class): the bf16 kernel's clamped polynomial is 1.9e-4 off.
#include <cstdlib>
#include <type_traits>

#include "amuse_dev.hpp"
#include "amuse_audio_x.hpp"
#include "amuse_kernels.hpp"   // DeviceOnce

namespace amuse {
namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int kColGroup = 3;   // feature tiles per column group of the tile walk (as k_gemm_tm)
constexpr int TM = kGemmXTM, TN = kGemmXTN, BK = 32;
constexpr int XFR = TM / 16, WFR = TN / 16;          // token / feature fragments of a tile: 8, 8
constexpr int FX = WFR / 2;                          // feature fragments of a wave: 4
constexpr int NSLOT = 4;
constexpr int kOffX = 2 * WFR * 1024;                // stage: W fragment x -> units 2 x (hi), 2 x + 1 (lo) | X hi fragments | X lo fragments
constexpr int STAGE = kOffX + 2 * XFR * 1024;        // 32 KiB
constexpr int kOffBias = NSLOT * STAGE;              // [TN] float: the bias of the current tile's features
constexpr int kGemmXLds = kOffBias + 1024;           // 132,096 B
constexpr int PW = 8;                                // DMA pieces of a wave per stage: 2 W fragment rows x (hi, lo), 2 X fragment rows x (hi, lo)
static_assert(kGemmXLds <= 160 * 1024, "one workgroup per CU");

// LDS-DMA: 64 lanes x 16 B from (wave-uniform base + 32-bit lane offset) to LDS [dst, dst + 1 KiB), lane-linear (k_audio_gemm.hip)
__device__ __forceinline__ void glds16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}
__device__ __forceinline__ f32x4 gelu4(f32x4 v) { return f32x4{gelu_erf_bf(v[0]), gelu_erf_bf(v[1]), gelu_erf_bf(v[2]), gelu_erf_bf(v[3])}; }

template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gemm_x(GemmXArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), g = lane >> 4, j = lane & 15;
    const int wf = wave >> 1, wr = wave & 1;   // feature half (64), token half (64) of the tile
    const int N = a.N;
    const int tiles_n = N / TN, tiles_m = (a.M + TM - 1) / TM, n_tiles = tiles_n * tiles_m, nk = a.K / BK;
    // PERSISTENT: workgroup w computes tiles w, w + grid, ...; each XCD gets a contiguous range of w (k_gemm_tm)
    int wg = blockIdx.x;
    if ((gridDim.x & 7) == 0) wg = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (wg >= n_tiles) return;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)smem;
    const unsigned voff = lane * 16;
    // fetch cursor (wave-uniform): the stage fetched next = k-step f_k of tile f_tile into slot f_slot.  This wave's pieces of a stage:
    // W fragment rows 2 wave, + 1 (a k-step of a row is 2 KiB: hi | lo), X fragment rows 2 wave, + 1 of both planes
    int f_tile = wg, f_k = 0, f_slot = 0;
    const size_t w_row = (size_t)nk * 2048, x_row = (size_t)nk * 1024;   // bytes between consecutive fragment rows
    const char *fw, *fxh, *fxl;
    const int cg = tiles_n % kColGroup == 0 ? kColGroup : tiles_n;
    auto tile_tm = [&](int tile) { return (tile % (tiles_m * cg)) / cg; };
    auto tile_tn = [&](int tile) { return (tile / (tiles_m * cg)) * cg + tile % cg; };
    auto cursor = [&]() {
        fw = reinterpret_cast<const char*>(a.W) + (size_t)(tile_tn(f_tile) * WFR + 2 * wave) * w_row;
        const size_t xo = (size_t)(tile_tm(f_tile) * XFR + 2 * wave) * x_row;
        fxh = reinterpret_cast<const char*>(a.A_hi) + xo;
        fxl = reinterpret_cast<const char*>(a.A_lo) + xo;
    };
    cursor();
    auto fetch_piece = [&](int i) {   // i = 0..7 (compile-time after unrolling)
        const unsigned d = lds0 + f_slot * STAGE;
        const int r = (i >> 1) & 1, lo = i & 1;   // fragment row of the wave's two, plane
        if (i < 4) glds16s(fw + r * w_row + (size_t)f_k * 2048 + lo * 1024, voff, d + (2 * (2 * wave + r) + lo) * 1024);
        else glds16s((lo ? fxl : fxh) + r * x_row + (size_t)f_k * 1024, voff, d + kOffX + (lo * XFR + 2 * wave + r) * 1024);
    };
    auto fetch_advance = [&]() {
        f_slot = f_slot == NSLOT - 1 ? 0 : f_slot + 1;
        if (++f_k == nk) {
            f_k = 0;
            const int nt = f_tile + gridDim.x;
            f_tile = nt < n_tiles ? nt : f_tile;   // past the end: the last tile again (lands in a free slot, never read)
            cursor();
        }
    };
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
#pragma unroll
        for (int i = 0; i < PW; ++i) fetch_piece(i);
        fetch_advance();
    }
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PW * (NSLOT - 1)) : "memory");
    f16x8 wh[FX], wl[FX], xah[4], xal[4], xbh[4], xbl[4];
    {
        const char* sl = smem + lane * 16;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            xah[y] = *reinterpret_cast<const f16x8*>(sl + kOffX + (4 * wr + y) * 1024);
            xal[y] = *reinterpret_cast<const f16x8*>(sl + kOffX + (XFR + 4 * wr + y) * 1024);
        }
#pragma unroll
        for (int x = 0; x < FX; ++x) {
            wh[x] = *reinterpret_cast<const f16x8*>(sl + (2 * (FX * wf + x)) * 1024);
            wl[x] = *reinterpret_cast<const f16x8*>(sl + (2 * (FX * wf + x) + 1) * 1024);
        }
    }
    int r_slot = 1;
    f32x4 acc[FX][4];   // [feature fragment][token fragment]
    // one k-step: (xch, xcl) = this stage's X fragments (registers), (xnh, xnl) receive the next stage's.
    // swapped: the X fragment is the MFMA's A operand, so a lane ends up with 4 consecutive TOKENS of one feature (the V^T tiles)
    auto half = [&](auto swapped, f16x8 (&xch)[4], f16x8 (&xcl)[4], f16x8 (&xnh)[4], f16x8 (&xnl)[4], int bias_tile) {
        constexpr bool SW = decltype(swapped)::value;
        // this wave's pieces of the NEXT stage have landed (the NSLOT - 2 younger stages may still fly) and its reads of this stage are in
        // registers; behind the barrier that holds for every wave: the next stage is complete, this stage's slot is free
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(PW * (NSLOT - 2)) : "memory");
        if (bias_tile >= 0 && wave == 0)   // (every wave's epilogue reads of the previous tile's bias are in front of this barrier)
            glds16s(a.bias + (size_t)bias_tile * TN, (lane % (TN / 4)) * 16, lds0 + kOffBias);   // (512 B: the upper lanes repeat the lower half)
        const char* sl = smem + r_slot * STAGE + lane * 16;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            xnh[y] = *reinterpret_cast<const f16x8*>(sl + kOffX + (4 * wr + y) * 1024);
            xnl[y] = *reinterpret_cast<const f16x8*>(sl + kOffX + (XFR + 4 * wr + y) * 1024);
        }
#pragma unroll
        for (int x = 0; x < FX; ++x) {
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = SW ? mfma_f16(xch[y], wl[x], acc[x][y]) : mfma_f16(wl[x], xch[y], acc[x][y]);
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = SW ? mfma_f16(xcl[y], wh[x], acc[x][y]) : mfma_f16(wh[x], xcl[y], acc[x][y]);
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = SW ? mfma_f16(xch[y], wh[x], acc[x][y]) : mfma_f16(wh[x], xch[y], acc[x][y]);
            wh[x] = *reinterpret_cast<const f16x8*>(sl + (2 * (FX * wf + x)) * 1024);
            wl[x] = *reinterpret_cast<const f16x8*>(sl + (2 * (FX * wf + x) + 1) * 1024);
            fetch_piece(2 * x);
            fetch_piece(2 * x + 1);
            if (x == FX - 1) fetch_advance();
            __builtin_amdgcn_sched_barrier(0);   // (keeps the scheduler from hoisting every read to the top)
        }
        r_slot = r_slot == NSLOT - 1 ? 0 : r_slot + 1;
    };
    for (int tile = wg; tile < n_tiles; tile += gridDim.x) {
        const int tm = tile_tm(tile), tn = tile_tn(tile);
#pragma unroll
        for (int x = 0; x < FX; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = splat4(0.f);
        const bool vt_tile = EPI == EPI_QKV && tn >= 2 * kAstDim / TN;   // (uniform)
        if (EPI == EPI_QKV && vt_tile) {
#pragma unroll 1
            for (int kp = 0; kp < nk; kp += 2) {
                half(std::true_type{}, xah, xal, xbh, xbl, kp == 0 ? tn : -1);
                half(std::true_type{}, xbh, xbl, xah, xal, -1);
            }
        } else {
#pragma unroll 1
            for (int kp = 0; kp < nk; kp += 2) {
                half(std::false_type{}, xah, xal, xbh, xbl, kp == 0 ? tn : -1);
                half(std::false_type{}, xbh, xbl, xah, xal, -1);
            }
        }
        // ---- epilogue: lane (g, j): token row m0 + 16 y + j, features n0 + 32 p + 8 g .. + 7 = acc[2 p][y], acc[2 p + 1][y]
        const int m0 = tm * TM + 64 * wr, n0 = tn * TN + 16 * FX * wf;
        if (EPI == EPI_QKV && vt_tile) {
            // V^T (swapped MFMAs): lane (g, j) holds row j of feature fragment x - V^T row 16 F + j, F = the fragment's index among the 48 of
            // v - and tokens 16 y + 4 g + m of the wave's 64-row span; key slot order and tile addressing as in k_gemm_tm
            const float* bw = reinterpret_cast<const float*>(smem + kOffBias) + 16 * FX * wf;
            const int b = m0 / kAstRows, tok0 = m0 - b * kAstRows;
            if (m0 >= a.M) continue;   // (the pad half of the last row tile: no clip owns it)
#pragma unroll
            for (int x = 0; x < FX; ++x) {
                const float bv = bw[32 * (x >> 1) + 8 * (j >> 2) + 4 * (x & 1) + (j & 3)];   // fragment row j <-> this feature (pack_w)
                const size_t rt = (size_t)b * (kAstDim / 16) + ((n0 - 2 * kAstDim) >> 4) + x;   // row tile of the V^T matrix
#pragma unroll
                for (int Y = 0; Y < 2; ++Y) {
                    const F16Pair v = split_f16(acc[x][2 * Y] + splat4(bv), acc[x][2 * Y + 1] + splat4(bv));
                    const size_t off = (rt * (kAstRows / 32) + ((tok0 >> 5) + Y)) * 1024 + voff;
                    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.vt_hi) + off) = __builtin_bit_cast(u32x4, v.hi);
                    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.vt_lo) + off) = __builtin_bit_cast(u32x4, v.lo);
                }
            }
            continue;
        }
        const float* bl = reinterpret_cast<const float*>(smem + kOffBias) + 16 * FX * wf + 8 * g;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const size_t tile0 = (size_t)((m0 >> 4) + y) * (N >> 5) + (n0 >> 5);   // tile-major outputs: tile index of p = 0
            const size_t row = (size_t)m0 + 16 * y + j;
#pragma unroll
            for (int p = 0; p < FX / 2; ++p) {
                const int n = n0 + 32 * p + 8 * g;
                f32x4 v0 = acc[2 * p][y] + ld4(bl + 32 * p), v1 = acc[2 * p + 1][y] + ld4(bl + 32 * p + 4);
                if constexpr (EPI == EPI_GELU_BF16) {
                    const F16Pair v = split_f16(gelu4(v0), gelu4(v1));
                    __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v.hi), reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.out_hi) + (tile0 + p) * 1024 + voff));
                    __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v.lo), reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.out_lo) + (tile0 + p) * 1024 + voff));
                } else if constexpr (EPI == EPI_RESID_F32) {
                    float* c = reinterpret_cast<float*>(reinterpret_cast<char*>(a.out_f32) + (tile0 + p) * 2048 + voff);
                    v0 += ld4(c);
                    v1 += ld4(c + 256);
                    st4(c, v0);
                    st4(c + 256, v1);
                } else if constexpr (EPI == EPI_PATCH) {
                    // patch row = b * 1212 + q  ->  token row b * 1216 + 2 + q, + pos_embed[2 + q]
                    if (row < (size_t)a.M) {
                        const size_t b = row / kAstPatches, q = row - b * kAstPatches;
                        float* dst = a.out_f32 + tm_f32(b * kAstRows + 2 + q, n, kAstDim);
                        const float* ps = a.pos + (2 + q) * kAstDim + n;
                        st4(dst, v0 + ld4(ps));
                        st4(dst + 256, v1 + ld4(ps + 4));
                    }
                } else {  // EPI_QKV, q | k tiles, planes [M][1536]; q pre-scaled by head_dim ** -0.5 * log2(e) BEFORE the split: the attention's
                          // scores are exp2 arguments as they leave its MFMAs
                    const float sc = n < kAstDim ? 0.125f * 1.44269504088896340736f : 1.0f;
                    const F16Pair v = split_f16(v0 * sc, v1 * sc);
                    const size_t off = ((size_t)((m0 >> 4) + y) * (2 * kAstDim / 32) + (n0 >> 5) + p) * 1024 + voff;
                    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.out_hi) + off) = __builtin_bit_cast(u32x4, v.hi);
                    *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.out_lo) + off) = __builtin_bit_cast(u32x4, v.lo);
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the surplus fetches must not outlive the workgroup's LDS
}

template <int EPI>
hipError_t launch_gemm_x_t(const GemmXArgs& a, hipStream_t s) {
    static DeviceOnce once;
    int dev_;
    if (!once.done(&dev_)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_x<EPI>), hipFuncAttributeMaxDynamicSharedMemorySize, kGemmXLds);
        if (e != hipSuccess) return e;
        once.set(dev_);
    }
    const int n_tiles = (a.M + TM - 1) / TM * (a.N / TN);
    const int resident = 256;   // one workgroup per CU, 256 CUs
    hipLaunchKernelGGL((k_gemm_x<EPI>), dim3(n_tiles < resident ? n_tiles : resident), dim3(256), kGemmXLds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gemm_x(const GemmXArgs& a, int epi, hipStream_t s) {
    if (a.N % TN || a.K % (2 * BK) || a.K / BK < NSLOT || a.M < 1) return hipErrorInvalidValue;
    switch (epi) {
        case EPI_GELU_BF16: return launch_gemm_x_t<EPI_GELU_BF16>(a, s);
        case EPI_RESID_F32: return launch_gemm_x_t<EPI_RESID_F32>(a, s);
        case EPI_PATCH: return launch_gemm_x_t<EPI_PATCH>(a, s);
        case EPI_QKV: return launch_gemm_x_t<EPI_QKV>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace amuse
