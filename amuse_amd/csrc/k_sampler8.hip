// bf16 throughput variant of the persistent sampling kernel (k_sampler.hip has the design notes and the fp32
// parity kernel): the same T-step loop of PretrainedLPDM_v1.diffusion_backward (reference
// models/latent_diffusion/infer_ldm.py:137-161; Denoiser.forward denoiser.py:135-204; encoder blocks
// cross_attention.py:41-64,259-272; diffusers scheduler step) with EIGHT wavefronts per workgroup instead of four.
//
// Why: a wave's global_load blocks at issue while the CU's 64 B/clk vector-memory path is busy, so in the 4-wave
// kernel the weight fetch (3.8 MB per step and CU) and the MFMA / LDS / barrier chain of the SAME waves add up
// instead of overlapping.  Here the two halves of a block belong to different waves, and each
// group fetches its weights while the OTHER group is on the critical path:
//
//   wave w8 = 4 s + h.
//   Group A (s = 0): head h end to end (in_proj, attention, out_proj split-K) and FFN quarters 0,1 of head h's
//     slice.  It never reduces: in both combines it publishes its partial and then only waits for the result -
//     that is where it fetches its weights (the FFN half during the out_proj combine, the next block's attention
//     weights during the linear2 combine).
//   Group B (s = 1): reduces + normalises BOTH combines (wave h: feature tiles 2h, 2h+1) and computes FFN quarters
//     2,3.  It has nothing to do while the A waves run attention - that is where it fetches its FFN half.
//   So no wave issues a weight load while it is on the critical path (bar the B waves' 8-unit skip-linear groups), and the
//   FFN's MFMA + GELU work is spread over two waves per SIMD.
//   U-Net skip linears x = Linear(cat(x, skip)): split over OUTPUT tiles - B wave h computes its own feature tiles
//     2h, 2h+1 from the x half of the weights plus u = W[:, 128:] . skip, which A wave h prepared in its waiting time of
//     the previous linear2 combine; one barrier, no partial sums.  The skip stack is kept as packed bf16 MFMA
//     operands (what the 4-wave kernel's cvt_pk produces from its fp32 copy - same bits).
//   The residual stream travels between waves as packed bf16 MFMA operands (4 x 1 KiB per tile - what every GEMM
//   consumes); only the reducer of a feature tile keeps it in fp32 (the B waves, two tiles each, in registers).
//   Final LayerNorm + scheduler update in the B waves on their own tiles; latent in LDS.  With the updated latent of its two tiles still in
//   registers a B wave also assembles the NEXT step's input for them (latent + pe[0] | time token | condition tokens: amuse_sample8.hpp
//   assemble_own) and publishes it like a combine's result, so a step starts with that combine's four-read gather in every wave.
//
// LDS (163,328 B): combine matrix A8 [8 rows][8 tiles][64] f32x4 - fp32 partials off the diagonal, the published
// bf16 operands ON it (slots (c, c), c < 4), so the gather of one combine never aliases the partial writes of the
// next - | row statistics (and, in their reservation's last 32 B, the step's scheduler coefficients) | bf16 skip stack | small
// parameters | static token rows | latent | double-buffered time token.
#include "amuse_sample8.hpp"

// This file is compiled twice: as is (bf16 operands: k_sample8 / launch_sample8) and through k_sampler8h.hip with AMUSE_OP_F16
// defined (fp16 operands, AMUSE_PREC_F16: k_sample8h / launch_sample8h) - the same instruction stream on v_mfma_f32_16x16x32_f16
// with v_cvt_pk_f16_f32 and a GELU polynomial one degree higher; the stream holds fp16 weights.
#ifdef AMUSE_OP_F16
#define OPV f16x8
#define OP_PACK pack_f16
#define OP_MFMA mfma_f16
#define OP_PREC PREC_F16
#define OP_GELU gelu_poly4h
#define OP_KERNEL k_sample8h
#define OP_LAUNCH launch_sample8h
#else
#define OPV bf16x8
#define OP_PACK pack_bf16
#define OP_MFMA mfma_bf16
#define OP_PREC PREC_BF16
#define OP_GELU gelu_poly4
#define OP_KERNEL k_sample8
#define OP_LAUNCH launch_sample8
#endif

namespace amuse {

namespace {

// (amuse_sample8.hpp: combine matrix A8, then the row statistics at kStat8Off)
constexpr int kSkip8Off = kStat8Off + 8 * 16 * 8;              // [4 levels][4 pairs][64] uint4
constexpr int kCoef8Off = kSkip8Off - 32;                      // the step's 8 scheduler coefficients: the last 32 B of the statistics' 1 KiB, which use 512 B
constexpr int kPv8Off = kSkip8Off + 4 * 4 * 64 * 16;
constexpr int kPv8Floats = kLayers * kEncPv + 4 * kD + 2 * kD;
constexpr int kTokRows8Off = kPv8Off + kPv8Floats * 4;         // [8 tiles][64] f32x4
constexpr int kLat8Off = kTokRows8Off + kTiles * 64 * 16;      // [8 tiles][64] f32x4: the latent (rows tok == 0)
constexpr int kTT8Off = kLat8Off + kTiles * 64 * 16;           // [2][128] float
static_assert(kTT8Off + 2 * kD * 4 == kSample8LdsBytes, "LDS layout");

// Issue split of an A wave's 32 units inside the out_proj (C1) and linear2 (C2) combines: N0 before the first barrier
// (C2 only - there the A waves arrive early), N1 / N2 after the first / second barrier, the rest after the gather (C1: none
// since round 8 - kALate units go out from the FFN half instead).
// Values from sweeps on MI355X (rounds 1-4 and 8, docs/history.md 4.1b); all splits of the same family land within 2 %.
// kC1N2: 12 -> 10 together with kALate = 10 (N1, N2 = 16, 8 / 8, 16 with kALate = 8: 33.06 / 33.43 ms at 256 clips against 33.04 for 12, 12).
constexpr int kC1N1 = 12, kC1N2 = 10;
// kC2N0 swept again around the new FFN issue (8 / 12 / 16 / 20 / 24: 34.3 / 33.3 / 32.8 / 33.5 / 34.2 ms): stays.
constexpr int kC2N0 = 16, kC2N1 = 12;
// units a B wave issues during the A waves' attention phase; the rest of its 32 follow behind its first FFN MFMAs
// (18 / 20 / 21 / 22 / 23 / 24 / 26 with kALate = 8: 33.5 / 33.0 / 33.1 / 32.8 / 32.9 / 33.4 / 33.7 ms)
constexpr int kBEarly = 22;
// ... and go out in chunks of kDrawChunk with one slice of the step's noise draw behind each chunk (last block only, role_loop8): the ten Philox rounds spread
// over all slices but the last, which holds Box-Muller.  Behind the whole fetch - and behind a wait for it - the draw cost 1.4 k cycles of the step's chain; sliced
// it still costs 0.7 k (the four reducers draw at the same time, and an in-order wave blocked at a load cannot run the VALU work behind it), which is why the
// multiplies themselves were halved (amuse_dev.hpp philox4x32_round).  2 / 4 / 8 with the paired multiplies: 31.69 / 31.63 / 31.83 ms at 256 clips against 31.86;
// 2 / 4 with the 64-bit multiply: 31.94 / 31.42 against 31.90 (docs/history.md 4.1b, round 10).
constexpr int kDrawChunk = 4;
constexpr int kDrawSlices = (kBEarly + kDrawChunk - 1) / kDrawChunk;
constexpr int kDrawRounds = (10 + kDrawSlices - 2) / (kDrawSlices - 1);   // Philox rounds per slice
static_assert(kDrawSlices >= 2, "one slice of rounds, one of Box-Muller");
// units of an A wave's FFN half (its last ones, F2b and the tail of F2a) that go out behind ITS first FFN MFMAs instead of behind the out_proj
// combine's gather.  The reducers leave that gather at the same moment and need their own late units first (F2a reads them ~0.7 k cycles
// later, the A wave's F2b is the last thing it runs and it waits at the linear2 combine afterwards anyway): issued behind the gather, the A waves'
// 4 x 8 units sat in the CU's load path in front of them.  Not issuing them at all bounds this at 1.25 ms of 33.5 (tools/probes/ksample8_ffn_pacing);
// 0 / 4 / 8 / 10: 33.4 / 33.7 / 33.0 / 32.75 ms with kBEarly = 20 (0, 4, 8) and 22 (10).
constexpr int kALate = 10;
// VALU instructions scheduled behind each MFMA while one FFN quarter's GELU overlaps the other quarter's GEMM (ffn_half)
constexpr int kFfnValuPerMfma = 7;

// packed bf16 operand c (feature tiles 2c, 2c+1 of the residual stream) is published in diagonal slot (c, c)
__device__ __forceinline__ uint4* xb_slot(char* lds, int c, int lane) {
    return reinterpret_cast<uint4*>(a8_slot(lds, c, c, lane));
}
// acc[o] += W_o . x over the 128 features held as four packed operands; same unit order as gemm_ring (bf16)
template <int NO, bool SWAP, int PH>
__device__ __forceinline__ void gemm_xb(f32x4 (&acc)[NO], const OPV (&xb)[4], const Ring& rg) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const OPV wf = __builtin_bit_cast(OPV, rg.s[(PH + c * NO + o) % kR8]);
            acc[o] = SWAP ? OP_MFMA(xb[c], wf, acc[o]) : OP_MFMA(wf, xb[c], acc[o]);
        }
}

// ---- split-K combine, B waves reduce.  NP = 4: partials from the A waves only (out_proj); NP = 8: from all waves
// (linear2).  B wave h reduces feature tiles 2h, 2h+1: residual + bias, LayerNorm (row statistics of the four
// 32-feature slices merged with Chan's formula), publishes them on the diagonal of A8; every wave gathers.
// Partials travel through the rows part_row (amuse_sample8.hpp) assigns.
// LN = false (U-Net skip linear): tiles = sum + bias - no residual, no LayerNorm, and one barrier less.
template <int W, int NP, bool FAST, bool LN, bool DRP>
__device__ __forceinline__ void combine_red(f32x4 (&part)[kTiles], f32x4 (&xo)[2], OPV (&xb)[4], const float* bias,
                                            const float* gamma, const float* beta, char* lds, int lane, uint32_t dbits,
                                            float dscale) {
    float2* stats = reinterpret_cast<float2*>(lds + kStat8Off);
    const int g = lane >> 4, r = lane & 15;
    constexpr int T0 = 2 * W;
    if constexpr (NP == 8) {
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
            if (t != T0 && t != T0 + 1) *a8_slot(lds, part_row(4 + W, t), t, lane) = part[t];
    }
    f32x4 bi[2], ga[2], be[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        bi[i] = ld4(bias + 16 * (T0 + i) + 4 * g);
        if constexpr (LN) {
            ga[i] = ld4(gamma + 16 * (T0 + i) + 4 * g);
            be[i] = ld4(beta + 16 * (T0 + i) + 4 * g);
        }
    }
    __syncthreads();
    f32x4 y[2];
    {
        f32x4 p[NP][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int w = 0; w < NP; ++w) {
                if (w != 4 + W) p[w][i] = *a8_slot(lds, part_row(w, T0 + i), T0 + i, lane);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f32x4 sum;
            if constexpr (NP == 8) {
                p[4 + W][i] = part[T0 + i];
                sum = ((p[0][i] + p[1][i]) + (p[2][i] + p[3][i])) + ((p[4][i] + p[5][i]) + (p[6][i] + p[7][i]));
            } else {
                sum = ((p[0][i] + p[1][i]) + p[2][i]) + p[3][i];
            }
            f32x4 br = sum + bi[i];
            if constexpr (DRP) br = sdrop_apply4(br, dbits >> (4 * i), dscale);   // dropout1 / dropout2 (train-mode sampling)
            y[i] = LN ? xo[i] + br : br;
        }
    }
    if constexpr (LN) {
    const float2 st = row_stats32(y);
    if (g == 0) stats[W * 16 + r] = st;
    __syncthreads();
    const float2 ms = row_stats_merge<FAST>(stats, r);
    const float mean = ms.x, rstd = ms.y;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int m = 0; m < 4; ++m) y[i][m] = (y[i][m] - mean) * rstd * ga[i][m] + be[i][m];
    }
    xo[0] = y[0];
    xo[1] = y[1];
    // publish the two tiles as ONE packed bf16 operand (k-tile pair W of every following GEMM)
    xb[W] = OP_PACK(y[0], y[1]);
    *xb_slot(lds, W, lane) = __builtin_bit_cast(uint4, xb[W]);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c != W) xb[c] = __builtin_bit_cast(OPV, *xb_slot(lds, c, lane));
    // keeps SimplifyCFG from sinking the four cases' register-array stores into one block behind a pointer PHI (which
    // pins the arrays in scratch): an immediate operand cannot be merged
    asm volatile("; combine_red case %0" ::"n"(W));
}
// DRP: (sum + bias) of tile 2 h + i times sdrop_apply4(., dbits >> 4 i, dscale) before the residual add
template <int NP, bool FAST, bool LN = true, bool DRP = false>
__device__ __forceinline__ void combine_reduce(f32x4 (&part)[kTiles], f32x4 (&xo)[2], OPV (&xb)[4],
                                               const float* bias, const float* gamma, const float* beta, char* lds,
                                               int h, int lane, uint32_t dbits = 0, float dscale = 1.f) {
    if (h == 0) combine_red<0, NP, FAST, LN, DRP>(part, xo, xb, bias, gamma, beta, lds, lane, dbits, dscale);
    else if (h == 1) combine_red<1, NP, FAST, LN, DRP>(part, xo, xb, bias, gamma, beta, lds, lane, dbits, dscale);
    else if (h == 2) combine_red<2, NP, FAST, LN, DRP>(part, xo, xb, bias, gamma, beta, lds, lane, dbits, dscale);
    else combine_red<3, NP, FAST, LN, DRP>(part, xo, xb, bias, gamma, beta, lds, lane, dbits, dscale);
}
// The A waves' side: publish the partial, then the barriers and the gather - with the issue of N1 + N2 + N3
// weight-stream units into ring slots IPH0.. in between.  These waves are off the critical path here, so their
// blocking global_load issue costs nothing as long as it fits the reducers' phases.
// N0 units go out BEFORE the first barrier: free where the A waves arrive early (the linear2 combine - their FFN half
// is the shorter one), on the critical path where they arrive last (the out_proj combine: N0 = 0).
// hook: extra work of the waiting time behind the N1 units (train-mode sampling: this wave's FFN masks)
struct NoHook {
    __device__ void operator()() const {}
};
template <int N0, int N1, int N2, int N3, int IPH0, bool LN = true, class Hook = NoHook>
__device__ __forceinline__ void combine_publish(const f32x4 (&part)[kTiles], OPV (&xb)[4], char* lds, int h,
                                                int lane, Ring& rg, Hook hook = {}) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
        *a8_slot(lds, h + (h >= t ? 1 : 0), t, lane) = part[t];  // part_row(h, t), h < 4
    ring_issue<N0, kR8, IPH0 % kR8>(rg);
    __syncthreads();
    ring_issue<N1, kR8, (IPH0 + N0) % kR8>(rg);
    hook();
    if constexpr (LN) __syncthreads();   // (the reducers' row-statistics exchange)
    ring_issue<N2, kR8, (IPH0 + N0 + N1) % kR8>(rg);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) xb[c] = __builtin_bit_cast(OPV, *xb_slot(lds, c, lane));
    ring_issue<N3, kR8, (IPH0 + N0 + N1 + N2) % kR8>(rg);
}

// The A waves' side of the linear2 combine: as combine_publish, fetching the next block's group of 32 units - its
// first 8 units into slots 24..31, then q, k, v into slots 0..23.  In front of an ordinary block the leading 8 are out_proj.
// In front of an OUTPUT block (cross_attention.py:58-61: x = Linear(cat(x, skips.pop()))) they are this wave's units of
// the skip linear, and in its waiting time the wave computes u = W[:, 128:] . skip for feature tiles 2h, 2h+1 - the half
// of the skip linear that does not depend on the current block's result - and hands it to B wave h through u_slot
// (after the second barrier: the reducers are done with the partials).  out_proj then follows during the skip linear.
// One body for both cases, the extra work behind a branch that touches no ring slot: separate instantiations of the
// fetch make hipcc copy the ring registers at the merge - behind an s_waitcnt vmcnt that stalls the wave until its
// loads have landed, in front of the last barrier.
template <int N0, int N1, int N2>
__device__ __forceinline__ void combine_publish_c2(const f32x4 (&part)[kTiles], OPV (&xb)[4], char* lds, int h,
                                                   int lane, Ring& rg, bool skip_u, const uint4* skip_ops) {
    static_assert(N0 >= 8 && N0 + N1 + N2 == 32, "the leading 8 units go out before the first barrier");
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
        *a8_slot(lds, h + (h >= t ? 1 : 0), t, lane) = part[t];
    ring_issue<N0, kR8, 24>(rg);
    __syncthreads();
    ring_issue<N1, kR8, (24 + N0) % kR8>(rg);
    __syncthreads();
    if (skip_u) {
        OPV sk[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) sk[p] = __builtin_bit_cast(OPV, skip_ops[p * 64 + lane]);
        f32x4 u[2] = {splat4(0.f), splat4(0.f)};
        gemm_xb<2, false, 24>(u, sk, rg);
        *u_slot(lds, 2 * h, lane) = u[0];
        *u_slot(lds, 2 * h + 1, lane) = u[1];
    }
    ring_issue<N2, kR8, (24 + N0 + N1) % kR8>(rg);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) xb[c] = __builtin_bit_cast(OPV, *xb_slot(lds, c, lane));
}

// DROP: site 0 of train-mode sampling - probability m of this lane kept iff bit m of dbits
template <bool DROP = false>
__device__ __forceinline__ void attention_head8(const f32x4 (&q)[2], const f32x4 (&k)[2], const f32x4 (&v)[2],
                                                const bool (&kvalid)[4], f32x4 (&o)[2], uint32_t dbits = 0,
                                                float dscale = 1.f) {
    // S^T[j][i] = sum_d K[j][d] Q[i][d]  ->  lane (g, i) holds S[i][4 g + m]   (k_sampler.hip attention_head)
    f32x4 st = OP_MFMA(OP_PACK(k[0], k[1]), OP_PACK(q[0], q[1]), splat4(0.f));
    float mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < 4; ++m) mx = kvalid[m] ? fmaxf(mx, st[m]) : mx;
    mx = allreduce_g_max(mx);
    f32x4 p;
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float e = __builtin_amdgcn_exp2f(1.44269504088896340736f * (st[m] - mx));
        p[m] = kvalid[m] ? e : 0.f;
        sum += p[m];
    }
    sum = allreduce_g_sum(sum);
    const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
    for (int m = 0; m < 4; ++m) p[m] *= inv;
    if constexpr (DROP) p = sdrop_apply4(p, dbits, dscale);
#pragma unroll
    for (int td = 0; td < 2; ++td)
        o[td] = OP_MFMA(OP_PACK(v[td], splat4(0.f)), OP_PACK(p, splat4(0.f)), splat4(0.f));
}

// GELU (amuse_dev.hpp OP_GELU: the result is an MFMA operand, i.e. rounded to bf16 next) on one FFN quarter (two
// hidden tiles); linear1's bias is already in the accumulators (ffn_half)
// DROP: then the FFN's inner dropout (site 2), keep bits 0..3 / 4..7 of dbits for the two tiles
template <bool DROP>
__device__ __forceinline__ void gelu_pair(f32x4 (&hq)[2], uint32_t dbits, float dscale) {
    hq[0] = OP_GELU(hq[0]);
    hq[1] = OP_GELU(hq[1]);
    if constexpr (DROP) {
        hq[0] = sdrop_apply4(hq[0], dbits, dscale);
        hq[1] = sdrop_apply4(hq[1], dbits >> 4, dscale);
    }
}

// this wave's two FFN quarters (Q0, Q0 + 1 of head h's slice): linear1 for 2 hidden tiles each -> bias + GELU ->
// linear2 split-K contribution of those 32 features, software-pipelined by one quarter.  Ring: F1a F1b F2a F2b in
// slots 0..31, nothing re-armed.
// NLATE: the last NLATE units (slots 32 - NLATE .. 31) are issued only now, behind the first GEMM's MFMAs (B waves: their
// fetch window, the A waves' attention phase, is a little too short for all 32; A waves: kALate)
// DROP: site 2 keep bits of the four hidden tiles in dbits (bits 4 k + m: tile k of the half)
template <int Q0, int NLATE, bool DROP = false>
__device__ __forceinline__ void ffn_half(f32x4 (&part)[kTiles], const OPV (&xb)[4], Ring& rg, const float* pv,
                                         int h, int g, uint32_t dbits = 0, float dscale = 1.f) {
    constexpr int P = OP_PREC;
    // accumulators start at linear1's bias (this lane's 4 features of each hidden tile)
    const float* b1 = pv + PV_L1_B + 16 * (kTiles * h + 2 * Q0) + 4 * g;
    f32x4 ha[2] = {ld4(b1), ld4(b1 + 16)}, hb[2] = {ld4(b1 + 32), ld4(b1 + 48)};
    gemm_xb<2, false, 0>(ha, xb, rg);
    ring_issue<NLATE, kR8, 32 - NLATE>(rg);
    __builtin_amdgcn_sched_barrier(0);
    // An in-order wave that issues its 8 MFMAs back to back waits out the matrix pipe (16 cycles each) before its
    // first VALU instruction; interleaved 1 : 6 the GELU of one quarter runs in the shadow of the other quarter's
    // MFMAs (the two are independent).
    gemm_xb<2, false, 8>(hb, xb, rg);
    gelu_pair<DROP>(ha, dbits, dscale);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, kFfnValuPerMfma, 0);   // 7 VALU
    }
    __builtin_amdgcn_sched_barrier(0);
    gemm_ring<P, kTiles, 2, false, kR8, 16, false>(part, ha, rg);
    gelu_pair<DROP>(hb, dbits >> 8, dscale);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, kFfnValuPerMfma, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    gemm_ring<P, kTiles, 2, false, kR8, 24, false>(part, hb, rg);
}

// ---- train-mode sampling (amuse_hip.h amuse_set_sample_dropout): the uniform part of the mask counters; the per-lane part (global
// clip, the row's token) is re-derived by lane_info where the bits are drawn, and the bits themselves travel in one register
struct SDrop8 {
    uint64_t seed;
    uint32_t step, epoch2, thr;
    float scale;
};
template <bool DROP, class Args>
__device__ __forceinline__ SDrop8 sdrop8_of(const Args& a) {
    SDrop8 d{};
    if constexpr (DROP) {
        d.seed = a.drop_seed; d.epoch2 = 2u + *a.drop_epoch; d.thr = a.drop_thr; d.scale = a.drop_scale;
    }
    return d;
}
// site 0: the probabilities of query q = tok of head h held by this lane - keys k = 4 g + m - cl S, elements (h S + q) S + k =
// base + m, i.e. inside Philox groups base >> 2 and (base >> 2) + 1 (bits m of the result; groups below 0 only ever cover keys
// of other clips, whose probability is 0 anyway)
__device__ __forceinline__ uint32_t sdrop8_attn_bits(const SampleKernelArgs& a, const SDrop8& d, int blk, int h, int lane) {
    const Lane8 L = lane_info(a, lane);
    const int S = a.S, base = (h * S + L.tok) * S + 4 * L.g - L.cl * S, e4 = base >> 2;
    const uint32_t cu = (uint32_t)(a.clip0 + (uint64_t)L.clip), ls = 4u * blk;
    const uint32_t b = sdrop_bits4(d.seed, cu, d.step, ls, (uint32_t)e4 & 0xffffu, d.epoch2, d.thr) |
                       (sdrop_bits4(d.seed, cu, d.step, ls, (uint32_t)(e4 + 1) & 0xffffu, d.epoch2, d.thr) << 4);
    return b >> (base - 4 * e4);
}
// site 2 of FFN quarters Q0, Q0 + 1 of slice h (hidden tiles 8 h + 2 Q0 + k, element tok 512 + f): bits 4 k + m
template <int Q0>
__device__ __forceinline__ uint32_t sdrop8_ffn_bits(const SampleKernelArgs& a, const SDrop8& d, int blk, int h, int lane) {
    const Lane8 L = lane_info(a, lane);
    const uint32_t cu = (uint32_t)(a.clip0 + (uint64_t)L.clip), e4 = (uint32_t)(L.tok * 128 + 4 * (kTiles * h + 2 * Q0) + L.g);
    uint32_t b = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) b |= sdrop_bits4(d.seed, cu, d.step, 4u * blk + 2u, e4 + 4 * k, d.epoch2, d.thr) << (4 * k);
    return b;
}
// sites 1 / 3 (element tok 128 + f) of the reducer's tiles 2 h, 2 h + 1: bits 4 i + m
__device__ __forceinline__ uint32_t sdrop8_row_bits(const SampleKernelArgs& a, const SDrop8& d, uint32_t ls, int h, int lane) {
    const Lane8 L = lane_info(a, lane);
    const uint32_t cu = (uint32_t)(a.clip0 + (uint64_t)L.clip), e4 = (uint32_t)(L.tok * 32 + 8 * h + L.g);
    return sdrop_bits4(d.seed, cu, d.step, ls, e4, d.epoch2, d.thr) | (sdrop_bits4(d.seed, cu, d.step, ls, e4 + 4, d.epoch2, d.thr) << 4);
}

// A noise draw in progress: the Philox counters of a reducer's two tiles, and whether this lane draws at all.  Local to the early fetch of ONE block.
struct Draw8 {
    uint32_t c[2][4];
    bool on;
};
template <int I>
struct Slice {
    static constexpr int value = I;
};
struct NoDraw {
    template <int I>
    __device__ void operator()(Draw8&, Slice<I>) const {}
};
// The reducers' early fetch: units C0 .. kBEarly - 1 of their FFN half into slots C0 .., slice i of `early` behind chunk i.  One body for every block - the
// slices sit behind a uniform branch that touches no ring slot (combine_publish_c2 has the reason).
template <int C0, class Early>
__device__ __forceinline__ void early_fetch(Ring& rg, Draw8& dw, Early& early) {
    if constexpr (C0 < kBEarly) {
        constexpr int N = kBEarly - C0 < kDrawChunk ? kBEarly - C0 : kDrawChunk;
        ring_issue<N, kR8, C0>(rg);
        early(dw, Slice<C0 / kDrawChunk>{});
        early_fetch<C0 + N>(rg, dw, early);
    }
}

// One TransformerEncoderLayer.forward_post (cross_attention.py:259-272), A / B role split.  The two roles are
// separate instantiations (and the whole step loop is instantiated per role, OP_KERNEL below): sharing one body
// behind a runtime branch makes hipcc's register allocator spill hundreds of VGPRs at the merges.
// xb: the residual stream as four packed bf16 operands (every wave); xo: this B wave's two feature tiles in fp32.
// DROP: train-mode sampling - the A waves draw the attention bits in front of in_proj and their FFN bits in the out_proj combine's
// waiting time, the B waves all of theirs (both combines, FFN) while the A waves run attention
template <bool ROLEA, bool PROF, bool DROP, class Early = NoDraw>
__device__ __forceinline__ void encoder_block8(OPV (&xb)[4], f32x4 (&xo)[2], Ring& rg, const float* pv,
                                               const bool (&kvalid)[4], char* lds, int h, int lane, bool next_has_skip,
                                               const uint4* skip_next, Prof8& pf, const SampleKernelArgs& a,
                                               const SDrop8& dr, int blk, Early early = {}) {
    constexpr int P = OP_PREC;
    const int g = lane >> 4, r = lane & 15;
    f32x4 part[kTiles];
    if constexpr (ROLEA) {
        uint32_t abits = 0, fbits = 0;
        if constexpr (DROP) abits = sdrop8_attn_bits(a, dr, blk, h, lane);
        // ---- ring on entry: in_proj q,k (slots 0..15), v (16..23), out_proj (24..31)
        f32x4 b_qk[4];
        float b_v[2];
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            b_qk[o] = ld4(pv + PV_IN_B + 16 * (2 * h + o) + 4 * g);
            b_qk[2 + o] = ld4(pv + PV_IN_B + kD + 16 * (2 * h + o) + 4 * g);
            b_v[o] = pv[PV_IN_B + 2 * kD + 16 * (2 * h + o) + r];
        }
        f32x4 qk[4], v[2];
#pragma unroll
        for (int o = 0; o < 4; ++o) qk[o] = splat4(0.f);
        v[0] = v[1] = splat4(0.f);
        gemm_xb<4, false, 0>(qk, xb, rg);
        gemm_xb<2, true, 16>(v, xb, rg);
        const float scaling = 0.17677669529663687f;  // sqrt(1/32): q * scaling (F.multi_head_attention_forward)
        f32x4 q[2] = {(qk[0] + b_qk[0]) * scaling, (qk[1] + b_qk[1]) * scaling};
        f32x4 k[2] = {qk[2] + b_qk[2], qk[3] + b_qk[3]};
        v[0] += splat4(b_v[0]);
        v[1] += splat4(b_v[1]);
        f32x4 o[2];
        attention_head8<DROP>(q, k, v, kvalid, o, abits, dr.scale);
#pragma unroll
        for (int t = 0; t < kTiles; ++t) part[t] = splat4(0.f);
        gemm_ring<P, kTiles, 2, false, kR8, 24, false>(part, o, rg);
        stamp8<PROF>(pf);  // 1: in_proj + attention + out_proj partial
        // ---- out_proj combine (B reduces): meanwhile fetch this wave's FFN half
        if constexpr (DROP) {
            auto hook = [&]() { fbits = sdrop8_ffn_bits<0>(a, dr, blk, h, lane); };
            combine_publish<0, kC1N1, kC1N2, 32 - kC1N1 - kC1N2 - kALate, 0, true, decltype(hook)>(part, xb, lds, h, lane, rg, hook);
        } else {
            combine_publish<0, kC1N1, kC1N2, 32 - kC1N1 - kC1N2 - kALate, 0>(part, xb, lds, h, lane, rg);
        }
        stamp8<PROF>(pf);  // 2: combine 1
#pragma unroll
        for (int t = 0; t < kTiles; ++t) part[t] = splat4(0.f);
        ffn_half<0, kALate, DROP>(part, xb, rg, pv, h, g, fbits, dr.scale);
        stamp8<PROF>(pf);  // 3: FFN
        // ---- linear2 combine (B reduces): meanwhile fetch the next block's attention weights
        combine_publish_c2<kC2N0, kC2N1, 32 - kC2N0 - kC2N1>(part, xb, lds, h, lane, rg, next_has_skip, skip_next);
    } else {
        // ---- ring empty on entry: fetch this wave's FFN half while the A waves run attention
        // ... with work of the reducers' waiting time that no other wave's result feeds between the loads (role_loop8: the step's ancestral noise)
        Draw8 dw;
        early_fetch<0>(rg, dw, early);
        // bits 0..7: dropout1 of tiles 2 h, 2 h + 1; 8..15: dropout2 of the same; 16..31: the FFN's inner dropout
        uint32_t bbits = 0;
        if constexpr (DROP)
            bbits = sdrop8_row_bits(a, dr, 4u * blk + 1u, h, lane) | (sdrop8_row_bits(a, dr, 4u * blk + 3u, h, lane) << 8) |
                    (sdrop8_ffn_bits<2>(a, dr, blk, h, lane) << 16);
        stamp8<PROF>(pf);
#pragma unroll
        for (int t = 0; t < kTiles; ++t) part[t] = splat4(0.f);
        combine_reduce<4, true, true, DROP>(part, xo, xb, pv + PV_OUT_B, pv + PV_LN1_W, pv + PV_LN1_B, lds, h, lane, bbits, dr.scale);
        stamp8<PROF>(pf);
        ffn_half<2, 32 - kBEarly, DROP>(part, xb, rg, pv, h, g, bbits >> 16, dr.scale);
        stamp8<PROF>(pf);  // 3: FFN
        if (next_has_skip) ring_issue<8, kR8, 0>(rg);  // the x half of this wave's two output tiles of the next block's skip linear
        combine_reduce<8, true, true, DROP>(part, xo, xb, pv + PV_L2_B, pv + PV_LN2_W, pv + PV_LN2_B, lds, h, lane, bbits >> 8, dr.scale);
    }
    stamp8<PROF>(pf);  // 4: combine 2
}

// The whole T-step loop of one role.  Both roles execute the same sequence of workgroup barriers.
template <bool ROLEA, bool PROF, bool DROP, class Args>
__device__ __forceinline__ void role_loop8(const Args& a, char* smem, int w8, const Lane8& L0) {
    uint4* skipbf = reinterpret_cast<uint4*>(smem + kSkip8Off);
    const float* pvl = reinterpret_cast<const float*>(smem + kPv8Off);
    const f32x4* tokrows = reinterpret_cast<const f32x4*>(smem + kTokRows8Off);
    f32x4* latl = reinterpret_cast<f32x4*>(smem + kLat8Off);
    float* ttl = reinterpret_cast<float*>(smem + kTT8Off);
    float2* stats = reinterpret_cast<float2*>(smem + kStat8Off);
    const float* cfl = reinterpret_cast<const float*>(smem + kCoef8Off);   // this step's scheduler coefficients (step top)
    const float* pv_skip = pvl + kLayers * kEncPv;
    const float* pv_final = pv_skip + 4 * kD;
    const int lane = L0.lane, g = L0.g, r = L0.r, h = w8 & 3;
    const int S = a.S, R = S * a.G;
    bool kvalid[4];   // attention key mask of this lane's query row
#pragma unroll
    for (int m = 0; m < 4; ++m) kvalid[m] = key_valid8(L0, 4 * g + m, S, R);
    const bool tap = !ROLEA && a.tap_out != nullptr && blockIdx.x == 0;  // the B waves tap their own fp32 tiles
    const uint32_t wbase_units = ROLEA ? (uint32_t)w8 * (a.wave_units_a + kR8)
                                       : 4u * (a.wave_units_a + kR8) + (uint32_t)(w8 - 4) * a.wave_units_b;
    const uint4* wbase = a.wstream + (size_t)wbase_units * 64 + lane;
    // A waves enter every block with their 32 units in the ring (the stream's tail repeats its head for the wrap
    // at a step boundary); B waves enter with an empty ring (their fill is never consumed)
    Ring rg;
    if constexpr (ROLEA) {   // unit i of a block's group of 32 lives in slot (24 + i) % 32 (combine_publish_c2)
#pragma unroll
        for (int i = 0; i < kR8; ++i) rg.s[(24 + i) % kR8] = ldw(wbase + i * 64);
        rg.next = wbase + kR8 * 64;
    } else {
        ring_fill(rg, wbase);
    }
    Prof8 pf{a.prof_out ? a.prof_out + (size_t)w8 * 96 : nullptr, 0, false};
    SDrop8 dr = sdrop8_of<DROP>(a);
    // the first step's input (amuse_sample8.hpp assemble_own): each reducer's two tiles from the initial latent, published where the step head gathers
    f32x4 xo[2] = {splat4(0.f), splat4(0.f)};
    if constexpr (!ROLEA) {
        const Lane8 L = lane_info(a, lane);
        const f32x4 l[2] = {latl[(2 * h) * 64 + L.lane], latl[(2 * h + 1) * 64 + L.lane]};
        assemble_own(xo, l, a, L, tokrows, ttl, 0, h);
        *xb_slot(smem, h, L.lane) = __builtin_bit_cast(uint4, OP_PACK(xo[0], xo[1]));
    }
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < a.T; ++step) {
        if constexpr (PROF) {
            stamp8<PROF>(pf);  // (on only in the step behind the profiled one: its top closes that step, stamp to stamp)
            pf.on = a.prof_out != nullptr && blockIdx.x == 0 && lane == 0 && step == a.prof_step;
            stamp8<PROF>(pf);  // step top: the head (token assembly, wave 4's time-token copy) starts
        }
        dr.step = (uint32_t)step;
        // ---- token assembly (denoiser.py:174,180-181): done by the reducers in the previous step's tail (in front of the loop for the first step),
        // published like a combine's result - the head is that combine's gather; a B wave carries its own two tiles in fp32 (xo)
        OPV xb[4];
        f32x4 zn[2] = {splat4(0.f), splat4(0.f)};   // B waves: this step's ancestral noise of their two tiles, drawn ahead of the tail (below)
#pragma unroll
        for (int c = 0; c < 4; ++c) xb[c] = __builtin_bit_cast(OPV, *xb_slot(smem, c, lane));
        // next step's time token -> the other LDS buffer (the reducers read it in this step's tail, many barriers later); in the same load and store, by lanes
        // 32 and 33, THIS step's eight scheduler coefficients -> LDS: the reducers read them in the last block (is there noise to draw?) and in the tail, where
        // an LDS read neither waits for the weight stream's loads (vmcnt retires in order) nor costs a trip to memory on the reducers' lone stretch
        if (!ROLEA && w8 == 4) {
            const bool tt = lane < 32;
            const float* src = tt ? a.time_tok + (size_t)(step + 1) * kD + 4 * lane : a.coef + (size_t)step * 8 + 4 * (lane & 1);
            float* dst = reinterpret_cast<float*>(smem + (tt ? kTT8Off + (((step + 1) & 1) * kD + 4 * lane) * 4 : kCoef8Off + 16 * (lane & 1)));
            if (tt ? step + 1 < a.T : lane < 34) st4(dst, ld4(src));
        }
        if (tap && step == 0) {
            store_tap_tile(a.tap_out, 0, 2 * h, xo[0], g, r);
            store_tap_tile(a.tap_out, 0, 2 * h + 1, xo[1], g, r);
        }
        stamp8<PROF>(pf);  // step start: operands gathered, wave 4's time-token copy done
        rg.next = ROLEA ? wbase + kR8 * 64 : wbase;  // (A: the ring already holds units 0..31 of this step)
        // ---- SkipTransformerEncoder.forward (cross_attention.py:41-64)
#pragma unroll 1
        for (int blk = 0; blk < kLayers; ++blk) {
            if (blk >= 5) {
                // x = Linear(cat(x, skips.pop())) (cross_attention.py:58-61), split over OUTPUT tiles: B wave h computes
                // its own feature tiles 2h, 2h+1 = bias + u + W[:, :128] . x, where u = W[:, 128:] . skip was prepared by
                // A wave h during the previous linear2 combine (combine_publish_skipu).  It keeps them as its fp32 tiles
                // and publishes the packed operand: one barrier and no partial sums (the split-K version of this
                // 256 -> 128 linear cost 1.8 k cycles, mostly the 8-way reduction).  The A waves fetch out_proj.
                // Published in row 7 of the combine matrix: not the diagonal, which lagging waves may still be
                // gathering from the linear2 combine, and not a row the next out_proj combine's partials use.
                if constexpr (ROLEA) {
                    ring_issue<8, kR8, 24>(rg);
                } else {
                    const float* bs = pv_skip + (blk - 5) * kD + 32 * h + 4 * g;
                    f32x4 acc[2] = {ld4(bs) + *u_slot(smem, 2 * h, lane), ld4(bs + 16) + *u_slot(smem, 2 * h + 1, lane)};
                    gemm_xb<2, false, 0>(acc, xb, rg);
                    xo[0] = acc[0];
                    xo[1] = acc[1];
                    *reinterpret_cast<uint4*>(a8_slot(smem, 7, h, lane)) = __builtin_bit_cast(uint4, OP_PACK(acc[0], acc[1]));
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 4; ++c) xb[c] = __builtin_bit_cast(OPV, *reinterpret_cast<const uint4*>(a8_slot(smem, 7, c, lane)));
            }
            stamp8<PROF>(pf);  // 0: block start (after the skip linear, if any)
            // The noise of the scheduler update depends on (seed, clip, step, feature) alone, not on the network: Philox4x32-10 (80 integer multiplies in two
            // serial chains) and Box-Muller for two tiles, which the tail used to walk with the whole workgroup waiting.  The reducers draw it in the LAST
            // block instead, INSIDE their early fetch (slice I behind its chunk I: kDrawChunk), while they wait for the A waves' attention anyway; eight
            // registers carry it to the tail.  counter_normal4's arithmetic, the two tiles' rounds side by side; sigma comes from LDS (step top), so no wait
            // here covers the ring's loads.  Every lane computes - a lane mask would cost a branch per slice - and the lanes that do not draw keep their 0.
            auto early = [&](Draw8& dw, auto slice) {
                if constexpr (!ROLEA && !DROP) {   // (the train-mode instantiations have no register to spare: they draw in the tail)
                    constexpr int I = decltype(slice)::value;
                    if (blk == kLayers - 1 && !a.no_update && !a.step_noise) {
                        if constexpr (I == 0) {
                            const Lane8 L = lane_info(a, lane);
                            dw.on = L.is_lat && cfl[5] != 0.f;
#pragma unroll
                            for (int i = 0; i < 2; ++i) {
                                dw.c[i][0] = (uint32_t)(a.clip0 + (uint64_t)L.clip); dw.c[i][1] = (uint32_t)step;
                                dw.c[i][2] = (uint32_t)(4 * (2 * h + i) + L.g); dw.c[i][3] = 1u;
                            }
                        }
#pragma unroll
                        for (int rd = I * kDrawRounds; rd < (I + 1) * kDrawRounds && rd < 10 && I < kDrawSlices - 1; ++rd) {
                            philox4x32_round(dw.c[0], (uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)rd);
                            philox4x32_round(dw.c[1], (uint32_t)a.seed, (uint32_t)(a.seed >> 32), (uint32_t)rd);
                        }
                        if constexpr (I == kDrawSlices - 1) {
                            const f32x4 z0 = philox_normal4(dw.c[0]), z1 = philox_normal4(dw.c[1]);
                            zn[0] = dw.on ? z0 : zn[0];
                            zn[1] = dw.on ? z1 : zn[1];
                        }
                    }
                }
            };
            encoder_block8<ROLEA, PROF, DROP, decltype(early)>(xb, xo, rg, pvl + blk * kEncPv, kvalid, smem, h, lane, blk >= 4 && blk < kLayers - 1,
                                                               skipbf + (7 - blk) * 4 * 64, pf, a, dr, blk, early);
            if (!ROLEA && blk < 4 && w8 == 4) {
#pragma unroll
                for (int p = 0; p < 4; ++p) skipbf[(blk * 4 + p) * 64 + lane] = __builtin_bit_cast(uint4, xb[p]);
            }
            if (tap && step == 0) {
                store_tap_tile(a.tap_out, 1 + blk, 2 * h, xo[0], g, r);
                store_tap_tile(a.tap_out, 1 + blk, 2 * h + 1, xo[1], g, r);
            }
        }
        // ---- final LayerNorm (SkipTransformerEncoder.norm) + scheduler.step (diffusers 0.17.1 DDIM / DDPM;
        // amuse_hip.h amuse_schedule) on the B waves' own tiles; the latent lives in LDS
        // The reducers walk this tail alone on their SIMD (the A waves are parked at the step barrier), so every latency in it is
        // step time.  The step's coefficients (in LDS since the step top) are read BEFORE the barrier; behind it the final LayerNorm's
        // parameters and this wave's two latent tiles are read up front, beside the statistics, and the two tiles go through each stage
        // side by side (eight independent update chains) instead of tile after tile.  Same operations on the same operands.
        if constexpr (!ROLEA) {
            const float* cf = cfl;
            const float sb = cf[0], sa = cf[1], c0 = cf[2], cx = cf[3], ce = cf[4], sg = cf[5], clipv = cf[6];
            const float2 st = row_stats32(xo);
            if (g == 0) stats[h * 16 + r] = st;
            __syncthreads();
            const Lane8 L = lane_info(a, lane);
            f32x4 ga[2], be[2], l[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ga[i] = ld4(pv_final + 16 * (2 * h + i) + 4 * L.g);
                be[i] = ld4(pv_final + kD + 16 * (2 * h + i) + 4 * L.g);
                l[i] = latl[(2 * h + i) * 64 + L.lane];
            }
            const float2 ms = row_stats_merge<true>(stats, L.r);
            const float inv_sa = 1.0f / sa;
            f32x4 e[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int m = 0; m < 4; ++m) e[i][m] = (xo[i][m] - ms.x) * ms.y * ga[i][m] + be[i][m];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int t = 2 * h + i, f = 16 * t + 4 * L.g;
                if (tap && step == 0) store_tap_tile(a.tap_out, 10, t, e[i], L.g, L.r);
                if (a.eps_out && L.is_lat && step == a.T - 1) st4(a.eps_out + (size_t)L.clip * kD + f, e[i]);
            }
            if (!a.no_update) {
                // ancestral noise of the latent rows: counter (global clip, step, feature group) - the values amuse_counter_normal exposes
                f32x4 z[2] = {zn[0], zn[1]};   // drawn in the last block (above) unless the caller supplies the noise
                if (sg != 0.f && L.is_lat && (DROP || a.step_noise)) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int t = 2 * h + i, f = 16 * t + 4 * L.g;
                        z[i] = a.step_noise ? ld4(a.step_noise + ((size_t)step * a.B + L.clip) * kD + f)
                                            : counter_normal4(a.seed, a.clip0 + (uint64_t)L.clip, (uint32_t)step, (uint32_t)(4 * t + L.g), 1u);
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int m = 0; m < 4; ++m) l[i][m] = sched_update<true>(l[i][m], e[i][m], z[i][m], sb, sa, c0, cx, ce, sg, clipv, inv_sa);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int t = 2 * h + i, f = 16 * t + 4 * L.g;
                    latl[t * 64 + L.lane] = l[i];
                    if (a.traj_out && L.is_lat) st4(a.traj_out + ((size_t)step * a.B + L.clip) * kD + f, l[i]);
                }
            }
            // the next step's input from the updated latent, published for every wave's gather behind the step barrier (assemble_own)
            if (step + 1 < a.T) {
                assemble_own(xo, l, a, L, tokrows, ttl, step + 1, h);
                *xb_slot(smem, h, L.lane) = __builtin_bit_cast(uint4, OP_PACK(xo[0], xo[1]));
            }
        } else {
            __syncthreads();
        }
        stamp8<PROF>(pf);  // scheduler update done (B waves) / reached the step barrier
        __syncthreads();  // the next step's operands are visible to every wave's gather
    }
}

// DROP = true (train-mode sampling, a.drop_thr > 0) takes the whole SampleArgs, the eval instantiations the SampleKernelArgs slice
template <bool PROF, bool DROP, class Args>
__global__ __launch_bounds__(512) void OP_KERNEL(Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* pvl = reinterpret_cast<float*>(smem + kPv8Off);
    f32x4* tokrows = reinterpret_cast<f32x4*>(smem + kTokRows8Off);
    f32x4* latl = reinterpret_cast<f32x4*>(smem + kLat8Off);
    float* ttl = reinterpret_cast<float*>(smem + kTT8Off);
    for (int i = threadIdx.x; i < kLayers * kEncPv / 4; i += 512) {
        const int blk = (4 * i) / kEncPv, off = 4 * i - blk * kEncPv;
        st4(pvl + 4 * i, ld4(a.pvec + blk * PV_BLOCK + off));
    }
    for (int i = threadIdx.x; i < (4 * kD + 2 * kD) / 4; i += 512) st4(pvl + kLayers * kEncPv + 4 * i, ld4(a.pvec + PV_SKIP_B + 4 * i));
    const int w8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Lane8 L = lane_info(a, threadIdx.x & 63);
    // static token rows and the initial latent -> LDS (wave 0 owns the latent's update); the first step's time token
    if (w8 == 0) {
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            const int f = 16 * t + 4 * L.g;
            const f32x4 sv = static_row4(a, L, f), l0 = init_latent4(a, L, t, f);
            tokrows[t * 64 + L.lane] = sv;
            latl[t * 64 + L.lane] = l0;
        }
    }
    if (w8 == 4 && L.lane < 32 && !a.time_tok_clip) st4(ttl + 4 * L.lane, ld4(a.time_tok + 4 * L.lane));
    __syncthreads();
    if (w8 < 4) role_loop8<true, PROF, DROP>(a, smem, w8, L);
    else role_loop8<false, PROF, DROP>(a, smem, w8, L);
    if (L.is_lat && w8 == 0 && a.latents_out) {
#pragma unroll
        for (int t = 0; t < kTiles; ++t) st4(a.latents_out + (size_t)L.clip * kD + 16 * t + 4 * L.g, latl[t * 64 + L.lane]);
    }
}

}  // namespace

hipError_t OP_LAUNCH(const SampleArgs& a_in, hipStream_t stream) {
    SampleArgs a = a_in;
    if (a.drop_thr > 0 && !(a.drop_epoch = train_epoch_ptr())) return hipErrorOutOfMemory;
    const int tiles = (a.B + a.G - 1) / a.G;
    static DeviceOnce once;
    int dev_;
    if (!once.done(&dev_)) {
        for (const void* k : {reinterpret_cast<const void*>(&OP_KERNEL<false, false, SampleKernelArgs>), reinterpret_cast<const void*>(&OP_KERNEL<true, false, SampleKernelArgs>),
                              reinterpret_cast<const void*>(&OP_KERNEL<false, true, SampleArgs>), reinterpret_cast<const void*>(&OP_KERNEL<true, true, SampleArgs>)}) {
            hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kSample8LdsBytes);
            if (e != hipSuccess) return e;
        }
        once.set(dev_);
    }
    const SampleKernelArgs ka = a;
    if (a.drop_thr > 0) {
        if (a.prof_out) hipLaunchKernelGGL((OP_KERNEL<true, true, SampleArgs>), dim3(tiles), dim3(512), kSample8LdsBytes, stream, a);
        else hipLaunchKernelGGL((OP_KERNEL<false, true, SampleArgs>), dim3(tiles), dim3(512), kSample8LdsBytes, stream, a);
    } else if (a.prof_out) hipLaunchKernelGGL((OP_KERNEL<true, false, SampleKernelArgs>), dim3(tiles), dim3(512), kSample8LdsBytes, stream, ka);
    else hipLaunchKernelGGL((OP_KERNEL<false, false, SampleKernelArgs>), dim3(tiles), dim3(512), kSample8LdsBytes, stream, ka);
    return hipGetLastError();
}

}  // namespace amuse
