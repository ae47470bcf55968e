// What the 8-wave sampling kernels share (k_sampler8.hip - bf16, and fp16 through k_sampler8h.hip - and k_sampler8x.hip, fp32x): the combine
// matrix A8 and its slot rules, the per-lane constants, the phase stamps, and the value-returning pieces of what differs between the kernels
// only in the operand type they publish - key mask, row statistics, token assembly, the prologue's rows, the step's noise.  The role loops, the
// combines' publish sides and the FFN halves differ in ring depth, re-arming and parameter streaming and stay in the kernels' files.
// Device code only; k_sampler8.hip has the design notes.
#pragma once
#include "amuse_dev.hpp"
#include "amuse_kernels.hpp"

namespace amuse {
namespace {

constexpr int kR8 = kRing8;
using Ring = WRing<kR8>;
// LDS starts with the combine matrix A8 [8 rows][8 tiles][64] f32x4 and the row statistics; the rest of the map is each kernel's own
constexpr int kA8Bytes = 8 * kTiles * 64 * 16;                 // 65,536
constexpr int kStat8Off = kA8Bytes;                            // [4 reducers][16 rows] float2 (1 KiB reserved)

__device__ __forceinline__ f32x4* a8_slot(char* lds, int row, int col, int lane) {
    return reinterpret_cast<f32x4*>(lds) + (row * kTiles + col) * 64 + lane;
}
// Row of A8 holding writer w's partial of tile t in a split-K combine - never the diagonal (where the published operands go), and the
// tile's reducer (wave 4 + t/2) keeps its own partial in registers:
__device__ __forceinline__ constexpr int part_row(int w, int t) {
    const int red = 4 + (t >> 1);
    const int k = w - (w > red ? 1 : 0);
    return k + (k >= t ? 1 : 0);
}
// Slot of the combine matrix through which A wave h hands the skip-input half of the next output block's skip linear
// (feature tile t = 2h + i) to B wave h: off the diagonal, written after the reducers have read their partials.
__device__ __forceinline__ f32x4* u_slot(char* lds, int t, int lane) { return a8_slot(lds, t == 6 ? 5 : 6, t, lane); }

// optional phase timeline: s_memtime stamps by lane 0 of every wave of workgroup 0 during ONE step ([8][96] u64)
struct Prof8 {
    unsigned long long* out;
    int idx;
    bool on;
};
template <bool PROF>
__device__ __forceinline__ void stamp8(Prof8& pf) {
    if constexpr (PROF) {
        if (pf.on) pf.out[pf.idx++] = __builtin_readcyclecounter();
    }
}

// per-lane constants of the tile (row-lane layout: lane (g, r) holds row r)
struct Lane8 {
    int lane, g, r, cl, tok;
    long clip;
    bool valid, is_lat;
};
// Cheap to derive, expensive to keep: held across the block loop these constants get spilled to scratch (the ring
// leaves no slack), so the step loop re-derives them where it needs them from an opaque copy of the lane id.
__device__ __forceinline__ Lane8 lane_info(const SampleKernelArgs& a, int lane) {
    asm volatile("" : "+v"(lane));
    Lane8 L;
    L.lane = lane;
    L.g = lane >> 4;
    L.r = lane & 15;
    const int S = a.S, R = S * a.G;
    L.cl = L.r / S;
    L.tok = L.r - L.cl * S;
    L.clip = (long)blockIdx.x * a.G + L.cl;
    L.valid = (L.r < R) && (L.clip < (long)a.B);
    L.is_lat = L.valid && L.tok == 0;
    return L;
}

// debugging taps: one feature tile of the [16 x 128] residual stream
__device__ __forceinline__ void store_tap_tile(float* tap, int slot, int t, const f32x4& v, int g, int r) {
    st4(tap + ((size_t)slot * 16 + r) * kD + 16 * t + 4 * g, v);
}

// attention key mask for this lane's query row: key j (= 4 g + m) of the SAME clip; padding rows attend to
// themselves only (keeps them finite, they never touch valid rows)
__device__ __forceinline__ bool key_valid8(const Lane8& L0, int j, int S, int R) {
    return L0.valid ? (j < R && (j / S) == L0.cl) : (j == L0.r);
}

// LayerNorm statistics of a row whose 128 features are spread over four waves (32 each: tiles y[0], y[1]; lanes g = 0..3 of a row hold 8
// of them each).  row_stats32: {mean, M2} of this wave's slice, which its lanes g == 0 publish to stats[wave][row]; behind a barrier
// row_stats_merge combines the four slices in one fixed order with Chan's parallel-variance formula -> {mean, rstd} (eps 1e-5, biased
// variance; FAST: v_rsq_f32).  Both combines' reducers and the final LayerNorm use them.
// (These helpers and the ones below return values and leave every store to the kernel: written as functions that store - or that fill an
// array passed by reference - they change the kernels' register allocation.  combine_rs of the 4-wave kernels, amuse_dev.hpp, holds the
// same arithmetic inline for that reason.)
__device__ __forceinline__ float2 row_stats32(const f32x4 (&y)[2]) {
    float s = ((y[0][0] + y[0][1]) + (y[0][2] + y[0][3])) + ((y[1][0] + y[1][1]) + (y[1][2] + y[1][3]));
    s = allreduce_g_sum(s);
    const float mw = s * (1.0f / 32.0f);
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float d = y[i][m] - mw;
            m2 += d * d;
        }
    m2 = allreduce_g_sum(m2);
    return float2{mw, m2};
}
template <bool FAST>
__device__ __forceinline__ float2 row_stats_merge(const float2* stats, int r) {
    const float2 s0 = stats[r], s1 = stats[16 + r], s2 = stats[32 + r], s3 = stats[48 + r];
    const float mean = ((s0.x + s1.x) + (s2.x + s3.x)) * 0.25f;
    const float d0 = s0.x - mean, d1 = s1.x - mean, d2 = s2.x - mean, d3 = s3.x - mean;
    const float M2 = ((s0.y + s1.y) + (s2.y + s3.y)) + 32.0f * ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3));
    const float var = M2 * (1.0f / kD) + 1e-5f;
    return float2{mean, FAST ? __builtin_amdgcn_rsqf(var) : 1.0f / sqrtf(var)};
}

// The prologue's rows (denoiser.py:174,180-181), features f .. f + 3 of this lane's row: the static token row (pe[0] under the latent
// rows, condition tokens) and the initial latent of feature tile t.  They go to LDS: registers are the scarce resource at 2 waves / SIMD.
// A per-clip time token (time_tok_clip: a teacher-forced step, diffusion_forward) does not change from step to step either and is a static
// row of its clip; the per-step one (time_tok) travels through the double buffer instead and its row here stays 0 (token assembly, below).
template <class Args>
__device__ __forceinline__ f32x4 static_row4(const Args& a, const Lane8& L, int f) {
    f32x4 sv = splat4(0.f);
    if (L.valid) {
        if (L.tok == 0) sv = ld4(a.pe0 + f);
        else if (L.tok >= 2) sv = ld4(a.cond_tok + ((size_t)L.clip * (a.S - 2) + (L.tok - 2)) * kD + f);
        else if (a.time_tok_clip) sv = ld4(a.time_tok_clip + (size_t)L.clip * kD + f);
    }
    return sv;
}
template <class Args>
__device__ __forceinline__ f32x4 init_latent4(const Args& a, const Lane8& L, int t, int f) {
    f32x4 l0 = splat4(0.f);
    if (L.is_lat)
        l0 = a.x_init ? ld4(a.x_init + (size_t)L.clip * kD + f)
                      : counter_normal4(a.seed, a.clip0 + (uint64_t)L.clip, 0u, (uint32_t)(4 * t + L.g), 0u);
    return l0;
}
// Token assembly (denoiser.py:174,180-181): feature tile t of this lane's row of the step's input is
//   !valid ? 0 : tok == 0 ? latent + static row : tok == 1 ? time token : static row.
// Every operand lives in LDS and a lane's token never changes, so the lane fixes ONE source of its non-latent operand per step - the time-token
// buffer of this step for a time-token row, its static row otherwise (which holds 0 for padding rows and, under a per-clip time token, that
// token: static_row4) - and a tile costs one unconditional ds_read_b128 beside the latent, an add and a select.  No global or flat load, no
// lane-mask branch.
struct TokSrc {
    const f32x4* x;   // the lane's non-latent operand of tile 0 ...
    int stride;       // ... and the distance to the next tile's
    bool is_lat;
};
template <class Args>
__device__ __forceinline__ TokSrc tok_src(const Args& a, const Lane8& L, int lane, int g, const f32x4* tokrows, const float* ttl, int step) {
    const bool from_tt = L.valid && L.tok == 1 && !a.time_tok_clip;
    return TokSrc{from_tt ? reinterpret_cast<const f32x4*>(ttl + (step & 1) * kD) + g : tokrows + lane, from_tt ? 4 : 64, L.is_lat};
}
__device__ __forceinline__ f32x4 assemble_pick(const TokSrc& s, const f32x4& x, const f32x4& la) {
    const f32x4 sum = la + x;
    return s.is_lat ? sum : x;
}
// Who assembles.  k_sample8x: every wave, at the step's head, all tiles at once - the reads of tiles T0 .. T0 + N - 1 (T0 may be a runtime value:
// a reducer's own pair) issued before one wait (assemble_load), then the picks; lane: the step loop's own copy.
template <int N>
__device__ __forceinline__ void assemble_load(f32x4 (&x)[N], f32x4 (&la)[N], const TokSrc& s, const f32x4* latl, int lane, int T0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[i] = s.x[(T0 + i) * s.stride];
        la[i] = latl[(T0 + i) * 64 + lane];
    }
}
// k_sample8 / k_sample8h: the reducer of a tile pair (B wave h: tiles 2 h, 2 h + 1), which holds the updated latent of exactly those tiles in
// registers at the end of a step's tail.  It builds the NEXT step's two tiles there (and, in front of the first step, from the initial latent),
// keeps them as its fp32 tiles and publishes them as one operand where a combine's result goes; every wave's step head is then a combine's
// gather - four reads - instead of sixteen to twenty (8 waves x 16-20 KiB of LDS reads bound the head above at ~1.2 k cycles of LDS bandwidth).
// -> the two tiles of step `step`'s input from latent tiles la; L: lane_info's opaque re-derivation
template <class Args>
__device__ __forceinline__ void assemble_own(f32x4 (&xo)[2], const f32x4 (&la)[2], const Args& a, const Lane8& L, const f32x4* tokrows, const float* ttl,
                                             int step, int h) {
    const TokSrc s = tok_src(a, L, L.lane, L.g, tokrows, ttl, step);
    const f32x4 x0 = s.x[(2 * h) * s.stride], x1 = s.x[(2 * h + 1) * s.stride];
    xo[0] = assemble_pick(s, x0, la[0]);
    xo[1] = assemble_pick(s, x1, la[1]);
}

}  // namespace
}  // namespace amuse
