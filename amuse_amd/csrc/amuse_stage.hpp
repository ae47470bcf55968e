// The LDS-DMA weight-stage ring of the kernels that share a weight stream across a workgroup (amuse_fused.hpp: k_vae_fused / k_den_fused and
// their fp16 builds; k_vae_fusedx.hip; k_vae_rows8.hip).  The stream is in consumption order, cut into stages of kStage units (16 KiB); the
// copying waves move each stage global -> LDS with glds16 (amuse_dev.hpp) into a ring of kWBufs buffers, kWBufs - 1 stages ahead of the stage
// being read; a stage ends with "all of my DMA but the fetch issued in this stage has landed" + s_barrier.  Device code only.
#pragma once
#include "amuse_dev.hpp"
#include "amuse_kernels.hpp"

namespace amuse {
namespace {

constexpr int kStage = kVaeFusedStageUnits;   // units per LDS stage: 16 KiB (fp32x streams: 8 hi | lo pairs)
constexpr int kStageBytes = kStage * 1024;
// LDS stages in the ring: the copy keeps kWBufs - 1 stages ahead of the stage being read, kWBufs - 2 of them may still be in flight at a stage's
// end (deeper rings measured flat in k_vae_rows8x: profiles/r04_rows8x_ring_depth_ab.txt)
constexpr int kWBufs = 3;

// P = pieces (1 KiB units) a copying wave moves per stage: 2 (eight waves copy: the fused kernels), 4 (four waves), 16 (one wave copies
// everything), 0 (a wave that reads beside a dedicated copying wave: no vmcnt at a stage's end)
// Who: every wave of the workgroup copies (EveryWave), or the waves whose wave-uniform `dma` flag is set (SomeWaves).  (A flag that is always true is not free: as a
// field of the fused kernels' ring it reorders their LDS-DMA address arithmetic.)
struct EveryWave { static constexpr bool dma = true; };
struct SomeWaves { bool dma; };
template <int P, class Who = EveryWave>
struct StageRing : Who {
    const uint4* src;   // this lane's source address of the wave's pieces of the NEXT stage to fetch
    unsigned dst0;      // LDS byte address of the wave's pieces inside buffer 0
    const char* ring;   // weight ring base (generic pointer) + lane * 16
    int widx, ridx;     // buffer the next fetch fills / buffer the current stage reads
};
// (A wave-uniform source base in SGPRs + a 32-bit lane offset - the saddr form of global_load_lds_dwordx4 - and 32-bit LDS addresses for
// the ring were tried in round 4 to free the four registers these pointers hold: hipcc's allocation got WORSE, 28 -> 46 spilled registers.)
template <int P, class Who>
__device__ __forceinline__ void stage_fetch(StageRing<P, Who>& s) {
    if constexpr (P == 0) return;
    if (s.dma) {   // (the other waves' vmcnt(P) at the stage's end is trivially true - the barrier is what they need)
        const unsigned d = __builtin_amdgcn_readfirstlane(s.dst0 + s.widx * kStageBytes);
#pragma unroll
        for (int i = 0; i < P; ++i) glds16(s.src + i * 64, d + i * 1024);
    }
    s.src += kStage * 64;
    s.widx = s.widx == kWBufs - 1 ? 0 : s.widx + 1;
}
// end of a stage: all of this wave's DMA except the P pieces of the fetch issued in this stage has landed, its LDS reads
// and writes are done; after the barrier that holds for every wave - the next stage's buffer is complete, this stage's is free
template <int P, class Who>
__device__ __forceinline__ void stage_end(StageRing<P, Who>& s) {
    if constexpr (P == 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else if constexpr (P == 16) asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(P) : "memory");
    s.ridx = s.ridx == kWBufs - 1 ? 0 : s.ridx + 1;
}
// unit u of the current stage as an MFMA operand of type V
template <class V, int P, class Who>
__device__ __forceinline__ V wfrag(const StageRing<P, Who>& s, int u) {
    return __builtin_bit_cast(V, *reinterpret_cast<const uint4*>(s.ring + s.ridx * kStageBytes + u * 1024));
}
// the 8 unit pairs (hi | lo fp16 fragments) of the current stage, pair i -> f(i, hi, lo); the fragments of pair i + 1 are read before
// pair i's MFMAs.  FETCH: issue the next fetch first; END: stage_end behind the last pair.
template <bool FETCH = true, bool END = true, int P, class Who, class F>
__device__ __forceinline__ void for_pairs(StageRing<P, Who>& s, F&& f) {
    if constexpr (FETCH) stage_fetch(s);
    f16x8 h = wfrag<f16x8>(s, 0), l = wfrag<f16x8>(s, 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f16x8 ch = h, cl = l;
        if (i + 1 < 8) { h = wfrag<f16x8>(s, 2 * i + 2); l = wfrag<f16x8>(s, 2 * i + 3); }
        f(i, ch, cl);
    }
    if constexpr (END) stage_end(s);
}

}  // namespace
}  // namespace amuse
