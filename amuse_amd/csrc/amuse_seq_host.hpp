// What the host code of every extension shares: the error slot of the C ABI, the sizes of a motion row, and the ONE statement of how a call's sequences travel
// to a kernel.  Per-sequence offsets go BY VALUE in the kernel arguments - no device table, no copy, no allocation, so the call can sit inside a captured
// graph - kSeqPerLaunch sequences per launch, further sequences in further launches.  Context-free: nothing here reads or keeps state.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/amuse_hip.h"

// error slot of the C ABI (thread-local text behind amuse_last_error; defined in amuse_api.hip, tests/host_check.hpp: a stand-in that keeps the text)
__attribute__((visibility("hidden"), format(printf, 2, 3))) int amuse_failf(int code, const char* fmt, ...);

namespace amuse {

constexpr int kSmplxJoints = 55;      // SMPL-X joints of a pose row: 165 contiguous floats
constexpr int kMotionSlots = 56;      // lanes per frame: one per joint, one for the translation
constexpr int kSeqPerLaunch = 32;     // 32 x 16 B of offsets beside a few pointers and a 56-byte table stay far inside the 4 KiB of kernel arguments

// do the byte ranges [a, a + a_floats) and [b, b + b_floats) share a byte?
inline bool ranges_overlap(const float* a, long long a_floats, const float* b, long long b_floats) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + (uintptr_t)b_floats * sizeof(float) && pb < pa + (uintptr_t)a_floats * sizeof(float);
}

// S sequences in launches of up to kSeqPerLaunch.  proto: the call's common fields, everything else zero - every launch starts from a copy of it, so the seq[]
// slots a launch does not use are zero.  fill(a, k, s) writes a.seq[k] for the call's sequence s, advances the caller's running offsets and keeps the launch's
// maximum.  entry: the C entry point's name, for the error text.
template <class Args, class Fill>
inline int launch_sequences(const char* entry, int S, const Args& proto, Fill fill, hipError_t (*launch)(const Args&, hipStream_t), hipStream_t stream) {
    for (int s0 = 0; s0 < S; s0 += kSeqPerLaunch) {
        Args a = proto;
        a.nseq = S - s0 < kSeqPerLaunch ? S - s0 : kSeqPerLaunch;
        for (int k = 0; k < a.nseq; ++k) fill(a, k, s0 + k);
        const hipError_t e = launch(a, stream);
        if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "%s: launch failed: %s", entry, hipGetErrorString(e));
    }
    return AMUSE_OK;
}

}  // namespace amuse
