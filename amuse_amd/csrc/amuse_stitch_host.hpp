// Long-form inference (include/amuse_hip.h amuse_longform_plan / amuse_stitch_windows): everything the join needs on the host, shared by k_stitch.hip (the
// kernel and its launcher), amuse_stitch.hip (the two C entry points) and tests/stitch_host (the same host code on a stand-in launcher, under sanitizers):
//   - the window plan: the ONE statement of how a waveform of n samples is cut into overlapping clips;
//   - the argument checks of the join, made before any HIP call;
//   - the call's sequences, packed into launches by amuse_seq_host.hpp.
// Context-free: nothing here reads or keeps state.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kStitchBlock = 256;

constexpr int kClipFrames = 300;          // the model's clip (dm/dm.py:91)
constexpr int kClipSamples = 160000;      // 10 s at 16 kHz = 300 frames at 30 fps
constexpr int kSamplesPerFrame3 = 1600;   // 3 frames = 1600 samples: 16000 / 30 is no whole number

struct StitchSeq {
    int win0;     // first window of the sequence (index into poses / trans, in windows)
    int out0;     // first output frame of the sequence (index into poses_out / trans_out, in frames)
    int W, L;     // windows, output frames
};

struct StitchArgs {
    const float* poses;    // [windows][F][55][3]
    const float* trans;    // [windows][F][3] or null
    const float* blend;    // [F - hop]
    float* poses_out;      // [frames][55][3]
    float* trans_out;      // [frames][3] or null
    int F, hop, nseq, max_L;
    StitchSeq seq[kSeqPerLaunch];
};

// k_stitch.hip (tests/stitch_host: a stand-in that records the arguments)
hipError_t launch_stitch(const StitchArgs& a, hipStream_t stream);

// ---- the window plan
inline int longform_plan(long long n_samples, int hop_frames, int* windows, int* frames, int* hop_samples) {
    if (n_samples < 0) return amuse_failf(AMUSE_EINVAL, "amuse_longform_plan: n_samples %lld is negative", n_samples);
    if (hop_frames % 3 != 0 || hop_frames < kClipFrames / 2 || hop_frames > kClipFrames)
        return amuse_failf(AMUSE_EINVAL, "amuse_longform_plan: hop_frames %d must be a multiple of 3 in %d..%d", hop_frames, kClipFrames / 2, kClipFrames);
    if (n_samples > (long long)INT_MAX / 3 * kSamplesPerFrame3)
        return amuse_failf(AMUSE_EINVAL, "amuse_longform_plan: n_samples %lld gives more frames than an int holds", n_samples);
    const long long fl = 3 * n_samples / kSamplesPerFrame3;
    const int L = fl < kClipFrames ? kClipFrames : (int)fl;
    const int W = L <= kClipFrames ? 1 : (L - kClipFrames + hop_frames - 1) / hop_frames + 1;
    if (windows) *windows = W;
    if (frames) *frames = L;
    if (hop_samples) *hop_samples = hop_frames / 3 * kSamplesPerFrame3;
    return AMUSE_OK;
}

// ---- the join's argument checks: everything that can be refused without touching the GPU
inline int stitch_check(const float* poses, const float* trans, int S, const int* windows, const int* frames, int F, int hop, const float* blend,
                        float* poses_out, float* trans_out) {
    if (S < 1) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: S %d < 1", S);
    if (F < 2) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: F %d < 2", F);
    if (hop < F / 2 || hop > F) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: hop %d outside F / 2 .. F = %d .. %d (at most two windows may cover a frame)", hop, F / 2, F);
    if (!windows || !frames) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: windows and frames must be given");
    long long wins = 0, out = 0;
    for (int s = 0; s < S; ++s) {
        const long long W = windows[s], L = frames[s];
        if (W < 1) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: sequence %d has %lld windows", s, W);
        if (L <= (W - 1) * hop || L > (W - 1) * hop + F)
            return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: sequence %d: %lld frames do not fit %lld windows of %d frames at hop %d (%lld < frames <= %lld)", s, L, W,
                               F, hop, (W - 1) * hop, (W - 1) * hop + F);
        wins += W;
        out += L;
        // window rows, output frames and the (frame, slot) thread index are ints in the kernel; it forms its element offsets in 64 bits
        if (wins * F > INT_MAX || out * kMotionSlots > INT_MAX) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: more frames in one call than the kernel's int indices hold");
    }
    if (!poses || !poses_out) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: poses and poses_out must be given");
    if (!blend && hop < F) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: blend is NULL with an overlap of %d frames", F - hop);
    if ((trans == nullptr) != (trans_out == nullptr)) return amuse_failf(AMUSE_EINVAL, "amuse_stitch_windows: trans and trans_out are NULL together");
    return AMUSE_OK;
}

// ---- checks, then the sequences in launches (hidden: only the C entry point calls it, and the library exports no new name for it)
__attribute__((visibility("hidden"))) inline int stitch_windows(const float* poses, const float* trans, int S, const int* windows, const int* frames, int F, int hop, const float* blend, float* poses_out,
                          float* trans_out, hipStream_t stream) {
    if (int rc = stitch_check(poses, trans, S, windows, frames, F, hop, blend, poses_out, trans_out)) return rc;
    StitchArgs p{};
    p.poses = poses; p.trans = trans; p.blend = blend; p.poses_out = poses_out; p.trans_out = trans_out;
    p.F = F; p.hop = hop;
    int win0 = 0, out0 = 0;
    auto fill = [&](StitchArgs& a, int k, int s) {
        a.seq[k] = StitchSeq{win0, out0, windows[s], frames[s]};
        win0 += windows[s];
        out0 += frames[s];
        if (frames[s] > a.max_L) a.max_L = frames[s];
    };
    return launch_sequences("amuse_stitch_windows", S, p, fill, launch_stitch, stream);
}

}  // namespace amuse
