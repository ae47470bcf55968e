// Long-form candidates (include/amuse_hip.h amuse_seam_plan / amuse_seam_cost / amuse_seam_path / amuse_seam_select): everything the seam choice needs on the
// host, shared by k_seam.hip (the kernels and their launchers), amuse_seam.hip (the four C entry points) and tests/seam_host (the same host code on stand-in
// launchers, under sanitizers):
//   - the plan: the ONE statement of how many seams a call has and how many bytes of quaternions amuse_seam_cost keeps for them;
//   - the argument checks of the three device entry points, made before any HIP call;
//   - the call's sequences, packed into launches by amuse_seq_host.hpp.
// Context-free: nothing here reads or keeps state.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kSeamBlock = 256;           // the conversion and the gather: a thread per element; the cost: four waves, a pair each
constexpr int kSeamMaxK = 64;             // candidates per window: a lane each in the path kernel
constexpr int kSeamPathWindows = 960;     // back-pointers the path kernel keeps in LDS at a time: 960 windows x 64 candidates x 1 B = 60 KiB
constexpr int kSeamMaxWindows = 32768;    // windows per sequence: 2 x its seams are a grid dimension of the conversion

struct SeamSeq {
    int win0;     // first window of the sequence (batch row win0 * K is its window 0, candidate 0)
    int seam0;    // first seam of the sequence (index into cost_out in [K][K] matrices, into the workspace in seams)
    int W, L;     // windows, output frames
};

struct SeamArgs {
    const float* poses;          // [windows * K][F][55][3]
    const float* trans;          // [windows * K][F][3] or null
    const float* row_weight;     // [F - hop]
    const float* joint_weight;   // [55]
    float4* quats;               // the workspace: [seams][2 sides][K][F - hop][55] (w, x, y, z)
    double* cost;                // [seams][K][K]
    float trans_weight;
    int K, F, hop, nseq, max_seams;
    SeamSeq seq[kSeqPerLaunch];
};

struct PathArgs {
    const double* cost;          // [seams][K][K]
    int* choice;                 // [windows]
    double* total;               // [sequences]
    int K, nseq, seq0;           // seq0: the call's index of the launch's first sequence
    SeamSeq seq[kSeqPerLaunch];  // (L unused: 0)
};

struct SelectArgs {
    const float* poses;
    const float* trans;
    const int* choice;
    float* poses_out;
    float* trans_out;
    int n, n_in, F;
};

// k_seam.hip (tests/seam_host: stand-ins that record the arguments)
hipError_t launch_seam_cost(const SeamArgs& a, hipStream_t stream);
hipError_t launch_seam_path(const PathArgs& a, hipStream_t stream);
hipError_t launch_seam_select(const SelectArgs& a, hipStream_t stream);

// ---- what the plan and the cost share: S, windows, K, F, hop -> seams and window rows
inline int seam_shape_check(const char* entry, int S, const int* windows, int K, int F, int hop, long long* seams, long long* wins) {
    if (S < 1) return amuse_failf(AMUSE_EINVAL, "%s: S %d < 1", entry, S);
    if (!windows) return amuse_failf(AMUSE_EINVAL, "%s: windows must be given", entry);
    if (K < 1 || K > kSeamMaxK) return amuse_failf(AMUSE_EINVAL, "%s: K %d outside 1..%d candidates", entry, K, kSeamMaxK);
    if (F < 2) return amuse_failf(AMUSE_EINVAL, "%s: F %d < 2", entry, F);
    long long n = 0, w = 0;
    for (int s = 0; s < S; ++s) {
        if (windows[s] < 1 || windows[s] > kSeamMaxWindows) return amuse_failf(AMUSE_EINVAL, "%s: sequence %d has %d windows (1..%d)", entry, s, windows[s], kSeamMaxWindows);
        n += windows[s] - 1;
        w += windows[s];
    }
    if (n > 0 && (hop < F / 2 || hop >= F))
        return amuse_failf(AMUSE_EINVAL, "%s: hop %d outside F / 2 .. F - 1 = %d .. %d (a seam needs an overlap, and at most two windows may cover a frame)", entry, hop, F / 2, F - 1);
    if (n == 0 && (hop < F / 2 || hop > F)) return amuse_failf(AMUSE_EINVAL, "%s: hop %d outside F / 2 .. F = %d .. %d", entry, hop, F / 2, F);
    // batch rows x F and the cost matrix's entries are ints in the kernels; they form their element offsets in 64 bits
    if (w * K * F > INT_MAX || n * K * K > INT_MAX) return amuse_failf(AMUSE_EINVAL, "%s: more window rows or seam pairs in one call than the kernels' int indices hold", entry);
    *seams = n;
    *wins = w;
    return AMUSE_OK;
}

inline size_t seam_workspace_bytes(long long seams, int K, int F, int hop) {
    return (size_t)seams * 2 * (size_t)K * (size_t)(F - hop) * kSmplxJoints * sizeof(float4);
}

// ---- the plan (host only)
inline int seam_plan(int S, const int* windows, int K, int F, int hop, long long* seams, size_t* workspace_bytes) {
    long long n = 0, w = 0;
    if (int rc = seam_shape_check("amuse_seam_plan", S, windows, K, F, hop, &n, &w)) return rc;
    if (seams) *seams = n;
    if (workspace_bytes) *workspace_bytes = n ? seam_workspace_bytes(n, K, F, hop) : 0;
    return AMUSE_OK;
}

// ---- the cost matrix: checks, then the sequences in launches (hidden: only the C entry point calls it)
__attribute__((visibility("hidden"))) inline int seam_cost(const float* poses, const float* trans, int S, const int* windows, const int* frames, int K, int F, int hop,
                                                            const float* row_weight, const float* joint_weight, float trans_weight, void* workspace, double* cost_out,
                                                            hipStream_t stream) {
    const char* me = "amuse_seam_cost";
    long long seams = 0, wins = 0;
    if (int rc = seam_shape_check(me, S, windows, K, F, hop, &seams, &wins)) return rc;
    if (!frames) return amuse_failf(AMUSE_EINVAL, "%s: frames must be given", me);
    for (int s = 0; s < S; ++s) {
        const long long W = windows[s], L = frames[s];
        if (L <= (W - 1) * hop || L > (W - 1) * hop + F)
            return amuse_failf(AMUSE_EINVAL, "%s: sequence %d: %lld frames do not fit %lld windows of %d frames at hop %d (%lld < frames <= %lld)", me, s, L, W, F, hop,
                               (W - 1) * hop, (W - 1) * hop + F);
    }
    if (!poses) return amuse_failf(AMUSE_EINVAL, "%s: poses must be given", me);
    if (!trans && trans_weight != 0.f) return amuse_failf(AMUSE_EINVAL, "%s: trans is NULL with trans_weight %g (must be 0)", me, (double)trans_weight);
    if (!(trans_weight >= 0.f) || !(trans_weight <= 3.0e38f)) return amuse_failf(AMUSE_EINVAL, "%s: trans_weight %g must be finite and >= 0", me, (double)trans_weight);
    if (!joint_weight) return amuse_failf(AMUSE_EINVAL, "%s: joint_weight must be given", me);
    if (seams == 0) return AMUSE_OK;                                     // nothing to score: no launch, the other pointers may be NULL
    if (!row_weight) return amuse_failf(AMUSE_EINVAL, "%s: row_weight is NULL with an overlap of %d frames", me, F - hop);
    if (!cost_out) return amuse_failf(AMUSE_EINVAL, "%s: cost_out must be given", me);
    if (!workspace) return amuse_failf(AMUSE_EINVAL, "%s: workspace is NULL; amuse_seam_plan asks for %zu bytes", me, seam_workspace_bytes(seams, K, F, hop));
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(float4)) return amuse_failf(AMUSE_EINVAL, "%s: workspace must be aligned to %zu bytes", me, sizeof(float4));
    SeamArgs p{};
    p.poses = poses; p.trans = trans; p.row_weight = row_weight; p.joint_weight = joint_weight;
    p.quats = static_cast<float4*>(workspace); p.cost = cost_out; p.trans_weight = trans_weight;
    p.K = K; p.F = F; p.hop = hop;
    int win0 = 0, seam0 = 0;
    auto fill = [&](SeamArgs& a, int k, int s) {
        a.seq[k] = SeamSeq{win0, seam0, windows[s], frames[s]};
        win0 += windows[s];
        seam0 += windows[s] - 1;
        if (windows[s] - 1 > a.max_seams) a.max_seams = windows[s] - 1;
    };
    return launch_sequences(me, S, p, fill, launch_seam_cost, stream);
}

// ---- the best path
__attribute__((visibility("hidden"))) inline int seam_path(const double* cost, int S, const int* windows, int K, int* choice_out, double* total_out, hipStream_t stream) {
    const char* me = "amuse_seam_path";
    if (S < 1) return amuse_failf(AMUSE_EINVAL, "%s: S %d < 1", me, S);
    if (!windows) return amuse_failf(AMUSE_EINVAL, "%s: windows must be given", me);
    if (K < 1 || K > kSeamMaxK) return amuse_failf(AMUSE_EINVAL, "%s: K %d outside 1..%d candidates", me, K, kSeamMaxK);
    long long seams = 0, wins = 0;
    for (int s = 0; s < S; ++s) {
        if (windows[s] < 1) return amuse_failf(AMUSE_EINVAL, "%s: sequence %d has %d windows", me, s, windows[s]);
        seams += windows[s] - 1;
        wins += windows[s];
    }
    if (wins * K > INT_MAX || seams * K * K > INT_MAX) return amuse_failf(AMUSE_EINVAL, "%s: more window rows or seam pairs in one call than the kernel's int indices hold", me);
    if (!cost && seams > 0) return amuse_failf(AMUSE_EINVAL, "%s: cost is NULL with %lld seams", me, seams);
    if (!choice_out || !total_out) return amuse_failf(AMUSE_EINVAL, "%s: choice_out and total_out must be given", me);
    PathArgs p{};
    p.cost = cost; p.choice = choice_out; p.total = total_out; p.K = K;
    int win0 = 0, seam0 = 0;
    auto fill = [&](PathArgs& a, int k, int s) {
        if (k == 0) a.seq0 = s;
        a.seq[k] = SeamSeq{win0, seam0, windows[s], 0};
        win0 += windows[s];
        seam0 += windows[s] - 1;
    };
    return launch_sequences(me, S, p, fill, launch_seam_path, stream);
}

// ---- the gather
__attribute__((visibility("hidden"))) inline int seam_select(const float* poses, const float* trans, const int* choice, int n, int n_in, int F, float* poses_out, float* trans_out,
                                                              hipStream_t stream) {
    const char* me = "amuse_seam_select";
    if (n < 1 || n_in < 1) return amuse_failf(AMUSE_EINVAL, "%s: n %d and n_in %d must be >= 1", me, n, n_in);
    if (F < 1) return amuse_failf(AMUSE_EINVAL, "%s: F %d < 1", me, F);
    if ((long long)n * F > INT_MAX || (long long)n_in * F > INT_MAX) return amuse_failf(AMUSE_EINVAL, "%s: more frames in one call than the kernel's int indices hold", me);
    if (!poses || !choice || !poses_out) return amuse_failf(AMUSE_EINVAL, "%s: poses, choice and poses_out must be given", me);
    if ((trans == nullptr) != (trans_out == nullptr)) return amuse_failf(AMUSE_EINVAL, "%s: trans and trans_out are NULL together", me);
    const long long pin = (long long)n_in * F * kSmplxJoints * 3, tin = (long long)n_in * F * 3, pout = (long long)n * F * kSmplxJoints * 3, tout = (long long)n * F * 3;
    const float* ins[3] = {poses, trans, reinterpret_cast<const float*>(choice)};
    const long long in_floats[3] = {pin, tin, n};
    const float* outs[2] = {poses_out, trans_out};
    const long long out_floats[2] = {pout, tout};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 3; ++i)
            if (outs[o] && ins[i] && ranges_overlap(outs[o], out_floats[o], ins[i], in_floats[i]))
                return amuse_failf(AMUSE_EINVAL, "%s: an output range overlaps an input range (in place is refused)", me);
    if (trans_out && ranges_overlap(poses_out, pout, trans_out, tout)) return amuse_failf(AMUSE_EINVAL, "%s: poses_out and trans_out overlap", me);
    const hipError_t e = launch_seam_select(SelectArgs{poses, trans, choice, poses_out, trans_out, n, n_in, F}, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "%s: launch failed: %s", me, hipGetErrorString(e));
    return AMUSE_OK;
}

}  // namespace amuse
