// Motion metrics (include/amuse_hip.h amuse_motion_metrics_row / amuse_motion_metrics): everything the call needs on the host, shared by k_motion_metrics.hip
// (the kernel and its launcher), amuse_motion_metrics.hip (the two C entry points) and tests/motion_metrics_host (the same host code on a stand-in launcher,
// under sanitizers):
//   - the row layout: the ONE statement of where each block of a clip's 442 doubles begins (amuse_amd/motion_metrics.py ROW_BLOCKS restates the table and a
//     test holds its total to amuse_motion_metrics_row());
//   - the argument checks, made before any HIP call;
//   - the launch: one workgroup per clip, kMetricsWaves waves of 64 with a lane per joint.
// Context-free: nothing here reads or keeps state.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kMetricsWaves = 8;                        // waves of a clip's workgroup: each walks a contiguous eighth of the clip's frames
constexpr int kMetricsBlock = 64 * kMetricsWaves;
constexpr int kMetricsPartials = 19;                    // doubles a lane hands over after the first pass (the second pass reuses 12 of the slots)
constexpr int kMetricsLdsBytes = kMetricsWaves * kMetricsPartials * 64 * 8;

// the row: block offsets in doubles (include/amuse_hip.h states the same table)
enum : int {
    kRowApeRoot = 0,                                    // 1
    kRowApeTraj = 1,                                    // 1
    kRowApePose = 2,                                    // 54: joints 1..54
    kRowApeJoints = kRowApePose + 54,                   // 55
    kRowAveRoot = kRowApeJoints + 55,                   // 1
    kRowAveTraj = kRowAveRoot + 1,                      // 1
    kRowAvePose = kRowAveTraj + 1,                      // 54
    kRowAveJoints = kRowAvePose + 54,                   // 55
    kRowVelGen = kRowAveJoints + 55,                    // 55
    kRowVelRef = kRowVelGen + 55,                       // 55
    kRowAccGen = kRowVelRef + 55,                       // 55
    kRowAccRef = kRowAccGen + 55,                       // 55
    kMetricsRow = kRowAccRef + 55,
};
static_assert(kMetricsRow == 442, "the row of include/amuse_hip.h");

struct MotionMetricsArgs {
    const float* gen;       // [N][F][55][3]
    const float* ref;       // [N][F][55][3]
    const int* lengths;     // dev [N]
    double* rows;           // dev [N][442]
    int N, F;
};

// k_motion_metrics.hip (tests/motion_metrics_host: a stand-in that records the arguments)
hipError_t launch_motion_metrics(const MotionMetricsArgs& a, hipStream_t stream);

// ---- the argument checks: everything that can be refused without touching the GPU (the lengths live on the device: the kernel answers a bad one with NaN)
inline int motion_metrics_check(const float* gen, const float* ref, const int* lengths_dev, int N, int F, const double* rows_out) {
    if (!gen || !ref) return amuse_failf(AMUSE_EINVAL, "amuse_motion_metrics: joints_gen and joints_ref must be given");
    if (!lengths_dev) return amuse_failf(AMUSE_EINVAL, "amuse_motion_metrics: lengths_dev must be given");
    if (!rows_out) return amuse_failf(AMUSE_EINVAL, "amuse_motion_metrics: rows_out must be given");
    if (N < 1) return amuse_failf(AMUSE_EINVAL, "amuse_motion_metrics: N %d < 1", N);
    if (F < 2) return amuse_failf(AMUSE_EINVAL, "amuse_motion_metrics: F %d < 2", F);
    // clips, frames and row indices are ints in the kernel; it forms its element offsets in 64 bits
    if ((long long)N * F > INT_MAX || (long long)N * kMetricsRow > INT_MAX)
        return amuse_failf(AMUSE_EINVAL, "amuse_motion_metrics: N %d x F %d: more frames or row entries in one call than an int holds", N, F);
    return AMUSE_OK;
}

// ---- checks, then one launch
inline int motion_metrics(const float* gen, const float* ref, const int* lengths_dev, int N, int F, double* rows_out, hipStream_t stream) {
    if (int rc = motion_metrics_check(gen, ref, lengths_dev, N, F, rows_out)) return rc;
    const MotionMetricsArgs a{gen, ref, lengths_dev, rows_out, N, F};
    const hipError_t e = launch_motion_metrics(a, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_motion_metrics: launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

}  // namespace amuse
