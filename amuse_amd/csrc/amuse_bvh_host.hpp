// BVH export (include/amuse_hip.h amuse_bvh_layout / amuse_bvh_format / amuse_bvh_motion / amuse_bvh_decode): everything the export needs on the host, shared by
// k_bvh.hip (the kernels and their launchers), amuse_bvh.hip (the C entry points) and tests/bvh_host (the same host code on stand-in launchers, under sanitizers):
//   - the layout: the depth-first column order of a parent list, children in ascending index;
//   - the argument checks of the formatter, the exporter and the decoder, made before any HIP call;
//   - a call's sequences, packed into launches by amuse_seq_host.hpp; the 55 column joints travel by value beside them.
// Context-free: nothing here reads or keeps state.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kBvhCols = AMUSE_BVH_COLS;                  // numbers of a MOTION row: 3 root positions + 55 x 3 angles
constexpr int kBvhField = AMUSE_BVH_FIELD;                // bytes of a number: %11.6f and its separator
constexpr int kBvhRowBytes = kBvhCols * kBvhField;        // 2,016: a multiple of 4, so every field of every row is dword-aligned from an aligned base
constexpr int kBvhBlock = 256;
constexpr int kBvhMaxFrames = (INT_MAX - kBvhBlock) / kMotionSlots;   // a launch's (frame, slot) index, rounded up to whole workgroups, is an int
constexpr int kBvhWalkBlock = 64;                         // the unwrap walk: one lane per (sequence, column joint), one wave per workgroup
static_assert(kBvhRowBytes % 4 == 0 && kBvhCols == 3 + 3 * kSmplxJoints, "row layout");

struct BvhSeq {
    long long row0;   // first frame of the sequence (index into poses / trans / euler_out rows; text_out byte offset / 2016)
    int F;            // frames
    int s;            // the sequence's index in the CALL: its root_rest row and its status word
};

struct BvhArgs {
    const float* poses;       // [rows][55][3]
    const float* trans;       // [rows][3] or null
    const float* root_rest;   // [S][3]
    float* euler;             // [rows][168] or null
    unsigned char* text;      // [rows][2016] or null
    int* status;              // [S]
    float scale;
    int ai, aj, ak;           // the axes of the three channels, in channel order: R = R_ai R_aj R_ak
    float e;                  // the permutation sign of (ak, aj, ai)
    int unwrap, nseq, max_F;
    unsigned char dfs[kSmplxJoints];   // column c holds joint dfs[c]
    BvhSeq seq[kSeqPerLaunch];
};

struct BvhDecodeArgs {
    const float* channels;    // [rows][168]
    const float* root_rest;   // [S][3]
    float* poses_out;         // [rows][55][3]
    float* trans_out;         // [rows][3]
    float scale;
    int ai, aj, ak, nseq, max_F;
    unsigned char dfs[kSmplxJoints];
    BvhSeq seq[kSeqPerLaunch];
};

// k_bvh.hip (tests/bvh_host: stand-ins that record the arguments)
hipError_t launch_bvh_format(const float* values, long long n, int per_row, unsigned char* text, int* status, hipStream_t stream);
hipError_t launch_bvh_motion(const BvhArgs& a, hipStream_t stream);
hipError_t launch_bvh_decode(const BvhDecodeArgs& a, hipStream_t stream);

// ---- the layout.  parents[0] = -1 and 0 <= parents[j] < j, as BodyModel holds them; children in ascending index, so the list is built from the last joint down
inline int bvh_layout(const int* parents, int n, int* dfs_out) {
    if (n < 1 || n > 65536) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_layout: n %d outside 1..65536", n);
    if (!parents || !dfs_out) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_layout: parents and dfs_out must be given");
    if (parents[0] != -1) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_layout: parents[0] = %d, not -1", parents[0]);
    for (int j = 1; j < n; ++j)
        if (parents[j] < 0 || parents[j] >= j) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_layout: parents[%d] = %d outside 0..%d", j, parents[j], j - 1);
    std::vector<int> first(n, -1), next(n, -1), stack;
    for (int j = n - 1; j >= 1; --j) {
        next[j] = first[parents[j]];
        first[parents[j]] = j;
    }
    // a joint's next column is its first child, else the next sibling of the nearest ancestor that has one
    stack.reserve(n);
    int out = 0, j = 0;
    while (j >= 0) {
        dfs_out[out++] = j;
        if (next[j] >= 0) stack.push_back(next[j]);
        if (first[j] >= 0) {
            j = first[j];
        } else if (!stack.empty()) {
            j = stack.back();
            stack.pop_back();
        } else {
            j = -1;
        }
    }
    return AMUSE_OK;
}

// ---- the order: the six Tait-Bryan orders, AMUSE_BVH_XYZ .. AMUSE_BVH_ZYX; channel c turns about axis ax[c]
inline bool bvh_order_axes(int order, int (&ax)[3], float* e) {
    static const int tab[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    if (order < 0 || order > 5) return false;
    for (int c = 0; c < 3; ++c) ax[c] = tab[order][c];
    // the sign of the permutation (ak, aj, ai): even for the cyclic shifts of (0, 1, 2)
    if (e) *e = ((ax[2] + 1) % 3 == ax[1]) ? 1.f : -1.f;
    return true;
}

inline bool bvh_dfs_ok(const int* dfs) {
    bool seen[kSmplxJoints] = {};
    for (int c = 0; c < kSmplxJoints; ++c) {
        if (dfs[c] < 0 || dfs[c] >= kSmplxJoints || seen[dfs[c]]) return false;
        seen[dfs[c]] = true;
    }
    return true;
}

// frames: every F_s >= 1, and the call's rows x 168 numbers x 12 bytes within 2^62 (the kernels form their offsets in 64 bits; a launch's (frame, slot) index
// is an int, so one SEQUENCE holds at most kBvhMaxFrames frames)
inline int bvh_frames_check(const char* who, int S, const int* frames) {
    if (S < 1) return amuse_failf(AMUSE_EINVAL, "%s: S %d < 1", who, S);
    if (!frames) return amuse_failf(AMUSE_EINVAL, "%s: frames must be given", who);
    for (int s = 0; s < S; ++s)
        if (frames[s] < 1 || frames[s] > kBvhMaxFrames) return amuse_failf(AMUSE_EINVAL, "%s: sequence %d has %d frames (1..%d)", who, s, frames[s], kBvhMaxFrames);
    return AMUSE_OK;
}

// the exporter's and the decoder's sequences: rows back to back, each with its index in the call
struct BvhFill {
    const int* frames;
    long long row0 = 0;
    template <class Args>
    void operator()(Args& a, int k, int s) {
        a.seq[k] = BvhSeq{row0, frames[s], s};
        row0 += frames[s];
        if (frames[s] > a.max_F) a.max_F = frames[s];
    }
};

inline int bvh_format(const float* values, long long n, int per_row, unsigned char* text, int* status, hipStream_t stream) {
    if (n < 1 || n > (long long)INT_MAX * kBvhBlock) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_format: n %lld outside 1..%lld", n, (long long)INT_MAX * kBvhBlock);
    if (per_row < 1) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_format: per_row %d < 1", per_row);
    if (!values || !text || !status) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_format: values, text_out and status must be given");
    if (reinterpret_cast<uintptr_t>(text) % 4) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_format: text_out must be 4-byte aligned (a field is stored as three dwords)");
    const hipError_t e = launch_bvh_format(values, n, per_row, text, status, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_bvh_format: launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

inline int bvh_motion(const float* poses, const float* trans, const float* root_rest, int S, const int* frames, const int* dfs, int order, float scale, int unwrap,
                      float* euler, unsigned char* text, int* status, hipStream_t stream) {
    if (int rc = bvh_frames_check("amuse_bvh_motion", S, frames)) return rc;
    int ax[3];
    float e;
    if (!bvh_order_axes(order, ax, &e)) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_motion: order %d outside 0..5 (AMUSE_BVH_XYZ .. AMUSE_BVH_ZYX)", order);
    if (!dfs || !bvh_dfs_ok(dfs)) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_motion: dfs must be a permutation of 0..54 (amuse_bvh_layout)");
    if (!(scale > 0.f) || !std::isfinite(scale)) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_motion: scale %g must be positive and finite", (double)scale);
    if (!poses || !root_rest || !status) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_motion: poses, root_rest and status must be given");
    if (!euler && !text) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_motion: euler_out and text_out are both NULL: nothing to write");
    if (reinterpret_cast<uintptr_t>(text) % 4) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_motion: text_out must be 4-byte aligned (a field is stored as three dwords)");
    BvhArgs p{};
    p.poses = poses; p.trans = trans; p.root_rest = root_rest; p.euler = euler; p.text = text; p.status = status;
    p.scale = scale; p.ai = ax[0]; p.aj = ax[1]; p.ak = ax[2]; p.e = e; p.unwrap = unwrap ? 1 : 0;
    for (int c = 0; c < kSmplxJoints; ++c) p.dfs[c] = (unsigned char)dfs[c];
    return launch_sequences("amuse_bvh_motion", S, p, BvhFill{frames}, launch_bvh_motion, stream);
}

inline int bvh_decode(const float* channels, int S, const int* frames, const int* dfs, int order, float scale, const float* root_rest, float* poses_out,
                      float* trans_out, hipStream_t stream) {
    if (int rc = bvh_frames_check("amuse_bvh_decode", S, frames)) return rc;
    int ax[3];
    if (!bvh_order_axes(order, ax, nullptr)) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_decode: order %d outside 0..5 (AMUSE_BVH_XYZ .. AMUSE_BVH_ZYX)", order);
    if (!dfs || !bvh_dfs_ok(dfs)) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_decode: dfs must be a permutation of 0..54 (amuse_bvh_layout)");
    if (!(scale > 0.f) || !std::isfinite(scale)) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_decode: scale %g must be positive and finite", (double)scale);
    if (!channels || !root_rest || !poses_out || !trans_out) return amuse_failf(AMUSE_EINVAL, "amuse_bvh_decode: channels, root_rest, poses_out and trans_out must be given");
    BvhDecodeArgs p{};
    p.channels = channels; p.root_rest = root_rest; p.poses_out = poses_out; p.trans_out = trans_out;
    p.scale = scale; p.ai = ax[0]; p.aj = ax[1]; p.ak = ax[2];
    for (int c = 0; c < kSmplxJoints; ++c) p.dfs[c] = (unsigned char)dfs[c];
    return launch_sequences("amuse_bvh_decode", S, p, BvhFill{frames}, launch_bvh_decode, stream);
}

}  // namespace amuse
