// Motion smoothing (include/amuse_hip.h amuse_smooth_banks / amuse_smooth_motion): everything the filter needs on the host, shared by k_smooth.hip (the kernel
// and its launcher), amuse_smooth.hip (the two C entry points) and tests/smooth_host (the same host code on a stand-in launcher, under sanitizers):
//   - the bank: the hat matrices H_1 .. H_15 of the local polynomial fit, in double, rounded to fp32;
//   - the argument checks of the filter, made before any HIP call;
//   - the call's sequences, packed into launches by amuse_seq_host.hpp; the 56 half-windows travel by value beside them.
// Context-free: nothing here reads or keeps state.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kSmoothMaxHalf = AMUSE_SMOOTH_MAX_HALF;     // m <= 15: windows up to 31 frames
constexpr int kSmoothMaxOrder = 5;
constexpr int kSmoothBankFloats = AMUSE_SMOOTH_BANK_FLOATS;
constexpr int kSmoothTile = 32;                           // T: output frames of one workgroup
constexpr int kSmoothBlock = 256;
constexpr int kSmoothLdsRows = kSmoothTile + 2 * kSmoothMaxHalf;   // the tile and the widest halo on either side

// H_m's first float in the bank: 9 + 25 + ... + (2 m - 1)^2 = n (4 n^2 + 12 n + 11) / 3 with n = m - 1
__host__ __device__ constexpr int smooth_bank_offset(int m) { return (m - 1) * (4 * (m - 1) * (m - 1) + 12 * (m - 1) + 11) / 3; }
static_assert(smooth_bank_offset(1) == 0 && smooth_bank_offset(2) == 9 && smooth_bank_offset(3) == 34, "bank layout");
static_assert(smooth_bank_offset(kSmoothMaxHalf + 1) == kSmoothBankFloats, "bank size");

struct SmoothSeq {
    int row0;     // first frame of the sequence (index into poses / trans and their outputs, in frames)
    int L;        // frames
};

struct SmoothArgs {
    const float* poses;      // [frames][55][3]
    const float* trans;      // [frames][3] or null
    const float* banks;      // [5455]
    float* poses_out;        // [frames][55][3]
    float* trans_out;        // [frames][3] or null
    int nseq, max_L, halo;   // halo: the largest half-window a slot of this call filters with (rows loaded on either side of a tile)
    unsigned char hw[kMotionSlots];
    SmoothSeq seq[kSeqPerLaunch];
};

// k_smooth.hip (tests/smooth_host: a stand-in that records the arguments)
hipError_t launch_smooth(const SmoothArgs& a, hipStream_t stream);

// ---- the bank.  H = Q Q^T for an orthonormal basis Q of the columns of A: the same matrix as A (A^T A)^-1 A^T.  Q by modified Gram-Schmidt, each column
// orthogonalised twice, on the abscissae (i - m) / m (a column scaling of A: the column space, hence H, is unchanged).
inline void smooth_hat(int m, int pm, double* H /* [(2 m + 1)^2] */) {
    const int n = 2 * m + 1, nd = pm + 1;
    double Q[kSmoothMaxOrder + 1][2 * kSmoothMaxHalf + 1];
    for (int d = 0; d < nd; ++d) {
        for (int i = 0; i < n; ++i) Q[d][i] = std::pow((double)(i - m) / (double)m, d);
        for (int pass = 0; pass < 2; ++pass)
            for (int e = 0; e < d; ++e) {
                double dot = 0.0;
                for (int i = 0; i < n; ++i) dot += Q[e][i] * Q[d][i];
                for (int i = 0; i < n; ++i) Q[d][i] -= dot * Q[e][i];
            }
        double nn = 0.0;
        for (int i = 0; i < n; ++i) nn += Q[d][i] * Q[d][i];
        nn = std::sqrt(nn);
        for (int i = 0; i < n; ++i) Q[d][i] /= nn;
    }
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            for (int d = 0; d < nd; ++d) s += Q[d][r] * Q[d][k];
            H[r * n + k] = s;
        }
}

inline int smooth_banks(int order, float* out) {
    if (order < 0 || order > kSmoothMaxOrder) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_banks: order %d outside 0..%d", order, kSmoothMaxOrder);
    if (!out) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_banks: banks_out_host is NULL");
    double H[(2 * kSmoothMaxHalf + 1) * (2 * kSmoothMaxHalf + 1)];
    for (int m = 1; m <= kSmoothMaxHalf; ++m) {
        const int n = 2 * m + 1;
        smooth_hat(m, order < 2 * m ? order : 2 * m, H);
        float* dst = out + smooth_bank_offset(m);
        for (int i = 0; i < n * n; ++i) dst[i] = (float)H[i];
    }
    return AMUSE_OK;
}

// ---- the filter's argument checks: everything that can be refused without touching the GPU
inline int smooth_check(const float* poses, const float* trans, int S, const int* frames, const unsigned char* half_window, const float* banks, float* poses_out,
                        float* trans_out) {
    if (S < 1) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: S %d < 1", S);
    if (!frames || !half_window) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: frames and half_window must be given");
    long long total = 0;
    for (int s = 0; s < S; ++s) {
        if (frames[s] < 1) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: sequence %d has %d frames", s, frames[s]);
        total += frames[s];
        // frames and the (frame, slot) index are ints in the kernel; it forms its element offsets in 64 bits
        if (total * kMotionSlots > INT_MAX) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: more frames in one call than the kernel's int indices hold");
    }
    for (int i = 0; i < kMotionSlots; ++i)
        if (half_window[i] > kSmoothMaxHalf)
            return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: half_window[%d] = %d above %d", i, (int)half_window[i], kSmoothMaxHalf);
    if (!poses || !poses_out || !banks) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: poses, poses_out and banks_dev must be given");
    if ((trans == nullptr) != (trans_out == nullptr)) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: trans and trans_out are NULL together");
    // the filter reads a frame's neighbours: an output that overlaps an input would be read after it was written
    const long long np = total * kSmplxJoints * 3, nt = total * 3;
    bool ov = ranges_overlap(poses_out, np, poses, np);
    if (trans) ov = ov || ranges_overlap(trans_out, nt, trans, nt) || ranges_overlap(poses_out, np, trans, nt) || ranges_overlap(trans_out, nt, poses, np);
    if (ov) return amuse_failf(AMUSE_EINVAL, "amuse_smooth_motion: an output range overlaps an input range (the filter reads a frame's neighbours: not in place)");
    return AMUSE_OK;
}

// ---- checks, then the sequences in launches (hidden: only the C entry point calls it, and the library exports no new name for it)
__attribute__((visibility("hidden"))) inline int smooth_motion(const float* poses, const float* trans, int S, const int* frames, const unsigned char* half_window, const float* banks, float* poses_out,
                         float* trans_out, hipStream_t stream) {
    if (int rc = smooth_check(poses, trans, S, frames, half_window, banks, poses_out, trans_out)) return rc;
    SmoothArgs p{};
    p.poses = poses; p.trans = trans; p.banks = banks; p.poses_out = poses_out; p.trans_out = trans_out;
    for (int i = 0; i < (trans ? kMotionSlots : kSmplxJoints); ++i)
        if (half_window[i] > p.halo) p.halo = half_window[i];
    for (int i = 0; i < kMotionSlots; ++i) p.hw[i] = half_window[i];
    int row0 = 0;
    auto fill = [&](SmoothArgs& a, int k, int s) {
        a.seq[k] = SmoothSeq{row0, frames[s]};
        row0 += frames[s];
        if (frames[s] > a.max_L) a.max_L = frames[s];
    };
    return launch_sequences("amuse_smooth_motion", S, p, fill, launch_smooth, stream);
}

}  // namespace amuse
