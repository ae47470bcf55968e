// The join of long-form inference (include/amuse_hip.h amuse_stitch_windows): the windows of a sequence, sampled independently at a stride of `hop` frames, become
// ONE motion.  A frame only one window produced - or the later window's part past the overlap - is a bitwise copy of that window's row; a frame two neighbouring
// windows both produced is their rotation crossfade, joint by joint: axis-angle -> unit quaternion, shorter arc, slerp at the caller's weight, back to axis-angle
// (the translation: a lerp).  One thread per (output frame, joint | translation): at most 24 B in and 12 B out each, nothing shared, no LDS; the sequence is the
// grid's y, its offsets sit in the kernel arguments.  A translation unit of its own; the quaternion conversions are amuse_rot.hpp's.
#include "amuse_rot.hpp"
#include "amuse_stitch_host.hpp"

namespace amuse {

namespace {

__device__ __forceinline__ void stitch_joint(const float* __restrict__ a, const float* __restrict__ b, float w, float (&out)[3]) {
    const Quat qa = aa_to_quat(a[0], a[1], a[2]);
    Quat qb = aa_to_quat(b[0], b[1], b[2]);
    float d = qa.w * qb.w + qa.x * qb.x + qa.y * qb.y + qa.z * qb.z;
    if (d < 0.f) { qb.w = -qb.w; qb.x = -qb.x; qb.y = -qb.y; qb.z = -qb.z; d = -d; }      // the shorter arc
    // the angle between them from the part of q_b orthogonal to q_a (acos of d loses everything as d -> 1)
    const float rw = qb.w - d * qa.w, rx = qb.x - d * qa.x, ry = qb.y - d * qa.y, rz = qb.z - d * qa.z;
    const float omega = atan2f(sqrtf(rw * rw + rx * rx + ry * ry + rz * rz), d);
    const float so = sinf(omega);
    float ca = 1.f - w, cb = w;                                                           // sin Omega too small to divide by: the slerp's own limit
    if (so >= 1e-4f) { ca = sinf((1.f - w) * omega) / so; cb = sinf(w * omega) / so; }
    const float qw = ca * qa.w + cb * qb.w, qx = ca * qa.x + cb * qb.x, qy = ca * qa.y + cb * qb.y, qz = ca * qa.z + cb * qb.z;
    quat_to_aa(quat_unit_short(Quat{qw, qx, qy, qz}), out);                               // blended frames carry the short representation
}

__global__ void __launch_bounds__(kStitchBlock) k_stitch(const StitchArgs a) {
    const StitchSeq sq = a.seq[blockIdx.y];
    const int idx = blockIdx.x * kStitchBlock + threadIdx.x;
    const int f = idx / kMotionSlots, j = idx - f * kMotionSlots;
    if (f >= sq.L) return;
    const bool is_trans = j == kSmplxJoints;
    if (is_trans && a.trans == nullptr) return;
    int k = f / a.hop;
    if (k > sq.W - 1) k = sq.W - 1;
    const int i = f - k * a.hop;                       // the frame's row in window k: < F by the entry point's check on L
    const size_t row_b = (size_t)(sq.win0 + k) * a.F + i, row_o = (size_t)sq.out0 + f;
    const float* src = is_trans ? a.trans + row_b * 3 : a.poses + (row_b * kSmplxJoints + j) * 3;
    float* dst = is_trans ? a.trans_out + row_o * 3 : a.poses_out + (row_o * kSmplxJoints + j) * 3;
    const float b0 = src[0], b1 = src[1], b2 = src[2];
    if (k == 0 || i >= a.F - a.hop) {                  // one window's frame: its bits
        dst[0] = b0; dst[1] = b1; dst[2] = b2;
        return;
    }
    const size_t row_a = row_b - a.F + a.hop;          // window k - 1, row i + hop: the same frame
    const float* pa = is_trans ? a.trans + row_a * 3 : a.poses + (row_a * kSmplxJoints + j) * 3;
    const float av[3] = {pa[0], pa[1], pa[2]}, bv[3] = {b0, b1, b2};
    const float w = a.blend[i];
    if (is_trans) {
        for (int c = 0; c < 3; ++c) dst[c] = (1.f - w) * av[c] + w * bv[c];
        return;
    }
    float o[3];
    stitch_joint(av, bv, w, o);
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

}  // namespace

hipError_t launch_stitch(const StitchArgs& a, hipStream_t stream) {
    const long long threads = (long long)a.max_L * kMotionSlots;
    const dim3 grid((unsigned)((threads + kStitchBlock - 1) / kStitchBlock), (unsigned)a.nseq);
    hipLaunchKernelGGL(k_stitch, grid, dim3(kStitchBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
