// The rotation arithmetic of the motion kernels (k_stitch.hip, k_smooth.hip, k_bvh.hip), stated once: unit quaternions (w, x, y, z) and their way to and from
// axis-angle.  Every expression keeps the operand order its kernels were pinned with: HIP contracts a * b + c to an FMA, and which product of a sum is the
// FMA's follows the order the compiler leaves the sum in, so the three units are held to the ISA they had with private copies (tools/isa_identity.py).
// Two statements stay outside for that reason: the decode tail (amuse_dev.hpp rot6d_to_axis_angle ends in quat_to_aa's lines; the benchmarked decode kernels'
// instructions move when it is routed through here) and the plain product q1 q2 (k_smooth.hip's `qc e`: behind a helper its qz contracts the other way).
#pragma once
#include <hip/hip_runtime.h>

namespace amuse {

struct Quat { float w, x, y, z; };

// axis-angle -> unit quaternion: half-angle sine and cosine, the sine term by its series below `series_below` (sin(a / 2) / a -> 1 / 2 - a^2 / 48, as
// train_gesture.axis_angle_to_rotation_6d has it)
__device__ __forceinline__ Quat aa_to_quat(float x, float y, float z, float series_below = 1e-6f) {
    const float ang = sqrtf(x * x + y * y + z * z);
    const float half = 0.5f * ang;
    const float s = (ang < series_below) ? (0.5f - (ang * ang) / 48.0f) : (sinf(half) / ang);
    return Quat{cosf(half), x * s, y * s, z * s};
}

// quaternion_to_axis_angle (rotation_conversions.py:480-509): the angle is 2 atan2(|v|, w), in [0, 2 pi) for a quaternion of either sign
__device__ __forceinline__ void quat_to_aa(const Quat& q, float (&aa)[3]) {
    const float nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z);
    const float half = atan2f(nrm, q.w);
    const float ang = 2.0f * half;
    const float s = (fabsf(ang) < 1e-6f) ? (0.5f - (ang * ang) / 48.0f) : (sinf(half) / ang);
    aa[0] = q.x / s; aa[1] = q.y / s; aa[2] = q.z / s;
}

// conj(a) b
__device__ __forceinline__ Quat quat_conj_mul(const Quat& a, const Quat& b) {
    return Quat{a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z,
                a.w * b.x - a.x * b.w - a.y * b.z + a.z * b.y,
                a.w * b.y + a.x * b.z - a.y * b.w - a.z * b.x,
                a.w * b.z - a.x * b.y + a.y * b.x - a.z * b.w};
}

// q / |q| with w >= 0: of the two unit quaternions of a rotation, the one whose angle is at most pi
__device__ __forceinline__ Quat quat_unit_short(const Quat& q) {
    float inv = 1.f / sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    if (q.w < 0.f) inv = -inv;
    return Quat{q.w * inv, q.x * inv, q.y * inv, q.z * inv};
}

}  // namespace amuse
