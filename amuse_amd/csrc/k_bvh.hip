// BVH export (include/amuse_hip.h amuse_bvh_format / amuse_bvh_motion / amuse_bvh_decode): SMPL-X axis-angle rows to Euler channels in degrees, and fp32 to the
// text of C's "%11.6f", on the GPU.  Four kernels, no LDS, no atomics, no matrix-core instruction, vector stores only:
//   k_bvh_format   one lane per number: the 12 bytes of a field (11 of the number, one separator) are assembled in registers and stored as three dwords.  Consecutive
//                  lanes store consecutive 12-byte fields, so a wave's stores cover 768 contiguous bytes.
//   k_bvh_motion   one lane per (frame, slot): slot c < 55 is column joint dfs[c] (three angles: three fields, 36 contiguous bytes), slot 55 the root's position.
//                  Fully parallel.  Without unwrap it writes the final values (the euler tap and / or the text); with unwrap it leaves the joints' PRINCIPAL
//                  values where the walk picks them up: in the euler tap, or - when the caller wants text alone - in the first dword of each number's own field.
//                  (The entry point may not allocate; a field is 12 bytes, the value 4, and the lane that reads it is the lane that overwrites it.)
//   k_bvh_walk     unwrap only: one lane per (sequence, column joint) walks the frames in order, picks the candidate nearer the frame before, formats.  The only
//                  sequential part; it does no transcendental work.
//   k_bvh_decode   one lane per (frame, slot): degrees -> three axis quaternions multiplied in channel order -> axis-angle with angle <= pi.
// The formatter: an fp32 times 1e6 is exact in double (a 24-bit by 14-bit significand product: 1e6 = 2^6 x 15625), so rint(double(x) * 1e6) - round-half-even,
// the default mode - is the integer printf prints, and the digits come out by 32-bit integer division.  One double multiply and one rint per number.
// A sequence's bytes depend on its own rows alone: every value is computed by one lane from that lane's inputs, with no reduction and no exchange.
#include "amuse_bvh_host.hpp"
#include "amuse_dev.hpp"
#include "amuse_rot.hpp"

namespace amuse {

namespace {

constexpr float kDeg = 57.29577951308232f;
constexpr float kRad = 0.017453292519943295f;

// the 12 bytes of one number as three little-endian dwords; false: it does not fit %11.6f (|x| rounds to 1000 or more, NaN, infinity) and the field is '#'
__device__ __forceinline__ bool bvh_field(float x, unsigned sep, unsigned (&w)[3]) {
    const double r = rint((double)x * 1e6);
    const bool ok = fabs(r) < 1e9;                       // (false for NaN)
    if (!ok) {
        w[0] = w[1] = 0x23232323u;
        w[2] = 0x00232323u | (sep << 24);
        return false;
    }
    const unsigned u = (unsigned)fabs(r);
    const unsigned ip = u / 1000000u, fr = u - ip * 1000000u;      // ip < 1000
    const bool neg = __float_as_uint(x) >> 31;                     // printf prints the sign of -0.0 and of a negative that rounds to zero
    const unsigned h = ip / 100u, t = (ip / 10u) % 10u, o = ip % 10u;
    // bytes 0..3: the integer part right-aligned, the sign just left of its first digit
    unsigned c0 = ' ', c1 = ' ', c2 = ' ';
    const unsigned c3 = '0' + o;
    if (ip >= 100u) { c1 = '0' + h; c2 = '0' + t; if (neg) c0 = '-'; }
    else if (ip >= 10u) { c2 = '0' + t; if (neg) c1 = '-'; }
    else if (neg) c2 = '-';
    w[0] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    const unsigned d0 = fr / 100000u, d1 = (fr / 10000u) % 10u, d2 = (fr / 1000u) % 10u, d3 = (fr / 100u) % 10u, d4 = (fr / 10u) % 10u, d5 = fr % 10u;
    w[1] = '.' | (('0' + d0) << 8) | (('0' + d1) << 16) | (('0' + d2) << 24);
    w[2] = ('0' + d3) | (('0' + d4) << 8) | (('0' + d5) << 16) | (sep << 24);
    return true;
}

__global__ void __launch_bounds__(kBvhBlock) k_bvh_format(const float* __restrict__ values, long long n, int per_row, unsigned* __restrict__ text, int* status) {
    const long long i = (long long)blockIdx.x * kBvhBlock + threadIdx.x;
    if (i >= n) return;
    unsigned w[3];
    const bool ok = bvh_field(values[i], (i % per_row == per_row - 1) ? '\n' : ' ', w);
    unsigned* dst = text + i * 3;
    dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
    if (!ok) *status = 1;
}

// (selects, not an indexed register array: no scratch)
__device__ __forceinline__ float bvh_pick(const float (&q)[3], int ax) { return ax == 0 ? q[0] : ax == 1 ? q[1] : q[2]; }

__device__ __forceinline__ float bvh_wrap180(float d) { return d - 360.0f * floorf((d + 180.0f) / 360.0f); }     // [-180, 180)

// the three channels in degrees, principal values: the half-sum / half-difference form on the quaternion (no rotation matrix)
__device__ __forceinline__ void bvh_euler(const float (&q)[3], float w, int ai, int aj, int ak, float e, float (&deg)[3]) {
    const float qi = bvh_pick(q, ai), qj = bvh_pick(q, aj), qk = bvh_pick(q, ak);
    const float a = w - qj, b = qk + e * qi, c = qj + w, d = e * qi - qk;
    const float mid = 2.0f * atan2f(hypotf(c, d), hypotf(a, b)) - 1.5707963267948966f;
    const bool ls = (a == 0.f && b == 0.f), ld = (c == 0.f && d == 0.f);     // exact gimbal lock: one pair vanishes, its angle is free
    float hs = ls ? 0.f : atan2f(b, a), hd = ld ? 0.f : atan2f(d, c);
    if (ls) hs = hd;                                                           // the free one is chosen so that the third channel is 0
    if (ld) hd = hs;
    deg[0] = bvh_wrap180(e * (hs + hd) * kDeg);
    deg[1] = mid * kDeg;
    deg[2] = bvh_wrap180((hs - hd) * kDeg);
}

__device__ __forceinline__ unsigned bvh_sep(int col) { return col == kBvhCols - 1 ? '\n' : ' '; }

// three consecutive numbers of row `row` from column `col` on: the tap, the text, the status
__device__ __forceinline__ void bvh_emit3(const BvhArgs& a, long long row, int col, const float (&v)[3], int s) {
    if (a.euler) {
        float* dst = a.euler + row * kBvhCols + col;
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
    }
    if (a.text) {
        unsigned* dst = reinterpret_cast<unsigned*>(a.text + row * kBvhRowBytes) + col * 3;
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            unsigned w[3];
            ok = bvh_field(v[k], bvh_sep(col + k), w) && ok;
            dst[3 * k] = w[0]; dst[3 * k + 1] = w[1]; dst[3 * k + 2] = w[2];
        }
        if (!ok) a.status[s] = 1;
    } else {
        bool ok = true;
        for (int k = 0; k < 3; ++k) ok = ok && fabs(rint((double)v[k] * 1e6)) < 1e9;
        if (!ok) a.status[s] = 1;
    }
}

__global__ void __launch_bounds__(kBvhBlock) k_bvh_motion(const BvhArgs a) {
    const BvhSeq sq = a.seq[blockIdx.y];
    const int i = blockIdx.x * kBvhBlock + threadIdx.x;                  // (F <= kBvhMaxFrames: checked on the host)
    if (i >= sq.F * kMotionSlots) return;
    const int f = i / kMotionSlots, c = i - f * kMotionSlots;
    const long long row = sq.row0 + f;
    float v[3];
    if (c == kSmplxJoints) {                                               // the root's position: (J_rest[0] + trans) x scale
        const float* rr = a.root_rest + 3 * sq.s;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        if (a.trans) { const float* t = a.trans + row * 3; t0 = t[0]; t1 = t[1]; t2 = t[2]; }
        v[0] = (rr[0] + t0) * a.scale; v[1] = (rr[1] + t1) * a.scale; v[2] = (rr[2] + t2) * a.scale;
        bvh_emit3(a, row, 0, v, sq.s);
        return;
    }
    const float* p = a.poses + (row * kSmplxJoints + a.dfs[c]) * 3;
    const Quat qu = aa_to_quat(p[0], p[1], p[2], 1e-3f);              // the series from 1e-3 down (its next term is below 2^-24 there): the bits the export was pinned with
    const float q[3] = {qu.x, qu.y, qu.z};
    bvh_euler(q, qu.w, a.ai, a.aj, a.ak, a.e, v);
    const int col = 3 + 3 * c;
    if (!a.unwrap) {
        bvh_emit3(a, row, col, v, sq.s);
    } else if (a.euler) {                                                // the walk's input: in the tap ...
        float* dst = a.euler + row * kBvhCols + col;
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
    } else {                                                             // ... or in the first dword of each number's own field
        float* dst = reinterpret_cast<float*>(a.text + row * kBvhRowBytes) + col * 3;
        dst[0] = v[0]; dst[3] = v[1]; dst[6] = v[2];
    }
}

// x moved by the multiple of 360 that brings it nearest to prev
__device__ __forceinline__ float bvh_near(float x, float prev) { return x + 360.0f * rintf((prev - x) / 360.0f); }

__global__ void __launch_bounds__(kBvhWalkBlock) k_bvh_walk(const BvhArgs a) {
    const int i = blockIdx.x * kBvhWalkBlock + threadIdx.x;
    if (i >= a.nseq * kSmplxJoints) return;
    const int k = i / kSmplxJoints, c = i - k * kSmplxJoints;
    const BvhSeq sq = a.seq[k];
    const int col = 3 + 3 * c;
    float prev[3] = {0.f, 0.f, 0.f};
    for (int f = 0; f < sq.F; ++f) {
        const long long row = sq.row0 + f;
        float p[3];
        if (a.euler) {
            const float* src = a.euler + row * kBvhCols + col;
            p[0] = src[0]; p[1] = src[1]; p[2] = src[2];
        } else {
            const float* src = reinterpret_cast<const float*>(a.text + row * kBvhRowBytes) + col * 3;
            p[0] = src[0]; p[1] = src[3]; p[2] = src[6];
        }
        float v[3] = {p[0], p[1], p[2]};
        if (f > 0) {
            // the same rotation twice: (alpha, beta, gamma) and (alpha + 180, 180 - beta, gamma + 180)
            const float a0 = bvh_near(p[0], prev[0]), a1 = bvh_near(p[1], prev[1]), a2 = bvh_near(p[2], prev[2]);
            const float b0 = bvh_near(p[0] + 180.0f, prev[0]), b1 = bvh_near(180.0f - p[1], prev[1]), b2 = bvh_near(p[2] + 180.0f, prev[2]);
            const float ca = fabsf(a0 - prev[0]) + fabsf(a1 - prev[1]) + fabsf(a2 - prev[2]);
            const float cb = fabsf(b0 - prev[0]) + fabsf(b1 - prev[1]) + fabsf(b2 - prev[2]);
            if (cb < ca) { v[0] = b0; v[1] = b1; v[2] = b2; } else { v[0] = a0; v[1] = a1; v[2] = a2; }
        }
        bvh_emit3(a, row, col, v, sq.s);
        prev[0] = v[0]; prev[1] = v[1]; prev[2] = v[2];
    }
}

__global__ void __launch_bounds__(kBvhBlock) k_bvh_decode(const BvhDecodeArgs a) {
    const BvhSeq sq = a.seq[blockIdx.y];
    const int i = blockIdx.x * kBvhBlock + threadIdx.x;
    if (i >= sq.F * kMotionSlots) return;
    const int f = i / kMotionSlots, c = i - f * kMotionSlots;
    const long long row = sq.row0 + f;
    const float* src = a.channels + row * kBvhCols;
    if (c == kSmplxJoints) {                                               // trans = position / scale - J_rest[0]
        const float* rr = a.root_rest + 3 * sq.s;
        float* dst = a.trans_out + row * 3;
        dst[0] = src[0] / a.scale - rr[0]; dst[1] = src[1] / a.scale - rr[1]; dst[2] = src[2] / a.scale - rr[2];
        return;
    }
    // q = q_ai(alpha) q_aj(beta) q_ak(gamma): each factor has one vector component
    float qw = 1.f, qv[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) {
        const float half = 0.5f * kRad * src[3 + 3 * c + k];
        const float cw = cosf(half), sv = sinf(half);
        const int axk = k == 0 ? a.ai : k == 1 ? a.aj : a.ak;
        const float r[3] = {axk == 0 ? sv : 0.f, axk == 1 ? sv : 0.f, axk == 2 ? sv : 0.f};
        const float nw = qw * cw - (qv[0] * r[0] + qv[1] * r[1] + qv[2] * r[2]);
        const float nx = qw * r[0] + cw * qv[0] + (qv[1] * r[2] - qv[2] * r[1]);
        const float ny = qw * r[1] + cw * qv[1] + (qv[2] * r[0] - qv[0] * r[2]);
        const float nz = qw * r[2] + cw * qv[2] + (qv[0] * r[1] - qv[1] * r[0]);
        qw = nw; qv[0] = nx; qv[1] = ny; qv[2] = nz;
    }
    // the decode tail's helper takes the first two ROWS of the rotation matrix (the 6D form) and ends in its quaternion -> axis-angle lines
    const float x = qv[0], y = qv[1], z = qv[2];
    const float d6[6] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - z * qw), 2.f * (x * z + y * qw),
                         2.f * (x * y + z * qw), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - x * qw)};
    float aa[3];
    rot6d_to_axis_angle(d6, 0, aa);
    // the helper does not standardise its quaternion's sign, so its angle lies in [0, 2 pi): the same rotation with angle <= pi
    const float n = sqrtf(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
    if (n > 3.14159265358979f) {
        const float g = (n - 6.283185307179586f) / n;
        aa[0] *= g; aa[1] *= g; aa[2] *= g;
    }
    float* dst = a.poses_out + (row * kSmplxJoints + a.dfs[c]) * 3;
    dst[0] = aa[0]; dst[1] = aa[1]; dst[2] = aa[2];
}

}  // namespace

hipError_t launch_bvh_format(const float* values, long long n, int per_row, unsigned char* text, int* status, hipStream_t stream) {
    const unsigned blocks = (unsigned)((n + kBvhBlock - 1) / kBvhBlock);
    hipLaunchKernelGGL(k_bvh_format, dim3(blocks), dim3(kBvhBlock), 0, stream, values, n, per_row, reinterpret_cast<unsigned*>(text), status);
    return hipGetLastError();
}

hipError_t launch_bvh_motion(const BvhArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)a.max_F * kMotionSlots + kBvhBlock - 1) / kBvhBlock), (unsigned)a.nseq);
    hipLaunchKernelGGL(k_bvh_motion, grid, dim3(kBvhBlock), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.unwrap) return e;
    hipLaunchKernelGGL(k_bvh_walk, dim3((unsigned)((a.nseq * kSmplxJoints + kBvhWalkBlock - 1) / kBvhWalkBlock)), dim3(kBvhWalkBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_bvh_decode(const BvhDecodeArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)a.max_F * kMotionSlots + kBvhBlock - 1) / kBvhBlock), (unsigned)a.nseq);
    hipLaunchKernelGGL(k_bvh_decode, grid, dim3(kBvhBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
