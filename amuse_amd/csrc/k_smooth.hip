// Motion smoothing (include/amuse_hip.h amuse_smooth_motion): a Savitzky-Golay filter over time, on SO(3) for the 55 joints and on R^3 for the translation.
// A workgroup takes a tile of kSmoothTile = 32 consecutive frames of ONE sequence (grid x: the tile, y: the sequence, its offsets in the kernel arguments):
//   1. it loads the tile and a halo of a.halo = max_j m_j frames on either side, clipped to the sequence (a sequence's last tile reaches back to the start of the end
//      window, L - 1 - 2 halo) - consecutive lanes read consecutive 12-byte triples of
//      the 165-float pose rows - and turns every (frame, joint) into a unit quaternion ONCE, into LDS; the translation rides along as (x, y, z, 0);
//   2. each lane then filters one (frame, slot) from LDS, 7 rounds of 256 lanes for a full tile: the 2 m + 1 relative rotations to the frame's own quaternion,
//      their logarithms weighted by the bank row, the exponential back.  ONE code path for interior and edge frames: the window start and the bank row are the
//      only things the frame's place in its sequence decides, and the sum runs k = 0 .. 2 m for all of them, so a frame's bits do not depend on where the tile
//      boundaries lie, nor on the launch or the batch.
// LDS layout: one 16-byte float4 per (row, slot), slot-major inside a row, rows back to back: [62][56] float4 = 55,552 B.  The lanes of a round hold
// consecutive (frame, slot) pairs, and lanes that share a half-window read, at step k, the float4s at their own index plus one constant: consecutive 16-byte
// slots, which ds_read_b128 / ds_write_b128 serve without bank conflicts (each 16-lane group covers one 256-byte bank row); only where m_j changes between
// neighbouring joints (body -> fingers) do the two parts of a wave read at different row offsets.  A structure of four float planes would take four reads for
// the same bytes.  55,552 B let two workgroups share a CU (2 waves per SIMD); the register bound of tests/test_smooth_isa_cpu.py keeps that.
// Bank rows are read through L2, not staged: the lanes of a frame that share m read the SAME row (one address per load, a broadcast), and every interior frame
// of the call reads row m of its H_m - a few hundred bytes that stay in the caches.
// No atomics, no double, no matrix-core instruction, no scratch.  The quaternion arithmetic is amuse_rot.hpp's; the tile stays float4 (.x = w, .y .z .w = the
// vector part) and is converted where it is stored and loaded.
#include "amuse_rot.hpp"
#include "amuse_smooth_host.hpp"

namespace amuse {

namespace {

__device__ __forceinline__ Quat tile_quat(const float4 v) { return Quat{v.x, v.y, v.z, v.w}; }

// one joint of one frame: qc the frame's own quaternion, win the first float4 of its window (stride kMotionSlots), h the bank row, n = 2 m + 1
__device__ __forceinline__ void smooth_joint(const Quat qc, const float4* win, const float* __restrict__ h, int n, float (&out)[3]) {
    float vx = 0.f, vy = 0.f, vz = 0.f;
    for (int k = 0; k < n; ++k) {
        const Quat d = quat_conj_mul(qc, tile_quat(win[k * kMotionSlots]));
        float dw = d.w, dx = d.x, dy = d.y, dz = d.z;
        if (dw < 0.f) { dw = -dw; dx = -dx; dy = -dy; dz = -dz; }          // the shorter arc
        const float nv = sqrtf(dx * dx + dy * dy + dz * dz);
        const float fac = (nv < 1e-6f) ? 2.0f : (2.0f * atan2f(nv, dw)) / nv;
        const float w = h[k] * fac;
        vx += w * dx; vy += w * dy; vz += w * dz;
    }
    const Quat e = aa_to_quat(vx, vy, vz);
    // qc e, written out: behind a helper the compiler sums qz's first two products the other way round, the FMA takes the other one and the bits move
    const float qw = qc.w * e.w - qc.x * e.x - qc.y * e.y - qc.z * e.z;
    const float qx = qc.w * e.x + qc.x * e.w + qc.y * e.z - qc.z * e.y;
    const float qy = qc.w * e.y - qc.x * e.z + qc.y * e.w + qc.z * e.x;
    const float qz = qc.w * e.z + qc.x * e.y - qc.y * e.x + qc.z * e.w;
    quat_to_aa(quat_unit_short(Quat{qw, qx, qy, qz}), out);                // smoothed frames carry the short representation
}

__global__ void __launch_bounds__(kSmoothBlock) k_smooth(const SmoothArgs a) {
    __shared__ float4 s_q[kSmoothLdsRows * kMotionSlots];
    const SmoothSeq sq = a.seq[blockIdx.y];
    const int t0 = blockIdx.x * kSmoothTile;
    if (t0 >= sq.L) return;                                    // (uniform: the grid's x covers the launch's longest sequence)
    const bool has_trans = a.trans != nullptr;
    // rows [lo, hi) of the sequence, at most kSmoothLdsRows of them.  A window start is clamp(f - m, 0, L - 1 - 2 m): in a sequence's last tile it can lie up to
    // 2 m before the frame, so the low side reaches back to L - 1 - 2 halo there (hi is L then: 2 halo + 1 rows or fewer more than the plain halo would load)
    int lo = t0 - a.halo < sq.L - 1 - 2 * a.halo ? t0 - a.halo : sq.L - 1 - 2 * a.halo;
    if (lo < 0) lo = 0;
    const int hi = t0 + kSmoothTile + a.halo < sq.L ? t0 + kSmoothTile + a.halo : sq.L;
    const int nt = sq.L - t0 < kSmoothTile ? sq.L - t0 : kSmoothTile;
    const size_t row_lo = (size_t)sq.row0 + lo;
    const float* __restrict__ src = a.poses + row_lo * (kSmplxJoints * 3);
    for (int i = threadIdx.x; i < (hi - lo) * kMotionSlots; i += kSmoothBlock) {
        const int row = i / kMotionSlots, j = i - row * kMotionSlots;
        if (j < kSmplxJoints) {
            const float* p = src + (row * kSmplxJoints + j) * 3;
            const Quat q = aa_to_quat(p[0], p[1], p[2]);
            s_q[i] = make_float4(q.w, q.x, q.y, q.z);
        } else if (has_trans) {
            const float* p = a.trans + (row_lo + row) * 3;
            s_q[i] = make_float4(p[0], p[1], p[2], 0.f);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nt * kMotionSlots; i += kSmoothBlock) {
        const int fl = i / kMotionSlots, j = i - fl * kMotionSlots;
        const bool is_trans = j == kSmplxJoints;
        if (is_trans && !has_trans) continue;
        const int f = t0 + fl, m = a.hw[j], n = 2 * m + 1;
        const size_t row_o = (size_t)sq.row0 + f;
        float* dst = is_trans ? a.trans_out + row_o * 3 : a.poses_out + (row_o * kSmplxJoints + j) * 3;
        if (m == 0 || sq.L < n) {                               // not filtered: the input's bits
            const float* p = is_trans ? a.trans + row_o * 3 : a.poses + (row_o * kSmplxJoints + j) * 3;
            const float b0 = p[0], b1 = p[1], b2 = p[2];
            dst[0] = b0; dst[1] = b1; dst[2] = b2;
            continue;
        }
        int s = f - m;
        if (s > sq.L - n) s = sq.L - n;
        if (s < 0) s = 0;
        const int r = f - s;                                    // the frame's place in its window: m in the interior, 0 .. 2 m at the two ends
        const float* __restrict__ h = a.banks + smooth_bank_offset(m) + r * n;
        const float4* win = s_q + (s - lo) * kMotionSlots + j;  // s >= min(t0 - m, L - 1 - 2 m) >= lo and s + 2 m <= max(min(f + m, L - 1), 2 m) < hi: inside the loaded rows
        if (is_trans) {
            float x = 0.f, y = 0.f, z = 0.f;
            for (int k = 0; k < n; ++k) {
                const float4 v = win[k * kMotionSlots];
                x += h[k] * v.x; y += h[k] * v.y; z += h[k] * v.z;
            }
            dst[0] = x; dst[1] = y; dst[2] = z;
            continue;
        }
        float o[3];
        smooth_joint(tile_quat(s_q[(f - lo) * kMotionSlots + j]), win, h, n, o);
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    }
}

}  // namespace

hipError_t launch_smooth(const SmoothArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.max_L + kSmoothTile - 1) / kSmoothTile), (unsigned)a.nseq);
    hipLaunchKernelGGL(k_smooth, grid, dim3(kSmoothBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
