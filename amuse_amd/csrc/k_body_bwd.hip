// Backward pass of SMPL-X linear blend skinning on gfx950 (amuse_body_vertex_loss_grad; host side amuse_body_grad.hip, layouts amuse_body_pack.hpp).
// The gradient of S = sum SmoothL1(x_cand - x_ref) with respect to the candidate's 6D feature rows, in two launches per candidate.
//
// k_body_skin_bwd, 8 waves per workgroup = one 16-frame tile x a chunk of vertex-group PAIRS, the reference and ONE candidate: a wave recomputes the pose-blend
//   product of two consecutive vertex groups for both sets exactly as k_body_skin does (same fragments, same order of the split products), skins them in-lane and
//   forms g = clamp(x_cand - x_ref, -1, 1) (0 for pad vertices, pad frames, skipped clips).  No vertex is written.  Then, per lane = (vertex, frame):
//     * translation: g accumulates in the lane (fp32, the wave's vertices in fixed order) and joins the fixed-point sums below once at the end;
//     * dA_j += w_vj [g p^T | g]: the fp32 products go, as round(value x 2^38), into int64 sums in LDS ([16 frames][664], ds_add_u64).  Integer addition commutes,
//       so the sums do not depend on the order in which waves and lanes arrive: DETERMINISTIC without an owner thread or a second pass over the vertices.
//       Capacity 2^25 per sum (|w g p| <= |p|, 10,475 vertices: body-local coordinates up to 3,000 m), resolution 3.6e-12 per addend.
//     * dp = T.R^T g, scaled by 2^10 and cut into fp16 hi | lo: the accumulator layout of the forward product (rows 4 (lane >> 4) + r at column lane & 15) makes
//       the two groups' (x, y, z, pad) x 2 the lane's B fragment of v_mfma_f32_16x16x32_f16 as it stands (k = 8 (lane >> 4) + i: vertex-in-group, group parity,
//       coordinate) - no LDS round trip.  The A operand is the transposed posedirs image (512 feature rows x the pair's 32 k), 32 feature tiles per pair:
//       dpf[feature][frame] += Ptl.dh + Pth.dl + Pth.dh, small terms first, accumulated over the whole chunk in 32 x 4 accumulator registers per lane.
//   At the end the eight waves' dpf accumulators are added in wave order through LDS (the dead feature planes) and leave as one fp32 partial per workgroup, with
//   the fixed-point sums converted to fp32.  Cost of the determinism: 12 x nnz 64-bit LDS atomics per (vertex, frame) and 42 + 32 KiB of partials per workgroup.
//   Budget: LDS 64 KiB feature planes (2 sets x hi | lo; 32 KiB one-product) + 83 KiB fixed-point sums = 147 KiB (115 KiB) of 160: one workgroup per CU, which is
//   also what 512 threads x (128 dpf accumulators + the forward's fragments and accumulators, within 256 registers) allow.  One candidate per pass: a second
//   candidate's 128 accumulators do not fit.  Matrix-core instructions: 16 k-steps x 2 groups x 2 sets x (3 | 1) forward + 32 feature tiles x (3 | 1) transposed
//   = 288 split, 96 one-product, all unrolled.
// k_body_pose_bwd, one 64-lane workgroup per frame: adds the chunk partials in index order in double; dG_j = [dA_j.R - dA_j.t J_j^T | dA_j.t]; walks the chain
//   from joint 54 down (parents[j] < j), twelve lanes per step, with R_j recomputed from the row and G_parent.R read from the A the forward pose kernel left;
//   adds dpf to dR_1..54; Gram-Schmidt backward (the max(norm, 1e-12) clamps pass no gradient to a clamped norm); writes scale x the row.  All in double: a few
//   thousand flops per frame.  Frames of skipped clips are left untouched.
#include "amuse_body_bwd.hpp"
#include "amuse_body.hpp"
#include "amuse_dev.hpp"
#include "amuse_kernels.hpp"   // DeviceOnce

namespace amuse {
namespace {

struct SkinPair { int joint; float weight; };

__device__ __forceinline__ void fix_add(long long* p, float v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__float2ll_rn(v * (float)(1ll << kBodyFixShift)));
}

template <bool SPLIT>
__global__ __launch_bounds__(512) void k_body_skin_bwd(BodySkinBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PLANES = SPLIT ? 2 : 1;
    constexpr int PLANE_U4 = 16 * 64;   // uint4 per plane of a frame tile
    uint4* lds = reinterpret_cast<uint4*>(smem);                                                   // [2 sets][PLANES][16 k-steps][64 lanes]
    long long* fix = reinterpret_cast<long long*>(smem + (size_t)2 * PLANES * PLANE_U4 * 16);    // [16 frames][kBodyDAStride]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const int f = lane & 15, g = lane >> 4;
    const int fr = tile * 16 + f;
    const int sub = fr < a.nframes ? a.subject[fr / a.F] : -1;
    const bool valid = sub >= 0 && sub < a.n_subjects;
    if (!__syncthreads_or(valid)) return;   // no frame of this tile is read by k_body_pose_bwd (uniform)
    for (int i = t; i < 16 * kBodyDAStride; i += 512) fix[i] = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int p = 0; p < PLANES; ++p) {
            const uint4* src = reinterpret_cast<const uint4*>(p ? a.pf_lo[s] : a.pf_hi[s]) + (size_t)tile * PLANE_U4;
#pragma unroll
            for (int i = 0; i < PLANE_U4 / 512; ++i) lds[(s * PLANES + p) * PLANE_U4 + i * 512 + t] = src[i * 512 + t];
        }
    __syncthreads();
    const float* vs = a.v_shaped + (size_t)(valid ? sub : 0) * a.groups * 16;
    f32x4 trs[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) trs[s] = valid ? ld4(a.tr[s] + (size_t)fr * 4) : splat4(0.f);
    const int per = (a.pairs + a.chunks - 1) / a.chunks;
    const int q0 = chunk * per, q1 = q0 + per < a.pairs ? q0 + per : a.pairs;
    f32x4 dacc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) dacc[i] = splat4(0.f);
    float tgx = 0.f, tgy = 0.f, tgz = 0.f;
    long long* fixf = fix + f * kBodyDAStride;
    for (int q = q0 + wave; q < q1; q += 8) {
        // ---- the forward product of groups 2q, 2q + 1 (the second may lie past the last group of an odd count: its in-bounds stand-in is computed and dropped)
        f32x4 acc[2][2];
        int vgc[2];
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            vgc[gi] = 2 * q + gi < a.groups ? 2 * q + gi : a.groups - 1;
            acc[gi][0] = splat4(0.f);
            acc[gi][1] = splat4(0.f);
        }
#pragma unroll
        for (int k4 = 0; k4 < 16; k4 += 4) {
            uint4 ah[2][4], al[2][4];
#pragma unroll
            for (int gi = 0; gi < 2; ++gi)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ah[gi][i] = (reinterpret_cast<const uint4*>(a.pd_hi) + (size_t)vgc[gi] * PLANE_U4 + lane)[(k4 + i) * 64];
                    if constexpr (SPLIT) al[gi][i] = (reinterpret_cast<const uint4*>(a.pd_lo) + (size_t)vgc[gi] * PLANE_U4 + lane)[(k4 + i) * 64];
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int ks = k4 + i;
                    const f16x8 bh = __builtin_bit_cast(f16x8, lds[(s * PLANES) * PLANE_U4 + ks * 64 + lane]);
#pragma unroll
                    for (int gi = 0; gi < 2; ++gi) {
                        if constexpr (SPLIT) {
                            const f16x8 bl = __builtin_bit_cast(f16x8, lds[(s * PLANES + 1) * PLANE_U4 + ks * 64 + lane]);
                            acc[gi][s] = mfma_f16(__builtin_bit_cast(f16x8, al[gi][i]), bh, acc[gi][s]);
                            acc[gi][s] = mfma_f16(__builtin_bit_cast(f16x8, ah[gi][i]), bl, acc[gi][s]);
                        }
                        acc[gi][s] = mfma_f16(__builtin_bit_cast(f16x8, ah[gi][i]), bh, acc[gi][s]);
                    }
                }
        }
        // ---- skinning of both sets, g, the three gradients
        float dp[2][3];
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int v = vgc[gi] * 4 + g;
            const bool live = valid && 2 * q + gi < a.groups && v < a.V;
            const f32x4 v0 = ld4(vs + (size_t)v * 4);
            const SkinPair* list = reinterpret_cast<const SkinPair*>(a.skin) + (size_t)v * a.nnz;
            float out[2][3], px = 0.f, py = 0.f, pz = 0.f;
            f32x4 T0, T1, T2;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                px = v0[0] + acc[gi][s][0] * a.scale_inv; py = v0[1] + acc[gi][s][1] * a.scale_inv; pz = v0[2] + acc[gi][s][2] * a.scale_inv;
                T0 = splat4(0.f); T1 = splat4(0.f); T2 = splat4(0.f);
                const float* As = a.A[s] + (size_t)fr * kBodyAFloats;
                for (int i = 0; i < a.nnz; ++i) {
                    const SkinPair e = list[i];
                    if (!__any(e.weight != 0.f)) break;
                    if (valid && e.weight != 0.f) {
                        const float* Aj = As + e.joint * 12;
                        T0 += e.weight * ld4(Aj);
                        T1 += e.weight * ld4(Aj + 4);
                        T2 += e.weight * ld4(Aj + 8);
                    }
                }
                out[s][0] = T0[0] * px + T0[1] * py + T0[2] * pz + T0[3] + trs[s][0];
                out[s][1] = T1[0] * px + T1[1] * py + T1[2] * pz + T1[3] + trs[s][1];
                out[s][2] = T2[0] * px + T2[1] * py + T2[2] * pz + T2[3] + trs[s][2];
            }
            // (px, py, pz) and T are the candidate's from here on
            float gx = 0.f, gy = 0.f, gz = 0.f;
            if (live) {
                gx = fminf(fmaxf(out[1][0] - out[0][0], -1.f), 1.f);
                gy = fminf(fmaxf(out[1][1] - out[0][1], -1.f), 1.f);
                gz = fminf(fmaxf(out[1][2] - out[0][2], -1.f), 1.f);
            }
            tgx += gx; tgy += gy; tgz += gz;
            dp[gi][0] = T0[0] * gx + T1[0] * gy + T2[0] * gz;
            dp[gi][1] = T0[1] * gx + T1[1] * gy + T2[1] * gz;
            dp[gi][2] = T0[2] * gx + T1[2] * gy + T2[2] * gz;
            for (int i = 0; i < a.nnz; ++i) {
                const SkinPair e = list[i];
                if (!__any(e.weight != 0.f)) break;
                if (live && e.weight != 0.f) {
                    long long* o = fixf + e.joint * 12;
                    const float wx = e.weight * gx, wy = e.weight * gy, wz = e.weight * gz;
                    fix_add(o + 0, wx * px); fix_add(o + 1, wx * py); fix_add(o + 2, wx * pz);  fix_add(o + 3, wx);
                    fix_add(o + 4, wy * px); fix_add(o + 5, wy * py); fix_add(o + 6, wy * pz);  fix_add(o + 7, wy);
                    fix_add(o + 8, wz * px); fix_add(o + 9, wz * py); fix_add(o + 10, wz * pz); fix_add(o + 11, wz);
                }
            }
        }
        // ---- the transposed product: this lane's dp of the two groups IS its B fragment
        constexpr float DPS = (float)(1 << kBodyDpShift);
        f16x8 bh, bl;
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = dp[gi][c] * DPS;
                const _Float16 h = (_Float16)x;
                bh[gi * 4 + c] = h;
                bl[gi * 4 + c] = (_Float16)(x - (float)h);
            }
            bh[gi * 4 + 3] = (_Float16)0.f;
            bl[gi * 4 + 3] = (_Float16)0.f;
        }
        const uint4* th = reinterpret_cast<const uint4*>(a.pt_hi) + (size_t)q * (32 * 64) + lane;
        const uint4* tl = reinterpret_cast<const uint4*>(a.pt_lo) + (size_t)q * (32 * 64) + lane;
#pragma unroll
        for (int f8 = 0; f8 < 32; f8 += 8) {
            uint4 ph[8], pl[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                ph[i] = th[(f8 + i) * 64];
                if constexpr (SPLIT) pl[i] = tl[(f8 + i) * 64];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if constexpr (SPLIT) {
                    dacc[f8 + i] = mfma_f16(__builtin_bit_cast(f16x8, pl[i]), bh, dacc[f8 + i]);
                    dacc[f8 + i] = mfma_f16(__builtin_bit_cast(f16x8, ph[i]), bl, dacc[f8 + i]);
                }
                dacc[f8 + i] = mfma_f16(__builtin_bit_cast(f16x8, ph[i]), bh, dacc[f8 + i]);
            }
        }
    }
    fix_add(fixf + 660, tgx);
    fix_add(fixf + 661, tgy);
    fix_add(fixf + 662, tgz);
    __syncthreads();   // every sum is complete, the feature planes are dead
    // the eight waves' dpf accumulators, added in wave order in the planes' first 32 KiB
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    for (int w = 0; w < 8; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 32; ++i) red[i * 64 + lane] = w == 0 ? dacc[i] : red[i * 64 + lane] + dacc[i];
        }
        __syncthreads();
    }
    const size_t wg = (size_t)tile * a.chunks + chunk;
    float* op = a.dpf_part + wg * kBodyDpfFloats;
    for (int i = t; i < kBodyDpfFloats / 4; i += 512) st4(op + (size_t)i * 4, red[i]);
    float* oa = a.dA_part + wg * (16 * kBodyDAStride);
    for (int i = t; i < 16 * kBodyDAStride; i += 512) oa[i] = (float)((double)fix[i] * (1.0 / (double)(1ll << kBodyFixShift)));
}

__global__ __launch_bounds__(64) void k_body_pose_bwd(BodyPoseBwdArgs a) {
    __shared__ double R[55][9];
    __shared__ double dR[55][9];
    __shared__ double dG[55][12];
    const int fr = blockIdx.x, lane = threadIdx.x;
    const int sub = a.subject[fr / a.F];
    if (sub < 0 || sub >= a.n_subjects) return;   // a skipped clip: its rows stay as they are
    const int tile = fr >> 4, col = fr & 15;
    const float* row = a.rows + (size_t)fr * 333;
    const float* J = a.J + (size_t)sub * 55 * 4;
    const size_t wg0 = (size_t)tile * a.chunks;
    // Gram-Schmidt forward, kept for the way back
    double a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0}, b1[3] = {0, 0, 0}, b2[3] = {0, 0, 0}, n1r = 0, n1 = 1, n2r = 0, n2 = 1, dt = 0;
    if (lane < 55) {
        for (int c = 0; c < 3; ++c) { a1[c] = (double)row[lane * 6 + c]; a2[c] = (double)row[lane * 6 + 3 + c]; }
        n1r = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
        n1 = fmax(n1r, 1e-12);
        for (int c = 0; c < 3; ++c) b1[c] = a1[c] / n1;
        dt = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
        double u[3];
        for (int c = 0; c < 3; ++c) u[c] = a2[c] - dt * b1[c];
        n2r = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        n2 = fmax(n2r, 1e-12);
        for (int c = 0; c < 3; ++c) b2[c] = u[c] / n2;
        for (int c = 0; c < 3; ++c) { R[lane][c] = b1[c]; R[lane][3 + c] = b2[c]; }
        R[lane][6] = b1[1] * b2[2] - b1[2] * b2[1];
        R[lane][7] = b1[2] * b2[0] - b1[0] * b2[2];
        R[lane][8] = b1[0] * b2[1] - b1[1] * b2[0];
        // dA of this joint: the chunks in index order
        double s[12];
        for (int e = 0; e < 12; ++e) s[e] = 0.0;
        for (int c = 0; c < a.chunks; ++c) {
            const float* p = a.dA_part + ((wg0 + c) * 16 + col) * kBodyDAStride + lane * 12;
            for (int e = 0; e < 12; ++e) s[e] += (double)p[e];
        }
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) dG[lane][r * 4 + c] = s[r * 4 + c] - s[r * 4 + 3] * (double)J[lane * 4 + c];
            dG[lane][r * 4 + 3] = s[r * 4 + 3];
        }
        if (lane == 0)
            for (int e = 0; e < 9; ++e) dR[0][e] = 0.0;
    } else if (lane < 58) {
        double s = 0.0;
        for (int c = 0; c < a.chunks; ++c) s += (double)a.dA_part[((wg0 + c) * 16 + col) * kBodyDAStride + 660 + (lane - 55)];
        a.grad[(size_t)fr * 333 + 330 + (lane - 55)] = (float)((double)a.scale * s);
    }
    for (int k = lane; k < 486; k += 64) {
        const size_t i = (size_t)(k >> 4) * 256 + (size_t)(((k >> 2) & 3) * 16 + col) * 4 + (k & 3);
        double s = 0.0;
        for (int c = 0; c < a.chunks; ++c) s += (double)a.dpf_part[(wg0 + c) * kBodyDpfFloats + i];
        dR[1 + k / 9][k % 9] = s * (double)a.dpf_scale;
    }
    __syncthreads();
    // the chain in reverse: lane e < 12 owns element (r, c) of dG_parent and, for c < 3, of dR_j
    const int r = lane >> 2, c = lane & 3;
    const float* Af = a.A + (size_t)fr * kBodyAFloats;
    for (int j = 54; j >= 1; --j) {
        const int p = a.parents[j];
        if (lane < 12) {
            if (c < 3) {
                const float* Ap = Af + p * 12;   // G_p.R
                dR[j][r * 3 + c] += (double)Ap[r] * dG[j][c] + (double)Ap[4 + r] * dG[j][4 + c] + (double)Ap[8 + r] * dG[j][8 + c];
                const double l = (double)J[j * 4 + c] - (double)J[p * 4 + c];
                dG[p][r * 4 + c] += dG[j][r * 4] * R[j][c * 3] + dG[j][r * 4 + 1] * R[j][c * 3 + 1] + dG[j][r * 4 + 2] * R[j][c * 3 + 2] + dG[j][r * 4 + 3] * l;
            } else {
                dG[p][r * 4 + 3] += dG[j][r * 4 + 3];
            }
        }
        __syncthreads();
    }
    if (lane < 12 && c < 3) dR[0][r * 3 + c] += dG[0][r * 4 + c];
    __syncthreads();
    if (lane < 55) {
        double d1[3], d2[3], d3[3];
        for (int e = 0; e < 3; ++e) { d1[e] = dR[lane][e]; d2[e] = dR[lane][3 + e]; d3[e] = dR[lane][6 + e]; }
        // b3 = b1 x b2
        d1[0] += b2[1] * d3[2] - b2[2] * d3[1]; d1[1] += b2[2] * d3[0] - b2[0] * d3[2]; d1[2] += b2[0] * d3[1] - b2[1] * d3[0];
        d2[0] += d3[1] * b1[2] - d3[2] * b1[1]; d2[1] += d3[2] * b1[0] - d3[0] * b1[2]; d2[2] += d3[0] * b1[1] - d3[1] * b1[0];
        // b2 = u / max(|u|, 1e-12)
        double du[3];
        const double k2 = n2r >= 1e-12 ? (b2[0] * d2[0] + b2[1] * d2[1] + b2[2] * d2[2]) : 0.0;
        for (int e = 0; e < 3; ++e) du[e] = (d2[e] - b2[e] * k2) / n2;
        // u = a2 - (b1 . a2) b1
        const double ddt = -(b1[0] * du[0] + b1[1] * du[1] + b1[2] * du[2]);
        double g2[3];
        for (int e = 0; e < 3; ++e) { g2[e] = du[e] + ddt * b1[e]; d1[e] += -dt * du[e] + ddt * a2[e]; }
        // b1 = a1 / max(|a1|, 1e-12)
        const double k1 = n1r >= 1e-12 ? (b1[0] * d1[0] + b1[1] * d1[1] + b1[2] * d1[2]) : 0.0;
        float* o = a.grad + (size_t)fr * 333 + lane * 6;
        for (int e = 0; e < 3; ++e) {
            o[e] = (float)((double)a.scale * (d1[e] - b1[e] * k1) / n1);
            o[3 + e] = (float)((double)a.scale * g2[e]);
        }
    }
}

template <bool SPLIT>
hipError_t launch_skin_bwd_t(const BodySkinBwdArgs& a, hipStream_t st) {
    constexpr int lds = 2 * (SPLIT ? 2 : 1) * 16 * 1024 + 16 * kBodyDAStride * 8;
    static DeviceOnce once;
    int dev_;
    if (!once.done(&dev_)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_body_skin_bwd<SPLIT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        once.set(dev_);
    }
    const int tiles = (a.nframes + 15) / 16;
    hipLaunchKernelGGL((k_body_skin_bwd<SPLIT>), dim3(tiles, a.chunks), dim3(512), lds, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_body_skin_bwd(const BodySkinBwdArgs& a, int split, hipStream_t st) {
    return split ? launch_skin_bwd_t<true>(a, st) : launch_skin_bwd_t<false>(a, st);
}

hipError_t launch_body_pose_bwd(const BodyPoseBwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_body_pose_bwd, dim3(a.nframes), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace amuse
