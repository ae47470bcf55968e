// SMPL-X linear blend skinning on gfx950 (amuse_body_forward / amuse_body_vertex_loss; host side amuse_body.hip, layouts amuse_body_pack.hpp).
//
// k_body_pose, one 64-lane workgroup per frame: lane j < 55 turns joint j's axis-angle (Rodrigues with the published package's angle = |r + 1e-8|) or 6D vector
//   (Gram-Schmidt of rotation_6d_to_matrix) into R_j; the 486 pose features (R_1..R_54 - I), padded to 512, leave as fp16 hi | lo planes in the fragment order of
//   the MFMA's B operand; twelve lanes walk the kinematic chain (55 dependent 3x4 compositions through LDS); lanes j write A_j = [G_j.R | G_j.t - G_j.R J_j]
//   and the posed joints.  Frames of the last, ragged 16-frame tile get zero features.
// k_body_skin, 8 waves per workgroup = one 16-frame tile x a chunk of vertex groups, all motion sets of the call at once: the tile's pose-feature planes sit in
//   LDS (32 KiB per set split, 16 KiB one-product); a wave streams one vertex group's posedirs fragments (16 k-steps x hi | lo) into registers and multiplies them
//   with every set's features - Pl.fh + Ph.fl + Ph.fh on v_mfma_f32_16x16x32_f16, small terms first - so that a lane's accumulator IS vertex (4 group + lane / 16)'s
//   offset at frame (lane & 15).  Skinning runs in-lane over the vertex's (joint, weight) list: T = sum w A_j in the reference's order of operations
//   (blend first, then apply), vertex = T . [v_posed; 1] + transl.  Forward mode stores the vertices; loss mode never does - reference and candidates of a vertex
//   meet in registers, SmoothL1 accumulates per lane in fp32, one fp32 partial pair per workgroup, and k_body_loss_reduce adds the partials in index order in double.
#include "amuse_body.hpp"
#include "amuse_dev.hpp"
#include "amuse_kernels.hpp"   // DeviceOnce

namespace amuse {
namespace {

__device__ __forceinline__ void split_store(uint16_t* hi, uint16_t* lo, size_t i, float v) {
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    hi[i] = __builtin_bit_cast(unsigned short, h);
    lo[i] = __builtin_bit_cast(unsigned short, l);
}

__global__ __launch_bounds__(64) void k_body_pose(BodyPoseArgs a) {
    __shared__ float R[55][9];
    __shared__ float G[55][12];
    const int fr = blockIdx.x, lane = threadIdx.x;
    const size_t pf_base = (size_t)(fr >> 4) * (16 * 64 * 8);
    const int col = fr & 15;
    const int sub = fr < a.nframes ? a.subject[fr / a.F] : -1;
    if (sub < 0 || sub >= a.n_subjects) {   // pad frame of the last tile, or a clip that is skipped (subject outside 0..S-1): zero features, nothing else
        for (int k = lane; k < 512; k += 64) {
            const size_t i = pf_base + ((size_t)(k >> 5) * 64 + ((k >> 3) & 3) * 16 + col) * 8 + (k & 7);
            a.pf_hi[i] = 0;
            a.pf_lo[i] = 0;
        }
        return;
    }
    const float* row = a.rot + (size_t)fr * a.rot_stride;
    if (lane < 55) {
        float m[9];
        if (a.rot_kind == 0) {
            const float x = row[lane * 3], y = row[lane * 3 + 1], z = row[lane * 3 + 2];
            const float xe = x + 1e-8f, ye = y + 1e-8f, ze = z + 1e-8f;
            const float ang = sqrtf(xe * xe + ye * ye + ze * ze);
            const float rx = x / ang, ry = y / ang, rz = z / ang;
            const float s = sinf(ang), c1 = 1.f - cosf(ang);
            // I + sin K + (1 - cos) K^2, K = skew(rot_dir)
            m[0] = 1.f + c1 * (-(ry * ry) - rz * rz); m[1] = -s * rz + c1 * (rx * ry);          m[2] = s * ry + c1 * (rx * rz);
            m[3] = s * rz + c1 * (rx * ry);           m[4] = 1.f + c1 * (-(rx * rx) - rz * rz); m[5] = -s * rx + c1 * (ry * rz);
            m[6] = -s * ry + c1 * (rx * rz);          m[7] = s * rx + c1 * (ry * rz);           m[8] = 1.f + c1 * (-(rx * rx) - ry * ry);
        } else {
            const float* d6 = row + lane * 6;
            const float a1x = d6[0], a1y = d6[1], a1z = d6[2], a2x = d6[3], a2y = d6[4], a2z = d6[5];
            const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
            const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
            const float dt = b1x * a2x + b1y * a2y + b1z * a2z;
            float b2x = a2x - dt * b1x, b2y = a2y - dt * b1y, b2z = a2z - dt * b1z;
            const float n2 = fmaxf(sqrtf(b2x * b2x + b2y * b2y + b2z * b2z), 1e-12f);
            b2x /= n2; b2y /= n2; b2z /= n2;
            m[0] = b1x; m[1] = b1y; m[2] = b1z; m[3] = b2x; m[4] = b2y; m[5] = b2z;
            m[6] = b1y * b2z - b1z * b2y; m[7] = b1z * b2x - b1x * b2z; m[8] = b1x * b2y - b1y * b2x;
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) R[lane][e] = m[e];
    }
    __syncthreads();
    for (int k = lane; k < 512; k += 64) {
        float v = 0.f;
        if (k < 486) {
            const int e = k % 9;
            v = R[1 + k / 9][e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
        }
        split_store(a.pf_hi, a.pf_lo, pf_base + ((size_t)(k >> 5) * 64 + ((k >> 3) & 3) * 16 + col) * 8 + (k & 7), v);
    }
    // the chain: lane e < 12 owns element (r, c) of every G_j = G_parent . [R_j | J_j - J_parent]
    const float* J = a.J + (size_t)sub * 55 * 4;
    const int r = lane >> 2, c = lane & 3;
    for (int j = 0; j < 55; ++j) {
        const int p = a.parents[j];
        if (lane < 12) {
            float l0, l1, l2;   // column c of the local transform
            if (c < 3) { l0 = R[j][c]; l1 = R[j][3 + c]; l2 = R[j][6 + c]; }
            else if (p < 0) { l0 = J[j * 4]; l1 = J[j * 4 + 1]; l2 = J[j * 4 + 2]; }
            else { l0 = J[j * 4] - J[p * 4]; l1 = J[j * 4 + 1] - J[p * 4 + 1]; l2 = J[j * 4 + 2] - J[p * 4 + 2]; }
            float v;
            if (p < 0) v = r == 0 ? l0 : r == 1 ? l1 : l2;
            else {
                v = G[p][r * 4] * l0 + G[p][r * 4 + 1] * l1 + G[p][r * 4 + 2] * l2;
                if (c == 3) v += G[p][r * 4 + 3];
            }
            G[j][lane] = v;
        }
        __syncthreads();
    }
    const float* tp = a.trans ? a.trans + (size_t)fr * a.trans_stride : nullptr;
    const float tx = tp ? tp[0] : 0.f, ty = tp ? tp[1] : 0.f, tz = tp ? tp[2] : 0.f;
    if (lane == 0) st4(a.tr + (size_t)fr * 4, f32x4{tx, ty, tz, 0.f});
    if (lane < 55) {
        const float jx = J[lane * 4], jy = J[lane * 4 + 1], jz = J[lane * 4 + 2];
        float* o = a.A + ((size_t)fr * 55 + lane) * 12;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float g0 = G[lane][q * 4], g1 = G[lane][q * 4 + 1], g2 = G[lane][q * 4 + 2], g3 = G[lane][q * 4 + 3];
            st4(o + q * 4, f32x4{g0, g1, g2, g3 - (g0 * jx + g1 * jy + g2 * jz)});
        }
        if (a.joints_out) {
            float* jo = a.joints_out + ((size_t)fr * 55 + lane) * 3;
            jo[0] = G[lane][3] + tx; jo[1] = G[lane][7] + ty; jo[2] = G[lane][11] + tz;
        }
    }
}

__device__ __forceinline__ float smooth_l1(float d) {
    const float a = fabsf(d);
    return a < 1.f ? 0.5f * a * a : a - 0.5f;
}

struct SkinPair { int joint; float weight; };

template <int NSET, bool SPLIT, bool LOSS>
__global__ __launch_bounds__(512) void k_body_skin(BodySkinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PLANES = SPLIT ? 2 : 1;
    constexpr int PLANE_U4 = 16 * 64;   // uint4 per plane of a frame tile
    uint4* lds = reinterpret_cast<uint4*>(smem);   // [NSET][PLANES][16 k-steps][64 lanes]
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const int f = lane & 15, g = lane >> 4;
    const int fr = tile * 16 + f;
    const int sub = fr < a.nframes ? a.subject[fr / a.F] : -1;
    const bool valid = sub >= 0 && sub < a.n_subjects;   // not a pad frame, not a skipped clip
    if (!__syncthreads_or(valid)) {                      // nothing to do in this tile (uniform)
        if (LOSS && t == 0) {
            float* o = a.partials + ((size_t)tile * a.chunks + chunk) * 2;
            o[0] = 0.f;
            o[1] = 0.f;
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < NSET; ++s)
#pragma unroll
        for (int p = 0; p < PLANES; ++p) {
            const uint4* src = reinterpret_cast<const uint4*>(p ? a.pf_lo[s] : a.pf_hi[s]) + (size_t)tile * PLANE_U4;
#pragma unroll
            for (int i = 0; i < PLANE_U4 / 512; ++i) lds[(s * PLANES + p) * PLANE_U4 + i * 512 + t] = src[i * 512 + t];
        }
    __syncthreads();
    // lanes of pad frames and skipped clips compute on zeros (their transforms are never read) and store nothing
    const float* vs = a.v_shaped + (size_t)(valid ? sub : 0) * a.groups * 16;
    f32x4 trs[NSET];
#pragma unroll
    for (int s = 0; s < NSET; ++s) trs[s] = valid ? ld4(a.tr[s] + (size_t)fr * 4) : splat4(0.f);
    const int per = (a.groups + a.chunks - 1) / a.chunks;
    const int g0 = chunk * per, g1 = g0 + per < a.groups ? g0 + per : a.groups;
    float l0 = 0.f, l1 = 0.f;
    // a vertex group's posedirs fragments live in registers, hi | lo x 16 k-steps; each half (8 k-steps) is re-loaded for the wave's NEXT group as soon as its
    // products are issued, so the loads fly behind the other half's MFMAs and the skinning epilogue
    uint4 ah[16], al[16];
    auto load_half = [&](int vg, int h) {
        const int vgc = vg < g1 ? vg : g1 - 1;   // past the chunk: a redundant in-bounds load, never used
        const uint4* ph = reinterpret_cast<const uint4*>(a.pd_hi) + (size_t)vgc * PLANE_U4 + lane;
        const uint4* pl = reinterpret_cast<const uint4*>(a.pd_lo) + (size_t)vgc * PLANE_U4 + lane;
#pragma unroll
        for (int ks = 8 * h; ks < 8 * h + 8; ++ks) {
            ah[ks] = ph[ks * 64];
            if constexpr (SPLIT) al[ks] = pl[ks * 64];
        }
    };
    if (g0 + wave < g1) { load_half(g0 + wave, 0); load_half(g0 + wave, 1); }
    for (int vg = g0 + wave; vg < g1; vg += 8) {
        f32x4 acc[NSET];
#pragma unroll
        for (int s = 0; s < NSET; ++s) acc[s] = splat4(0.f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int ks = 8 * h; ks < 8 * h + 8; ++ks)
#pragma unroll
                for (int s = 0; s < NSET; ++s) {
                    const f16x8 bh = __builtin_bit_cast(f16x8, lds[(s * PLANES) * PLANE_U4 + ks * 64 + lane]);
                    if constexpr (SPLIT) {
                        const f16x8 bl = __builtin_bit_cast(f16x8, lds[(s * PLANES + 1) * PLANE_U4 + ks * 64 + lane]);
                        acc[s] = mfma_f16(__builtin_bit_cast(f16x8, al[ks]), bh, acc[s]);
                        acc[s] = mfma_f16(__builtin_bit_cast(f16x8, ah[ks]), bl, acc[s]);
                    }
                    acc[s] = mfma_f16(__builtin_bit_cast(f16x8, ah[ks]), bh, acc[s]);
                }
            __builtin_amdgcn_sched_barrier(0);   // the re-load must not rise above the products that still read these registers
            load_half(vg + 8, h);
            __builtin_amdgcn_sched_barrier(0);
        }
        const int v = vg * 4 + g;
        const f32x4 v0 = ld4(vs + (size_t)v * 4);
        const SkinPair* list = reinterpret_cast<const SkinPair*>(a.skin) + (size_t)v * a.nnz;
        float out[NSET][3];
#pragma unroll
        for (int s = 0; s < NSET; ++s) {
            const float px = v0[0] + acc[s][0] * a.scale_inv, py = v0[1] + acc[s][1] * a.scale_inv, pz = v0[2] + acc[s][2] * a.scale_inv;
            f32x4 T0 = splat4(0.f), T1 = splat4(0.f), T2 = splat4(0.f);
            const float* As = a.A[s] + (size_t)fr * kBodyAFloats;
            for (int i = 0; i < a.nnz; ++i) {
                const SkinPair e = list[i];
                if (!__any(e.weight != 0.f)) break;   // non-zeros come first in a list: the padding of all four vertices of the wave is reached (wave-uniform)
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
        if (valid && v < a.V) {
            if constexpr (LOSS) {
                l0 += smooth_l1(out[1][0] - out[0][0]) + smooth_l1(out[1][1] - out[0][1]) + smooth_l1(out[1][2] - out[0][2]);
                if constexpr (NSET == 3) l1 += smooth_l1(out[2][0] - out[0][0]) + smooth_l1(out[2][1] - out[0][1]) + smooth_l1(out[2][2] - out[0][2]);
            } else {
                float* o = a.vertices_out + ((size_t)fr * a.V + v) * 3;
                o[0] = out[0][0]; o[1] = out[0][1]; o[2] = out[0][2];
            }
        }
    }
    if constexpr (LOSS) {
        // fixed-order reduction: xor tree inside the wave, then waves 0..7 in order
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            l0 += __shfl_xor(l0, m);
            l1 += __shfl_xor(l1, m);
        }
        __syncthreads();   // the feature planes are dead: reuse their first bytes
        float* red = reinterpret_cast<float*>(smem);
        if (lane == 0) { red[wave * 2] = l0; red[wave * 2 + 1] = l1; }
        __syncthreads();
        if (t == 0) {
            float* o = a.partials + ((size_t)tile * a.chunks + chunk) * 2;
            float r0 = red[0], r1 = red[1];
            for (int w = 1; w < 8; ++w) { r0 += red[w * 2]; r1 += red[w * 2 + 1]; }
            o[0] = r0;
            o[1] = r1;
        }
    }
}

__global__ __launch_bounds__(64) void k_body_loss_reduce(const float* partials, int n, int nsets, double* sums_out) {
    __shared__ double red[64][2];
    const int lane = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = lane; i < n; i += 64) { s0 += (double)partials[(size_t)i * 2]; s1 += (double)partials[(size_t)i * 2 + 1]; }
    red[lane][0] = s0; red[lane][1] = s1;
    __syncthreads();
    if (lane == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int i = 0; i < 64; ++i) { t0 += red[i][0]; t1 += red[i][1]; }
        sums_out[0] = t0;
        sums_out[1] = nsets == 3 ? t1 : 0.0;
    }
}

template <int NSET, bool SPLIT, bool LOSS>
hipError_t launch_skin_t(const BodySkinArgs& a, hipStream_t st) {
    constexpr int lds = NSET * (SPLIT ? 2 : 1) * 16 * 1024;
    static DeviceOnce once;
    int dev_;
    if (!once.done(&dev_)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_body_skin<NSET, SPLIT, LOSS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        once.set(dev_);
    }
    const int tiles = (a.nframes + 15) / 16;
    hipLaunchKernelGGL((k_body_skin<NSET, SPLIT, LOSS>), dim3(tiles, a.chunks), dim3(512), lds, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_body_pose(const BodyPoseArgs& a, hipStream_t st) {
    const int frames16 = (a.nframes + 15) / 16 * 16;
    hipLaunchKernelGGL(k_body_pose, dim3(frames16), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_body_skin(const BodySkinArgs& a, int split, int loss, hipStream_t st) {
    if (!loss) return split ? launch_skin_t<1, true, false>(a, st) : launch_skin_t<1, false, false>(a, st);
    if (a.nsets == 3) return split ? launch_skin_t<3, true, true>(a, st) : launch_skin_t<3, false, true>(a, st);
    return split ? launch_skin_t<2, true, true>(a, st) : launch_skin_t<2, false, true>(a, st);
}

hipError_t launch_body_loss_reduce(const float* partials, int n, int nsets, double* sums_out, hipStream_t st) {
    hipLaunchKernelGGL(k_body_loss_reduce, dim3(1), dim3(64), 0, st, partials, n, nsets, sums_out);
    return hipGetLastError();
}

}  // namespace amuse
