// Host-side packing of the SMPL-X body model (amuse_body.hip): HIP-free, so that tests/body_host/ can run it under sanitizers without a runtime.
//   * posedirs [486][V * 3] -> the A operand of v_mfma_f32_16x16x32_f16.  A 16-output tile is FOUR vertices x (x, y, z, pad): output row (v & 3) * 4 + c, so that
//     in the C/D layout (col = lane & 15 = frame, row = (lane >> 4) * 4 + reg) a lane's four accumulators are ONE vertex's offset for one frame.  K = 486 padded to
//     512 = 16 k-steps of 32; unit (group, k-step) = 64 lanes x 8 halfs, lane (g, row) holds k = 32 ks + 8 g + 0..7.  Two planes: hi = rn16(s x), lo = rn16(s x - hi),
//     s = 2^shift chosen so that the largest entry sits at 2^13..2^14: entries of 1e-7 (SMPL-X's smallest that matter) then have NORMAL hi pieces and lo pieces
//     above fp16's smallest subnormal; without it a 1e-7 entry keeps one or two bits.  The scale is exact and is undone on the fp32 accumulator.
//   * skinning weights [V][55] -> per-vertex lists of (joint, weight), padded with (0, 0.f) to the model's largest non-zero count: exact for any matrix.
//   * per subject: v_shaped = v_template + shapedirs . betas and J = J_regressor . v_shaped in double, rounded to fp32 once.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace amuse_body {

constexpr int kJoints = 55;
constexpr int kPoseFeat = 486;   // 54 x 9
constexpr int kPoseK = 512;      // padded to 16 k-steps of 32
constexpr int kKSteps = 16;

struct SkinEntry { int32_t joint; float weight; };

// fp32 -> fp16 bits, round-to-nearest-even with gradual underflow (v_cvt_pk_f16_f32), and back (exact)
inline uint16_t f2h(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
    if (x < 0x38800000u) {
        float a;
        memcpy(&a, &x, 4);
        return (uint16_t)(sign | (uint16_t)nearbyintf(a * 16777216.0f));
    }
    x -= 0x38000000u;
    x += 0xfffu + ((x >> 13) & 1u);
    return (uint16_t)(sign | (x >> 13));
}
inline float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    float f;
    uint32_t u;
    if (e == 0) {
        f = (float)m * 5.9604644775390625e-8f;
        memcpy(&u, &f, 4);
        u |= sign;
    } else {
        u = sign | (e == 31 ? 0x7f800000u | (m << 13) : ((e + 112u) << 23) | (m << 13));
    }
    memcpy(&f, &u, 4);
    return f;
}

inline bool parents_valid(const int* parents) {
    if (parents[0] != -1) return false;
    for (int j = 1; j < kJoints; ++j)
        if (parents[j] < 0 || parents[j] >= j) return false;
    return true;
}

inline int vertex_groups(int V) { return (V + 3) / 4; }

// largest entry lands in [2^13, 2^14); 0 for an all-zero (or non-finite) matrix; clamped to 0..24
inline int posedirs_shift(const float* pd, size_t n) {
    float m = 0.f;
    for (size_t i = 0; i < n; ++i) {
        const float a = fabsf(pd[i]);
        if (a > m && std::isfinite(a)) m = a;
    }
    if (!(m > 0.f)) return 0;
    int e;
    (void)frexpf(m, &e);   // m = f 2^e, f in [0.5, 1)
    int s = 14 - e;
    return s < 0 ? 0 : s > 24 ? 24 : s;
}

// index (in halfs) of posedirs[k][v * 3 + c] inside a plane
inline size_t posedirs_index(int v, int c, int k) {
    const int group = v >> 2, row = (v & 3) * 4 + c, ks = k >> 5, g = (k >> 3) & 3, j = k & 7;
    return (((size_t)group * kKSteps + ks) * 64 + (size_t)(g * 16 + row)) * 8 + j;
}
inline size_t posedirs_plane_halfs(int V) { return (size_t)vertex_groups(V) * kKSteps * 64 * 8; }

inline void pack_posedirs(const float* pd, int V, int shift, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo) {
    const size_t n = posedirs_plane_halfs(V);
    hi.assign(n, 0);
    lo.assign(n, 0);
    const float s = ldexpf(1.f, shift);
    for (int k = 0; k < kPoseFeat; ++k) {
        const float* row = pd + (size_t)k * V * 3;
        for (int v = 0; v < V; ++v)
            for (int c = 0; c < 3; ++c) {
                const float x = row[(size_t)v * 3 + c] * s;
                const uint16_t h = f2h(x);
                const size_t i = posedirs_index(v, c, k);
                hi[i] = h;
                lo[i] = f2h(x - h2f(h));
            }
    }
}

// lists [groups * 4][nnz]; returns nnz >= 1
inline int pack_skin(const float* w, int V, std::vector<SkinEntry>& out) {
    int nnz = 1;
    for (int v = 0; v < V; ++v) {
        int c = 0;
        for (int j = 0; j < kJoints; ++j) c += w[(size_t)v * kJoints + j] != 0.f;
        if (c > nnz) nnz = c;
    }
    const size_t vpad = (size_t)vertex_groups(V) * 4;
    out.assign(vpad * nnz, SkinEntry{0, 0.f});
    for (int v = 0; v < V; ++v) {
        int c = 0;
        for (int j = 0; j < kJoints; ++j) {
            const float x = w[(size_t)v * kJoints + j];
            if (x != 0.f) out[(size_t)v * nnz + c++] = SkinEntry{j, x};
        }
    }
    return nnz;
}

// one subject: v_shaped [groups * 4][4] (x, y, z, 0; pad vertices zero), J [55][4]
inline void shape_subject(int V, int n_betas, const float* v_template, const float* shapedirs, const float* Jreg, const float* betas, float* v_shaped, float* J) {
    const size_t vpad = (size_t)vertex_groups(V) * 4;
    std::vector<double> vs((size_t)V * 3);
    for (size_t i = 0; i < (size_t)V * 3; ++i) {
        double a = v_template[i];
        const float* sd = shapedirs + i * n_betas;
        for (int b = 0; b < n_betas; ++b) a += (double)sd[b] * (double)betas[b];
        vs[i] = a;
    }
    for (size_t i = 0; i < vpad * 4; ++i) v_shaped[i] = 0.f;
    for (int v = 0; v < V; ++v)
        for (int c = 0; c < 3; ++c) v_shaped[(size_t)v * 4 + c] = (float)vs[(size_t)v * 3 + c];
    for (int j = 0; j < kJoints; ++j) {
        double a[3] = {0, 0, 0};
        const float* r = Jreg + (size_t)j * V;
        for (int v = 0; v < V; ++v) {
            const double x = r[v];
            if (x != 0.0) { a[0] += x * vs[(size_t)v * 3]; a[1] += x * vs[(size_t)v * 3 + 1]; a[2] += x * vs[(size_t)v * 3 + 2]; }
        }
        J[j * 4] = (float)a[0]; J[j * 4 + 1] = (float)a[1]; J[j * 4 + 2] = (float)a[2]; J[j * 4 + 3] = 0.f;
    }
}

// ---- gradients: the transposed image.  The backward kernel's second product sums over the vertices: dpf[feature][frame] = sum_k Pt[feature][k] dp[k][frame] with
// k = (vertex-in-group, group parity, coordinate | pad) of a PAIR of consecutive vertex groups - the order in which the forward product's accumulators of two
// groups already sit in a lane.  Unit (pair, feature tile of 16) = 64 lanes x 8 halfs: lane (kg = vertex & 3, row = feature & 15) holds, at element
// j = 4 (group & 1) + c, the SAME hi | lo halfs as the forward planes hold for posedirs[feature][vertex * 3 + c] (same pre-scale).  512 feature rows (486 + pad).
// Size: pairs * 32 * 512 halfs per plane = pairs * 65,536 bytes for hi + lo: 85,852,160 bytes at V = 10,475 (1,310 pairs).
inline int vertex_pairs(int V) { return (vertex_groups(V) + 1) / 2; }
inline size_t posedirs_t_index(int v, int c, int k) {
    const int group = v >> 2, q = group >> 1, ft = k >> 4;
    return ((((size_t)q * 32 + ft) * 64) + (size_t)((v & 3) * 16 + (k & 15))) * 8 + (size_t)((group & 1) * 4 + c);
}
inline size_t posedirs_t_plane_halfs(int V) { return (size_t)vertex_pairs(V) * 32 * 64 * 8; }

// from the dense matrix (the definition; tests) ...
inline void pack_posedirs_t(const float* pd, int V, int shift, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo) {
    const size_t n = posedirs_t_plane_halfs(V);
    hi.assign(n, 0);
    lo.assign(n, 0);
    const float s = ldexpf(1.f, shift);
    for (int k = 0; k < kPoseFeat; ++k) {
        const float* row = pd + (size_t)k * V * 3;
        for (int v = 0; v < V; ++v)
            for (int c = 0; c < 3; ++c) {
                const float x = row[(size_t)v * 3 + c] * s;
                const uint16_t h = f2h(x);
                const size_t i = posedirs_t_index(v, c, k);
                hi[i] = h;
                lo[i] = f2h(x - h2f(h));
            }
    }
}
// ... and from a forward plane (what amuse_body_enable_grad does: the context keeps no dense copy of posedirs; the halfs are the forward image's, bit for bit)
inline void transpose_posedirs_plane(const uint16_t* fwd, int V, std::vector<uint16_t>& out) {
    out.assign(posedirs_t_plane_halfs(V), 0);
    for (int v = 0; v < V; ++v)
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < kPoseFeat; ++k) out[posedirs_t_index(v, c, k)] = fwd[posedirs_index(v, c, k)];
}

// chunks of vertex-group pairs per frame tile (grid.y of the backward skinning kernel): one 8-wave workgroup per CU fits, so ~2 per CU, at least one pair per wave
inline int bwd_chunks(int tiles, int pairs) {
    int c = (512 + tiles - 1) / tiles, cmax = pairs / 8;
    if (c > cmax) c = cmax;
    return c < 1 ? 1 : c;
}
inline size_t bwd_partial_workgroups(size_t frames16) { return frames16 / 16 + 512; }   // tiles * bwd_chunks(tiles, .) <= tiles + 511

// chunks of vertex groups per frame tile (grid.y of the skinning kernel): enough workgroups to fill the chip, each with at least one group per wave
inline int skin_chunks(int tiles, int groups) {
    int c = (1024 + tiles - 1) / tiles, cmax = groups / 8;
    if (c > cmax) c = cmax;
    return c < 1 ? 1 : c;
}

}  // namespace amuse_body
