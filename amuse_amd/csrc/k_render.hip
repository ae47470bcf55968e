// Preview rendering (include/amuse_hip.h amuse_render): posed mesh -> flat-shaded RGB frames, two kernels per chunk of frames.
//
// k_render_project: one thread per (frame, vertex).  View-space position in fp32 (fma chains), X / Y snapped to 1/16 sample in fp32, Zq in double (24 bits of
// depth do not survive fp32 roundings; one vertex is a handful of double operations).  Invalid vertices are stored as (0, 0, -1).
//
// k_render_tile: one workgroup per (frame, tile of 32 x 32 samples).  The tile's keys - 1024 x 64 bit = 8 KiB - live in LDS, initialised to all ones.  The 256
// lanes walk ALL triangles of the frame, one triangle per lane per round: gather the three records (a frame's records stay in L2: 125 KB at V = 10,475), reject
// by bounding box against the tile, otherwise walk the box's samples inside the tile with three int64 edge functions stepped by addition; a covered sample does
// one 64-bit LDS minimum without return on key = zpix << 32 | t.  After a barrier the same workgroup writes the keys (when asked), shades its samples from LDS,
// box-filters for ss = 2 and writes the tile's RGB bytes.  No global depth buffer, no global atomic, no clear pass; the minimum of packed integers does not
// depend on arrival order, so the image is bitwise reproducible.  Lanes diverge by box size and every tile re-reads every triangle: deliberate (no binning), see
// DESIGN.md 4.14 for what it costs.
// Bounds: a sample index is clipped to the tile AND to the image before the walk, so LDS indices stay in 0 .. 1023; faces are checked against V on the host
// when the renderer is created; every global index is formed in size_t.
#include "amuse_render_host.hpp"

#include <cstdint>

namespace amuse {

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;

__global__ void __launch_bounds__(kRenderBlock) k_render_project(const RenderProjectArgs a) {
    const long long i = (long long)blockIdx.x * kRenderBlock + threadIdx.x;
    if (i >= a.n) return;
    const float* p = a.vertices + (size_t)i * 3;
    const float x = p[0], y = p[1], z = p[2];
    const amuse_camera& c = a.cam;
    const float xc = fmaf(c.R[0], x, fmaf(c.R[1], y, fmaf(c.R[2], z, c.t[0])));
    const float yc = fmaf(c.R[3], x, fmaf(c.R[4], y, fmaf(c.R[5], z, c.t[1])));
    const float zc = fmaf(c.R[6], x, fmaf(c.R[7], y, fmaf(c.R[8], z, c.t[2])));
    float* vw = a.view + (size_t)i * 3;
    vw[0] = xc; vw[1] = yc; vw[2] = zc;
    const float u = fmaf(c.fx, xc / zc, c.cx);
    const float v = fmaf(-c.fy, yc / zc, c.cy);
    const float Xf = rintf(a.scale * u), Yf = rintf(a.scale * v);      // (16 ss is a power of two: the product is exact; rintf rounds half to even)
    const double zd = (double)c.R[6] * x + ((double)c.R[7] * y + ((double)c.R[8] * z + (double)c.t[2]));
    const double nz = c.near_z, fz = c.far_z;
    // (every comparison is false for a NaN: an invalid vertex is whatever fails one of them)
    const bool ok = zd >= nz && zd <= fz && Xf >= (float)kRenderGuardLo && Xf <= (float)kRenderGuardHi && Yf >= (float)kRenderGuardLo && Yf <= (float)kRenderGuardHi &&
                    fabsf(xc) <= 3.0e38f && fabsf(yc) <= 3.0e38f;
    int X = 0, Y = 0, Zq = -1;
    if (ok) {
        X = (int)Xf;
        Y = (int)Yf;
        Zq = (int)floor(fz * (zd - nz) / (zd * (fz - nz)) * (double)kRenderZMax + 0.5);
    }
    int* s = a.screen + (size_t)i * 3;
    s[0] = X; s[1] = Y; s[2] = Zq;
}

__device__ __forceinline__ bool record_ok(int X, int Y, int Zq) {
    return Zq >= 0 && Zq <= kRenderZMax && X >= kRenderGuardLo && X <= kRenderGuardHi && Y >= kRenderGuardLo && Y <= kRenderGuardHi;
}

// top-left rule: a sample ON an edge (E == 0) counts only for a top edge (dy == 0, dx > 0) or a left edge (dy < 0); otherwise E >= 1 is required
__device__ __forceinline__ long long edge_bias(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }

// floor(num / d) EXACTLY, for num < 2^59 and 0 < d < 2^35 with a quotient below 2^25 (the depth interpolation: the quotient is a Zq): the double estimate
// num x (1 / d) is off by less than 2^25 x 4 x 2^-53 < 1, so the truncated estimate is the quotient or one beside it, and the remainder in int64 says which.
// (A 64-bit integer division is a hundred-instruction subroutine on this target; it ran once per covered sample.)
__device__ __forceinline__ unsigned long long floor_div(unsigned long long num, long long d, double inv_d) {
    long long q = (long long)((double)num * inv_d);
    const long long r = (long long)num - q * d;
    q += r >= d ? 1 : 0;
    q -= r < 0 ? 1 : 0;
    return (unsigned long long)q;
}

__device__ __forceinline__ void shade_sample(const RenderTileArgs& a, const float* __restrict__ view, unsigned long long key, int& r, int& g, int& b) {
    if (key == kEmptyKey) { r = a.bg[0]; g = a.bg[1]; b = a.bg[2]; return; }
    const int* fc = a.faces + (size_t)(unsigned)key * 3;
    const float* p0 = view + (size_t)fc[0] * 3;
    const float* p1 = view + (size_t)fc[1] * 3;
    const float* p2 = view + (size_t)fc[2] * 3;
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float nn = nx * nx + ny * ny + nz * nz;
    float c = a.ambient;
    if (nn > 0.f) c = fmaf(1.f - a.ambient, fabsf(nx * a.light[0] + ny * a.light[1] + nz * a.light[2]) / sqrtf(nn), a.ambient);
    r = min(255, (int)floorf(fmaf((float)a.body[0], c, 0.5f)));
    g = min(255, (int)floorf(fmaf((float)a.body[1], c, 0.5f)));
    b = min(255, (int)floorf(fmaf((float)a.body[2], c, 0.5f)));
}

__global__ void __launch_bounds__(kRenderBlock) k_render_tile(const RenderTileArgs a) {
    __shared__ unsigned long long keys[kRenderTile * kRenderTile];
    const int tid = threadIdx.x;
    const int f = blockIdx.y;
    const int tile_x = blockIdx.x % a.tiles_x, tile_y = blockIdx.x / a.tiles_x;
    const int Ws = a.W * a.ss, Hs = a.H * a.ss;
    const int sx0 = tile_x * kRenderTile, sy0 = tile_y * kRenderTile;
    const int sx1 = min(sx0 + kRenderTile - 1, Ws - 1), sy1 = min(sy0 + kRenderTile - 1, Hs - 1);
    for (int i = tid; i < kRenderTile * kRenderTile; i += kRenderBlock) keys[i] = kEmptyKey;
    __syncthreads();

    const int* __restrict__ scr = a.screen + (size_t)f * a.V * 3;
    for (int t = tid; t < a.T; t += kRenderBlock) {
        const int* fc = a.faces + (size_t)t * 3;
        const int* ra = scr + (size_t)fc[0] * 3;
        const int* rb = scr + (size_t)fc[1] * 3;
        const int* rc = scr + (size_t)fc[2] * 3;
        const int xa = ra[0], ya = ra[1], za = ra[2];
        int xb = rb[0], yb = rb[1], zb = rb[2];
        int xc = rc[0], yc = rc[1], zc = rc[2];
        if (!record_ok(xa, ya, za) || !record_ok(xb, yb, zb) || !record_ok(xc, yc, zc)) continue;
        // samples whose centre 16 s + 8 lies inside the box, clipped to the tile and the image
        const int lox = max((min(xa, min(xb, xc)) + 7) >> 4, sx0), hix = min((max(xa, max(xb, xc)) - 8) >> 4, sx1);
        const int loy = max((min(ya, min(yb, yc)) + 7) >> 4, sy0), hiy = min((max(ya, max(yb, yc)) - 8) >> 4, sy1);
        if (lox > hix || loy > hiy) continue;
        long long A2 = (long long)(xb - xa) * (yc - ya) - (long long)(yb - ya) * (xc - xa);
        if (A2 == 0) continue;
        if (A2 < 0) {
            int s;
            s = xb; xb = xc; xc = s;
            s = yb; yb = yc; yc = s;
            s = zb; zb = zc; zc = s;
            A2 = -A2;
        }
        const int dxab = xb - xa, dyab = yb - ya, dxbc = xc - xb, dybc = yc - yb, dxca = xa - xc, dyca = ya - yc;
        const long long bab = edge_bias(dxab, dyab), bbc = edge_bias(dxbc, dybc), bca = edge_bias(dxca, dyca);
        const int px0 = 16 * lox + 8;
        const double inv_a2 = 1.0 / (double)A2;
        for (int sy = loy; sy <= hiy; ++sy) {
            const int py = 16 * sy + 8;
            long long eab = (long long)dxab * (py - ya) - (long long)dyab * (px0 - xa);      // weight of c
            long long ebc = (long long)dxbc * (py - yb) - (long long)dybc * (px0 - xb);      // weight of a
            long long eca = (long long)dxca * (py - yc) - (long long)dyca * (px0 - xc);      // weight of b
            unsigned long long* row = keys + (sy - sy0) * kRenderTile;
            for (int sx = lox; sx <= hix; ++sx) {
                if (eab >= bab && ebc >= bbc && eca >= bca) {
                    const unsigned long long num = (unsigned long long)(ebc * za + eca * zb + eab * zc);    // < 2^59 (amuse_render_host.hpp)
                    const unsigned long long zpix = floor_div(num, A2, inv_a2);
                    atomicMin(row + (sx - sx0), (zpix << 32) | (unsigned)t);
                }
                eab -= 16ll * dyab;
                ebc -= 16ll * dybc;
                eca -= 16ll * dyca;
            }
        }
    }
    __syncthreads();

    if (a.keys) {
        unsigned long long* ko = a.keys + (size_t)f * Hs * Ws;
        for (int i = tid; i < kRenderTile * kRenderTile; i += kRenderBlock) {
            const int sx = sx0 + (i & (kRenderTile - 1)), sy = sy0 + i / kRenderTile;
            if (sx < Ws && sy < Hs) ko[(size_t)sy * Ws + sx] = keys[i];
        }
    }
    if (!a.rgb) return;
    const float* __restrict__ view = a.view + (size_t)f * a.V * 3;
    const int side = kRenderTile / a.ss;                       // pixels per tile side
    for (int p = tid; p < side * side; p += kRenderBlock) {
        const int lx = p % side, ly = p / side;
        const int px = sx0 / a.ss + lx, py = sy0 / a.ss + ly;
        if (px >= a.W || py >= a.H) continue;
        int r = 0, g = 0, b = 0;
        for (int j = 0; j < a.ss; ++j)
            for (int i = 0; i < a.ss; ++i) {
                int sr, sg, sb;
                shade_sample(a, view, keys[(ly * a.ss + j) * kRenderTile + lx * a.ss + i], sr, sg, sb);
                r += sr; g += sg; b += sb;
            }
        if (a.ss == 2) { r = (r + 2) >> 2; g = (g + 2) >> 2; b = (b + 2) >> 2; }
        unsigned char* o = a.rgb + (((size_t)f * a.H + py) * a.W + px) * 3;
        o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
    }
}

}  // namespace

hipError_t launch_render_project(const RenderProjectArgs& a, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a.n + kRenderBlock - 1) / kRenderBlock);     // n <= 256 frames x V
    hipLaunchKernelGGL(k_render_project, dim3(blocks), dim3(kRenderBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_render_tile(const RenderTileArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_render_tile, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)a.frames), dim3(kRenderBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
