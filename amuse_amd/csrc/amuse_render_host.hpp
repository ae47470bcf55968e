// Preview rendering (include/amuse_hip.h amuse_render_plan / amuse_renderer_create / amuse_render): everything the renderer needs on the host, shared by
// k_render.hip (the two kernels and their launchers), amuse_render.hip (the C entry points) and tests/render_host (the same host code on stand-in launchers,
// under sanitizers):
//   - the plan: the ONE statement of the tile grid, of the frames per chunk and of the workspace's size;
//   - every argument check, made before any HIP call;
//   - the renderer object: the faces in device memory, and a workspace that follows amuse_body_reserve's rules (sized on first use, grows only, an outgrown
//     block is kept until destroy so that a graph captured earlier still replays into it).
// AN EXTENSION: the reference renders with Blender; this is a flat-shaded preview and is pinned against nothing but its own restatement (tests/render_ref.py).
// The int64 bound of the depth interpolation: inside the guard band X, Y span at most 98,303 sub-sample units, so A2 <= 98,303^2 < 2^34; the three weights are
// >= 0 and sum to A2, every Zq < 2^24, so the numerator w_a Zq_a + w_b Zq_b + w_c Zq_c <= A2 (2^24 - 1) < 2^58 - below 2^59, far from int64's end.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kRenderTile = 32;                       // samples per tile side: the key tile is 32 x 32 x 8 bytes = 8 KiB of LDS
constexpr int kRenderBlock = 256;                     // threads of both kernels
constexpr int kRenderMaxSamples = 2048;               // width ss, height ss
constexpr int kRenderMaxChunk = 256;                  // frames per launch (grid y)
constexpr size_t kRenderWsBudget = 16u << 20;         // bytes of records + view positions a chunk may take
constexpr int kRenderGuardLo = -32768, kRenderGuardHi = 65535;
constexpr int kRenderZMax = (1 << 24) - 1;

struct RenderProjectArgs {
    const float* vertices;   // [frames][V][3]
    int* screen;             // [frames][V][3]
    float* view;             // [frames][V][3]
    amuse_camera cam;
    float scale;             // 16 ss
    long long n;             // frames x V
};

struct RenderTileArgs {
    const int* faces;        // [T][3]
    const int* screen;       // [frames][V][3]
    const float* view;       // [frames][V][3] (unused without rgb)
    unsigned char* rgb;      // [frames][H][W][3] or NULL: keys only
    unsigned long long* keys;   // [frames][Hs][Ws] or NULL
    int T, V, W, H, ss, tiles_x, tiles_y, frames;
    float light[3], ambient;
    unsigned char body[3], bg[3];
};

// k_render.hip (tests/render_host: stand-ins that record the arguments)
hipError_t launch_render_project(const RenderProjectArgs& a, hipStream_t stream);
hipError_t launch_render_tile(const RenderTileArgs& a, hipStream_t stream);

struct RenderPlan {
    int tiles_x, tiles_y, chunk_frames;
    size_t section_bytes, workspace_bytes;   // one of the two sections (records | view positions); both
};

inline size_t render_align(size_t n) { return (n + 255) & ~(size_t)255; }

inline int render_check_size(int width, int height, int ss, int V, int T) {
    if (ss != 1 && ss != 2) return amuse_failf(AMUSE_EINVAL, "amuse_render: ss %d (1 or 2)", ss);
    if (width < 1 || height < 1 || width * ss > kRenderMaxSamples || height * ss > kRenderMaxSamples)
        return amuse_failf(AMUSE_EINVAL, "amuse_render: %d x %d at ss %d outside 1..%d samples per axis", width, height, ss, kRenderMaxSamples);
    if (V < 1 || T < 1) return amuse_failf(AMUSE_EINVAL, "amuse_render: V %d, T %d: both must be >= 1", V, T);
    return AMUSE_OK;
}

inline int render_plan(int width, int height, int ss, int V, int T, int frames, RenderPlan* p) {
    if (int rc = render_check_size(width, height, ss, V, T)) return rc;
    if (frames < 1) return amuse_failf(AMUSE_EINVAL, "amuse_render: frames %d < 1", frames);
    p->tiles_x = (width * ss + kRenderTile - 1) / kRenderTile;
    p->tiles_y = (height * ss + kRenderTile - 1) / kRenderTile;
    size_t fit = kRenderWsBudget / ((size_t)24 * (size_t)V);
    if (fit < 1) fit = 1;
    if (fit > (size_t)kRenderMaxChunk) fit = kRenderMaxChunk;
    p->chunk_frames = (size_t)frames < fit ? frames : (int)fit;
    p->section_bytes = render_align((size_t)p->chunk_frames * (size_t)V * 12);
    p->workspace_bytes = 2 * p->section_bytes;
    return AMUSE_OK;
}

struct Renderer {
    int device, T, V, W, H, ss;
    int* faces_dev;
    char* ws;
    size_t ws_bytes;
    std::vector<void*> retired;   // workspaces outgrown by a later call: kept until destroy
};

inline Renderer* renderer_create(int device, const int* faces, int T, int V, int width, int height, int ss) {
    if (render_check_size(width, height, ss, V, T)) return nullptr;
    if (!faces) { amuse_failf(AMUSE_EINVAL, "amuse_renderer_create: faces is NULL"); return nullptr; }
    for (size_t i = 0; i < (size_t)T * 3; ++i)
        if (faces[i] < 0 || faces[i] >= V) {
            amuse_failf(AMUSE_EINVAL, "amuse_renderer_create: face %zu names vertex %d, outside 0..%d", i / 3, faces[i], V - 1);
            return nullptr;
        }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { amuse_failf(AMUSE_EHIP, "amuse_renderer_create: hipSetDevice(%d): %s", device, hipGetErrorString(e)); return nullptr; }
    int* d = nullptr;
    const size_t bytes = (size_t)T * 3 * sizeof(int);
    e = hipMalloc(reinterpret_cast<void**>(&d), bytes);
    if (e != hipSuccess) { amuse_failf(AMUSE_ENOMEM, "amuse_renderer_create: %zu bytes of faces: %s", bytes, hipGetErrorString(e)); return nullptr; }
    e = hipMemcpy(d, faces, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        amuse_failf(AMUSE_EHIP, "amuse_renderer_create: upload of the faces: %s", hipGetErrorString(e));
        return nullptr;
    }
    return new Renderer{device, T, V, width, height, ss, d, nullptr, 0, {}};
}

inline void renderer_destroy(Renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipFree(r->faces_dev);
    (void)hipFree(r->ws);
    for (void* p : r->retired) (void)hipFree(p);
    delete r;
}

inline int render_reserve(Renderer* r, size_t bytes) {
    if (bytes <= r->ws_bytes) return AMUSE_OK;
    char* p = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
    if (e != hipSuccess) return amuse_failf(AMUSE_ENOMEM, "amuse_render: %zu bytes of workspace: %s", bytes, hipGetErrorString(e));
    if (r->ws) r->retired.push_back(r->ws);
    r->ws = p;
    r->ws_bytes = bytes;
    return AMUSE_OK;
}

inline bool render_finite(const float* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

inline void render_fill_tile(const Renderer* r, const RenderPlan& p, const amuse_shading* s, RenderTileArgs* a) {
    a->faces = r->faces_dev;
    a->T = r->T; a->V = r->V; a->W = r->W; a->H = r->H; a->ss = r->ss;
    a->tiles_x = p.tiles_x; a->tiles_y = p.tiles_y;
    static const amuse_shading kDefault = {{0.f, 0.f, -1.f}, 0.25f, {200, 200, 208}, {32, 32, 36}};
    if (!s) s = &kDefault;
    const double lx = s->light[0], ly = s->light[1], lz = s->light[2], len = std::sqrt(lx * lx + ly * ly + lz * lz);
    a->light[0] = (float)(lx / len); a->light[1] = (float)(ly / len); a->light[2] = (float)(lz / len);
    a->ambient = s->ambient;
    for (int i = 0; i < 3; ++i) { a->body[i] = s->body_rgb[i]; a->bg[i] = s->bg_rgb[i]; }
}

inline int render_run(Renderer* r, const float* vertices, int M, const amuse_camera* cam, const amuse_shading* shading, unsigned char* rgb,
                      unsigned long long* keys, int* screen_out, hipStream_t stream) {
    if (!r) return amuse_failf(AMUSE_EINVAL, "amuse_render: renderer is NULL");
    if (!vertices || !cam || !rgb) return amuse_failf(AMUSE_EINVAL, "amuse_render: vertices, camera and rgb_out must be given");
    if (M < 1) return amuse_failf(AMUSE_EINVAL, "amuse_render: M %d < 1", M);
    const float lens[6] = {cam->fx, cam->fy, cam->cx, cam->cy, cam->near_z, cam->far_z};
    if (!render_finite(cam->R, 9) || !render_finite(cam->t, 3) || !render_finite(lens, 6))
        return amuse_failf(AMUSE_EINVAL, "amuse_render: the camera holds a non-finite number");
    if (!(cam->near_z > 0.f) || !(cam->near_z < cam->far_z))
        return amuse_failf(AMUSE_EINVAL, "amuse_render: near_z %g, far_z %g: 0 < near_z < far_z is required", (double)cam->near_z, (double)cam->far_z);
    if (shading) {
        const double l2 = (double)shading->light[0] * shading->light[0] + (double)shading->light[1] * shading->light[1] + (double)shading->light[2] * shading->light[2];
        if (!render_finite(shading->light, 3) || !(l2 > 0.0)) return amuse_failf(AMUSE_EINVAL, "amuse_render: the light direction must be finite and non-zero");
        if (!(shading->ambient >= 0.f && shading->ambient <= 1.f)) return amuse_failf(AMUSE_EINVAL, "amuse_render: ambient %g outside 0..1", (double)shading->ambient);
    }
    RenderPlan p{};
    if (int rc = render_plan(r->W, r->H, r->ss, r->V, r->T, M, &p)) return rc;
    hipError_t e = hipSetDevice(r->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_render: hipSetDevice(%d): %s", r->device, hipGetErrorString(e));
    if (int rc = render_reserve(r, p.workspace_bytes)) return rc;
    RenderTileArgs ta{};
    render_fill_tile(r, p, shading, &ta);
    const size_t fv = (size_t)r->V * 3, Ws = (size_t)r->W * r->ss, Hs = (size_t)r->H * r->ss;
    for (int f0 = 0; f0 < M; f0 += p.chunk_frames) {
        const int nf = M - f0 < p.chunk_frames ? M - f0 : p.chunk_frames;
        RenderProjectArgs pa{};
        pa.vertices = vertices + (size_t)f0 * fv;
        pa.screen = screen_out ? screen_out + (size_t)f0 * fv : reinterpret_cast<int*>(r->ws);   // the caller's records are the kernel's own: one copy
        pa.view = reinterpret_cast<float*>(r->ws + p.section_bytes);
        pa.cam = *cam;
        pa.scale = 16.f * (float)r->ss;
        pa.n = (long long)nf * r->V;
        e = launch_render_project(pa, stream);
        if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_render: projection launch failed: %s", hipGetErrorString(e));
        ta.screen = pa.screen;
        ta.view = pa.view;
        ta.rgb = rgb + (size_t)f0 * r->W * r->H * 3;
        ta.keys = keys ? keys + (size_t)f0 * Ws * Hs : nullptr;
        ta.frames = nf;
        e = launch_render_tile(ta, stream);
        if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_render: tile launch failed: %s", hipGetErrorString(e));
    }
    return AMUSE_OK;
}

inline int render_raster(Renderer* r, const int* screen, int M, unsigned long long* keys, hipStream_t stream) {
    if (!r) return amuse_failf(AMUSE_EINVAL, "amuse_debug_render_raster: renderer is NULL");
    if (!screen || !keys) return amuse_failf(AMUSE_EINVAL, "amuse_debug_render_raster: screen and keys_out must be given");
    if (M < 1) return amuse_failf(AMUSE_EINVAL, "amuse_debug_render_raster: M %d < 1", M);
    RenderPlan p{};
    if (int rc = render_plan(r->W, r->H, r->ss, r->V, r->T, M, &p)) return rc;
    hipError_t e = hipSetDevice(r->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_debug_render_raster: hipSetDevice(%d): %s", r->device, hipGetErrorString(e));
    RenderTileArgs ta{};
    render_fill_tile(r, p, nullptr, &ta);
    const size_t fv = (size_t)r->V * 3, Ws = (size_t)r->W * r->ss, Hs = (size_t)r->H * r->ss;
    for (int f0 = 0; f0 < M; f0 += kRenderMaxChunk) {          // (no workspace: only the grid's y extent bounds a launch)
        ta.frames = M - f0 < kRenderMaxChunk ? M - f0 : kRenderMaxChunk;
        ta.screen = screen + (size_t)f0 * fv;
        ta.view = nullptr;
        ta.rgb = nullptr;
        ta.keys = keys + (size_t)f0 * Ws * Hs;
        e = launch_render_tile(ta, stream);
        if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_debug_render_raster: tile launch failed: %s", hipGetErrorString(e));
    }
    return AMUSE_OK;
}

}  // namespace amuse
