// Preview rendering: the C entry points (include/amuse_hip.h).  The plan touches no HIP at all; create uploads the faces; the calls touch HIP only after
// their checks, in the launches amuse_render_host.hpp makes.
#include "amuse_render_host.hpp"

extern "C" {

int amuse_render_plan(int width, int height, int ss, int V, int T, int frames, int* tiles_x, int* tiles_y, int* chunk_frames, size_t* workspace_bytes) {
    amuse::RenderPlan p{};
    if (int rc = amuse::render_plan(width, height, ss, V, T, frames, &p)) return rc;
    if (tiles_x) *tiles_x = p.tiles_x;
    if (tiles_y) *tiles_y = p.tiles_y;
    if (chunk_frames) *chunk_frames = p.chunk_frames;
    if (workspace_bytes) *workspace_bytes = p.workspace_bytes;
    return AMUSE_OK;
}

amuse_renderer* amuse_renderer_create(int device, const int* faces, int T, int V, int width, int height, int ss) {
    return reinterpret_cast<amuse_renderer*>(amuse::renderer_create(device, faces, T, V, width, height, ss));   // (the opaque handle IS the host struct)
}

void amuse_renderer_destroy(amuse_renderer* r) { amuse::renderer_destroy(reinterpret_cast<amuse::Renderer*>(r)); }

int amuse_render(amuse_renderer* r, const float* vertices_dev, int M, const amuse_camera* camera, const amuse_shading* shading, unsigned char* rgb_out_dev,
                 unsigned long long* keys_out_dev, int* screen_out_dev, void* stream) {
    return amuse::render_run(reinterpret_cast<amuse::Renderer*>(r), vertices_dev, M, camera, shading, rgb_out_dev, keys_out_dev, screen_out_dev,
                             static_cast<hipStream_t>(stream));
}

int amuse_debug_render_raster(amuse_renderer* r, const int* screen_dev, int M, unsigned long long* keys_out_dev, void* stream) {
    return amuse::render_raster(reinterpret_cast<amuse::Renderer*>(r), screen_dev, M, keys_out_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
