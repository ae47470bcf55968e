// Stand-alone program (its own main): the host half of the preview renderer - csrc/amuse_render_host.hpp through the entry points of csrc/amuse_render.hip -
// under AddressSanitizer / UBSan on a machine without a GPU.  The two kernels' launchers are stand-ins here that keep the argument structs, the HIP runtime is
// the stub of tests/host_asan (hipMalloc = malloc, so the uploaded faces can be read back and every carve of the workspace is checked against its block):
//   - the plan: a sweep of sizes against the arithmetic written out again, the refused arguments
//   - create: the refusals (a face index outside 0..V-1 among them) launch and allocate nothing; the uploaded faces are the caller's
//   - the call: every refusal returns AMUSE_EINVAL and launches nothing; M around chunk_frames gives the chunks the plan states, each with its own slice of the
//     inputs and outputs, all inside the workspace's block; the workspace grows once and is kept; destroy leaves nothing behind
// tests/test_render_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "render_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amuse_amd/csrc/amuse_render_host.hpp"
#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();

#include "../host_check.hpp"

static std::vector<amuse::RenderProjectArgs> g_project;
static std::vector<amuse::RenderTileArgs> g_tile;
static hipStream_t g_stream = nullptr;
namespace amuse {
hipError_t launch_render_project(const RenderProjectArgs& a, hipStream_t s) {
    g_project.push_back(a);
    g_stream = s;
    // what the kernel writes, written here: the sanitizer sees a carve that leaves its block
    memset(a.screen, 0, (size_t)a.n * 3 * sizeof(int));
    memset(a.view, 0, (size_t)a.n * 3 * sizeof(float));
    return hipSuccess;
}
hipError_t launch_render_tile(const RenderTileArgs& a, hipStream_t s) {
    g_tile.push_back(a);
    g_stream = s;
    if (a.rgb) memset(a.rgb, 1, (size_t)a.frames * a.W * a.H * 3);
    if (a.keys) memset(a.keys, 2, (size_t)a.frames * a.W * a.ss * a.H * a.ss * sizeof(unsigned long long));
    return hipSuccess;
}
}  // namespace amuse

static int plan_checks() {
    int tx = 0, ty = 0, ch = 0;
    size_t ws = 0;
    const int sizes[][3] = {{1, 1, 1}, {32, 32, 1}, {33, 31, 1}, {72, 40, 1}, {40, 24, 2}, {512, 512, 2}, {1024, 1024, 2}, {2048, 16, 1}, {16, 2048, 1}};
    const int Vs[] = {1, 3, 203, 2730, 2731, 10475, 699050, 699051, 5000000};
    const int Fs[] = {1, 2, 66, 67, 255, 256, 257, 300, 100000};
    for (const auto& s : sizes)
        for (int V : Vs)
            for (int F : Fs) {
                CHECK(amuse_render_plan(s[0], s[1], s[2], V, 7, F, &tx, &ty, &ch, &ws) == 0);
                CHECK(tx == (s[0] * s[2] + 31) / 32 && ty == (s[1] * s[2] + 31) / 32);
                long long fit = (16ll << 20) / (24ll * V);                    // the frames 16 MiB hold, written out again
                if (fit < 1) fit = 1;
                if (fit > 256) fit = 256;
                CHECK(ch == (F < fit ? F : (int)fit));
                const size_t section = ((size_t)ch * V * 12 + 255) / 256 * 256;
                CHECK(ws == 2 * section && section >= (size_t)ch * V * 12);
            }
    CHECK(amuse_render_plan(64, 64, 1, 10, 10, 5, nullptr, nullptr, nullptr, nullptr) == 0);   // every output is optional
    CHECK(amuse_render_plan(64, 64, 0, 10, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(64, 64, 3, 10, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(2049, 64, 1, 10, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(64, 1025, 2, 10, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(0, 64, 1, 10, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(64, -1, 1, 10, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(64, 64, 1, 0, 10, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(64, 64, 1, 10, 0, 5, &tx, &ty, &ch, &ws) == AMUSE_EINVAL);
    CHECK(amuse_render_plan(64, 64, 1, 10, 10, 0, &tx, &ty, &ch, &ws) == AMUSE_EINVAL && strstr(g_err, "frames"));
    return 0;
}

static int call_checks() {
    const int V = 5, T = 3, W = 40, H = 24, ss = 2;
    const int faces[T * 3] = {0, 1, 2, 2, 1, 3, 4, 0, 3};
    {   // refusals of create: nothing allocated
        int bad[T * 3];
        memcpy(bad, faces, sizeof(bad));
        bad[7] = V;
        CHECK(amuse_renderer_create(0, bad, T, V, W, H, ss) == nullptr && strstr(g_err, "face 2"));
        bad[7] = -1;
        CHECK(amuse_renderer_create(0, bad, T, V, W, H, ss) == nullptr);
        CHECK(amuse_renderer_create(0, nullptr, T, V, W, H, ss) == nullptr);
        CHECK(amuse_renderer_create(0, faces, T, V, W, H, 3) == nullptr);
        CHECK(amuse_renderer_create(0, faces, T, V, 1025, H, 2) == nullptr);
        CHECK(amuse_renderer_create(0, faces, 0, V, W, H, ss) == nullptr);
        CHECK(amuse_renderer_create(0, faces, T, 0, W, H, ss) == nullptr);
        CHECK(amuse_stub_live_allocations() == 0);
    }
    amuse_renderer* r = amuse_renderer_create(0, faces, T, V, W, H, ss);
    CHECK(r != nullptr);
    const amuse::Renderer* rr = reinterpret_cast<const amuse::Renderer*>(r);
    CHECK(rr->T == T && rr->V == V && rr->W == W && rr->H == H && rr->ss == ss && rr->ws == nullptr && rr->ws_bytes == 0);
    CHECK(memcmp(rr->faces_dev, faces, sizeof(faces)) == 0);

    int chunk = 0;
    size_t ws_bytes = 0;
    CHECK(amuse_render_plan(W, H, ss, V, T, 1000, nullptr, nullptr, &chunk, &ws_bytes) == 0 && chunk == 256);
    const int Mmax = chunk + 1;
    std::vector<float> verts((size_t)Mmax * V * 3, 0.5f);
    std::vector<unsigned char> rgb((size_t)Mmax * W * H * 3);                 // exactly the announced sizes: a write past them is the sanitizer's to find
    std::vector<unsigned long long> keys((size_t)Mmax * W * ss * H * ss);
    std::vector<int> screen((size_t)Mmax * V * 3);
    amuse_camera cam = {{1, 0, 0, 0, 1, 0, 0, 0, -1}, {0, 0, 5}, 100.f, 100.f, 20.f, 12.f, 1.f, 9.f};
    amuse_shading sh = {{0.f, 3.f, -4.f}, 0.5f, {10, 20, 30}, {1, 2, 3}};
    void* st = reinterpret_cast<void*>(0x40);

    // refusals: nothing launched, nothing allocated
    CHECK(amuse_render(nullptr, verts.data(), 1, &cam, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_render(r, nullptr, 1, &cam, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_render(r, verts.data(), 1, nullptr, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_render(r, verts.data(), 1, &cam, nullptr, nullptr, nullptr, nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_render(r, verts.data(), 0, &cam, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL);
    {
        amuse_camera c = cam;
        c.near_z = 0.f;
        CHECK(amuse_render(r, verts.data(), 1, &c, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL && strstr(g_err, "near_z"));
        c.near_z = 9.f;
        CHECK(amuse_render(r, verts.data(), 1, &c, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL);
        c = cam;
        c.R[4] = NAN;
        CHECK(amuse_render(r, verts.data(), 1, &c, nullptr, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL && strstr(g_err, "non-finite"));
        amuse_shading s = sh;
        s.light[1] = s.light[2] = 0.f;
        CHECK(amuse_render(r, verts.data(), 1, &cam, &s, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL && strstr(g_err, "light"));
        s = sh;
        s.ambient = 1.25f;
        CHECK(amuse_render(r, verts.data(), 1, &cam, &s, rgb.data(), nullptr, nullptr, st) == AMUSE_EINVAL && strstr(g_err, "ambient"));
    }
    CHECK(amuse_debug_render_raster(nullptr, screen.data(), 1, keys.data(), st) == AMUSE_EINVAL);
    CHECK(amuse_debug_render_raster(r, nullptr, 1, keys.data(), st) == AMUSE_EINVAL);
    CHECK(amuse_debug_render_raster(r, screen.data(), 1, nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_debug_render_raster(r, screen.data(), 0, keys.data(), st) == AMUSE_EINVAL);
    CHECK(g_project.empty() && g_tile.empty() && rr->ws == nullptr && amuse_stub_live_allocations() == 1);   // (the faces)

    // one frame: the workspace is sized for it; defaults for the shading
    CHECK(amuse_render(r, verts.data(), 1, &cam, nullptr, rgb.data(), nullptr, nullptr, st) == 0);
    CHECK(g_project.size() == 1 && g_tile.size() == 1 && g_stream == static_cast<hipStream_t>(st));
    size_t ws1 = 0;
    CHECK(amuse_render_plan(W, H, ss, V, T, 1, nullptr, nullptr, nullptr, &ws1) == 0 && rr->ws_bytes == ws1 && rr->ws != nullptr);
    {
        const amuse::RenderProjectArgs& p = g_project[0];
        const amuse::RenderTileArgs& t = g_tile[0];
        CHECK(p.vertices == verts.data() && p.n == V && p.scale == 32.f && p.screen == reinterpret_cast<int*>(rr->ws));
        CHECK(reinterpret_cast<char*>(p.view) == rr->ws + ws1 / 2 && memcmp(&p.cam, &cam, sizeof(cam)) == 0);
        CHECK(t.faces == rr->faces_dev && t.screen == p.screen && t.view == p.view && t.rgb == rgb.data() && t.keys == nullptr && t.frames == 1);
        CHECK(t.T == T && t.V == V && t.W == W && t.H == H && t.ss == ss && t.tiles_x == 3 && t.tiles_y == 2);
        CHECK(t.light[0] == 0.f && t.light[1] == 0.f && t.light[2] == -1.f && t.ambient == 0.25f && t.body[0] == 200 && t.body[2] == 208 && t.bg[0] == 32 && t.bg[2] == 36);
    }
    const char* first_ws = rr->ws;
    g_project.clear();
    g_tile.clear();

    // M around chunk_frames: the workspace grows once (to the full chunk) and the outgrown block is kept, not freed
    const int Ms[] = {chunk - 1, chunk, chunk + 1};
    size_t grown_times = 0;
    for (int M : Ms) {
        const char* ws_before = rr->ws;
        const size_t bytes_before = rr->ws_bytes;
        CHECK(amuse_render(r, verts.data(), M, &cam, &sh, rgb.data(), keys.data(), screen.data(), nullptr) == 0);
        const size_t launches = M > chunk ? 2 : 1;
        CHECK(g_project.size() == launches && g_tile.size() == launches);
        size_t wsM = 0;
        CHECK(amuse_render_plan(W, H, ss, V, T, M, nullptr, nullptr, nullptr, &wsM) == 0 && rr->ws_bytes >= wsM);
        if (wsM > bytes_before) {                                             // grown: a new block of exactly the plan's size, the old one kept
            ++grown_times;
            CHECK(rr->ws != ws_before && rr->ws_bytes == wsM && rr->retired.size() == grown_times && rr->retired.back() == ws_before);
        } else {
            CHECK(rr->ws == ws_before && rr->ws_bytes == bytes_before && rr->retired.size() == grown_times);
        }
        int f0 = 0;
        for (size_t k = 0; k < launches; ++k) {
            const int nf = M - f0 < chunk ? M - f0 : chunk;
            const amuse::RenderProjectArgs& p = g_project[k];
            const amuse::RenderTileArgs& t = g_tile[k];
            CHECK(p.vertices == verts.data() + (size_t)f0 * V * 3 && p.n == (long long)nf * V);
            CHECK(p.screen == screen.data() + (size_t)f0 * V * 3);                             // the caller's records are the kernel's own
            CHECK(reinterpret_cast<char*>(p.view) >= rr->ws && reinterpret_cast<char*>(p.view) + (size_t)nf * V * 12 <= rr->ws + rr->ws_bytes);
            CHECK(t.frames == nf && t.screen == p.screen && t.view == p.view);
            CHECK(t.rgb == rgb.data() + (size_t)f0 * W * H * 3 && t.keys == keys.data() + (size_t)f0 * W * ss * H * ss);
            CHECK(t.light[0] == 0.f && t.light[1] == 0.6f && t.light[2] == -0.8f && t.ambient == 0.5f && t.body[1] == 20 && t.bg[2] == 3);
            f0 += nf;
        }
        CHECK(f0 == M);
        g_project.clear();
        g_tile.clear();
    }
    CHECK(grown_times >= 1 && rr->retired[0] == first_ws);                                    // (255 and 256 frames of 5 vertices round to the same 256-byte multiple)
    CHECK(amuse_stub_live_allocations() == 2 + (long)grown_times);                            // faces + workspace + the outgrown blocks
    const long live = amuse_stub_live_allocations();
    const char* grown = rr->ws;
    CHECK(amuse_render(r, verts.data(), 3, &cam, nullptr, rgb.data(), nullptr, nullptr, nullptr) == 0 && rr->ws == grown && amuse_stub_live_allocations() == live);
    CHECK(g_project[0].screen == reinterpret_cast<int*>(rr->ws));                              // without screen_out the records live in the workspace
    g_project.clear();
    g_tile.clear();

    // the raster stage alone: no projection, no workspace; one launch per 256 frames
    CHECK(amuse_debug_render_raster(r, screen.data(), Mmax, keys.data(), st) == 0);
    CHECK(g_project.empty() && g_tile.size() == 2 && g_tile[0].frames == 256 && g_tile[1].frames == 1 && g_tile[0].rgb == nullptr && g_tile[0].view == nullptr);
    CHECK(g_tile[1].screen == screen.data() + (size_t)256 * V * 3 && g_tile[1].keys == keys.data() + (size_t)256 * W * ss * H * ss);
    g_tile.clear();

    amuse_renderer_destroy(r);
    amuse_renderer_destroy(nullptr);
    CHECK(amuse_stub_live_allocations() == 0);
    return 0;
}

int main() {
    if (int e = plan_checks()) return e;
    if (int e = call_checks()) return e;
    puts("render_host ok");
    return 0;
}
