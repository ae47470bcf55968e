// Stand-alone program (its own main): the host half of the preview video encoder - csrc/amuse_mjpeg_host.hpp through the entry points of csrc/amuse_mjpeg.hip -
// under AddressSanitizer / UBSan on a machine without a GPU.  The kernels' launchers are stand-ins here that keep the argument structs and write what the kernels
// write, the HIP runtime is the stub of tests/host_asan (hipMalloc = malloc, so the uploaded tables can be read back and every carve of the workspace is checked
// against its block):
//   - the tables of every quality against the rule written out again; the Huffman words' known answers; the header walked segment by segment
//   - the plan: a sweep of sizes against the arithmetic written out again, the refused arguments
//   - create / reserve / the calls: every refusal returns AMUSE_EINVAL and launches and allocates nothing; the workspace's sections lie inside its block and
//     do not overlap; the workspace grows once and the outgrown block is kept; destroy leaves nothing behind
// tests/test_mjpeg_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "mjpeg_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amuse_amd/csrc/amuse_mjpeg_host.hpp"
#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();

#include "../host_check.hpp"

static std::vector<amuse::MjpegTransformArgs> g_transform;
static std::vector<amuse::MjpegEntropyArgs> g_size, g_scan, g_write;
static hipStream_t g_stream = nullptr;
namespace amuse {
// what each kernel writes, written here: the sanitizer sees a carve that leaves its block
hipError_t launch_mjpeg_transform(const MjpegTransformArgs& a, hipStream_t s) {
    g_transform.push_back(a);
    g_stream = s;
    memset(a.coef, 0, (size_t)a.mcus * 192 * sizeof(short));
    return hipSuccess;
}
hipError_t launch_mjpeg_size(const MjpegEntropyArgs& a, hipStream_t s) {
    g_size.push_back(a);
    g_stream = s;
    for (size_t i = 0; i < (size_t)a.frames * a.mcus_y; ++i) a.interval_bytes[i] = 10;
    return hipSuccess;
}
hipError_t launch_mjpeg_scan(const MjpegEntropyArgs& a, hipStream_t s) {
    g_scan.push_back(a);
    g_stream = s;
    unsigned long long at = 0;
    for (int f = 0; f < a.frames; ++f) {
        for (int k = 0; k < a.mcus_y; ++k) a.interval_offset[(size_t)f * a.mcus_y + k] = 10u * k;
        a.frame_entropy[f] = 10u * a.mcus_y;
        a.offsets[f] = at;
        a.sizes[f] = (unsigned)a.header_bytes + 10u * a.mcus_y + 2;
        at += a.sizes[f];
    }
    *a.total = at;
    return hipSuccess;
}
hipError_t launch_mjpeg_write(const MjpegEntropyArgs& a, hipStream_t s) {
    g_write.push_back(a);
    g_stream = s;
    const unsigned long long n = *a.total < a.out_capacity ? *a.total : a.out_capacity;
    memset(a.out, 0x5A, (size_t)n);
    return hipSuccess;
}
}  // namespace amuse

static int table_checks() {
    unsigned char lu[64], ch[64];
    for (int q = 1; q <= 100; ++q) {
        CHECK(amuse_mjpeg_tables(q, lu, ch) == 0);
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        for (int i = 0; i < 64; ++i) {
            int l = (amuse::kMjpegBaseLuma[i] * s + 50) / 100, c = (amuse::kMjpegBaseChroma[i] * s + 50) / 100;
            l = l < 1 ? 1 : l > 255 ? 255 : l;
            c = c < 1 ? 1 : c > 255 ? 255 : c;
            CHECK(lu[i] == l && ch[i] == c);
        }
    }
    CHECK(amuse_mjpeg_tables(50, lu, ch) == 0 && memcmp(lu, amuse::kMjpegBaseLuma, 64) == 0 && memcmp(ch, amuse::kMjpegBaseChroma, 64) == 0);
    CHECK(lu[0] == 16 && lu[1] == 11 && lu[8] == 12 && lu[63] == 99 && ch[0] == 17 && ch[3] == 47 && ch[4] == 99);
    CHECK(amuse_mjpeg_tables(0, lu, ch) == AMUSE_EINVAL && amuse_mjpeg_tables(101, lu, ch) == AMUSE_EINVAL && strstr(g_err, "quality"));
    CHECK(amuse_mjpeg_tables(50, nullptr, ch) == AMUSE_EINVAL && amuse_mjpeg_tables(50, lu, nullptr) == AMUSE_EINVAL);
    // the zigzag is a permutation that walks the anti-diagonals
    bool seen[64] = {};
    for (int k = 0; k < 64; ++k) {
        const int n = amuse::kMjpegZigzag[k];
        CHECK(n < 64 && !seen[n]);
        seen[n] = true;
        if (k) { const int p = amuse::kMjpegZigzag[k - 1], d = (n / 8 + n % 8) - (p / 8 + p % 8); CHECK(d == 0 || d == 1); }
    }
    // Annex K.3 known answers: EOB 1010, ZRL 11111111001, luma DC category 0 = 00; every table is complete up to its count
    unsigned int w[amuse::kMjpegHuffWords];
    amuse::mjpeg_huff_words(w);
    CHECK(w[0x00] == ((4u << 16) | 0xA) && w[0xF0] == ((11u << 16) | 0x7F9) && w[512] == ((2u << 16) | 0) && w[256] == ((2u << 16) | 0) && w[256 + 0xF0] == ((10u << 16) | 0x3FA));
    int used = 0;
    for (int i = 0; i < 512; ++i) used += w[i] != 0;
    CHECK(used == 2 * 162);
    for (int c = 0; c <= 11; ++c) CHECK(w[512 + c] != 0 && w[528 + c] != 0);
    for (int i = 0; i < amuse::kMjpegHuffWords; ++i) CHECK((w[i] >> 16) <= 16 && (w[i] == 0 || (w[i] & 0xFFFF) < (1u << (w[i] >> 16))));
    return 0;
}

static int header_checks() {
    const int sizes[][3] = {{16, 8, 50}, {21, 19, 90}, {512, 512, 90}, {4096, 1, 1}, {1, 4096, 100}};
    for (const auto& s : sizes) {
        std::vector<unsigned char> h(1024);
        int n = 0;
        CHECK(amuse_debug_mjpeg_header(s[0], s[1], s[2], h.data(), h.size(), &n) == 0 && n == 629 && (size_t)n == amuse::mjpeg_header_bytes());
        CHECK(h[0] == 0xFF && h[1] == 0xD8);
        const int want[] = {0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA};
        int p = 2;
        for (int m : want) {
            CHECK(p + 4 <= n && h[p] == 0xFF && h[p + 1] == m);
            const int len = h[p + 2] << 8 | h[p + 3];
            if (m == 0xC0) CHECK((h[p + 5] << 8 | h[p + 6]) == s[1] && (h[p + 7] << 8 | h[p + 8]) == s[0] && h[p + 9] == 3 && h[p + 11] == 0x11);
            if (m == 0xDD) CHECK((h[p + 4] << 8 | h[p + 5]) == (s[0] + 7) / 8);
            p += 2 + len;
        }
        CHECK(p == n);
        int small = -1;
        unsigned char two[2] = {7, 7};
        CHECK(amuse_debug_mjpeg_header(s[0], s[1], s[2], two, 2, &small) == 0 && small == 629 && two[0] == 7 && two[1] == 7);   // too small: the length only
    }
    unsigned char b[700];
    int n = 0;
    CHECK(amuse_debug_mjpeg_header(0, 8, 50, b, sizeof(b), &n) == AMUSE_EINVAL && amuse_debug_mjpeg_header(8, 8, 0, b, sizeof(b), &n) == AMUSE_EINVAL);
    CHECK(amuse_debug_mjpeg_header(8, 8, 50, nullptr, 0, &n) == AMUSE_EINVAL && amuse_debug_mjpeg_header(8, 8, 50, b, sizeof(b), nullptr) == AMUSE_EINVAL);
    return 0;
}

static int plan_checks() {
    int mx = 0, my = 0, hb = 0;
    size_t ws = 0, worst = 0;
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 7}, {16, 8}, {21, 19}, {40, 72}, {512, 512}, {4096, 4096}, {4096, 1}, {1, 4096}};
    const int Fs[] = {1, 2, 63, 64, 65, 300, 1800};
    for (const auto& s : sizes)
        for (int F : Fs) {
            CHECK(amuse_mjpeg_plan(s[0], s[1], F, &mx, &my, &hb, &ws, &worst) == 0);
            CHECK(mx == (s[0] + 7) / 8 && my == (s[1] + 7) / 8 && hb == 629);
            const size_t coef = ((size_t)F * mx * my * 384 + 255) / 256 * 256, iv = ((size_t)F * my * 4 + 255) / 256 * 256, fr = ((size_t)F * 4 + 255) / 256 * 256;
            CHECK(ws == coef + 2 * iv + fr);
            CHECK(worst == 629 + (size_t)my * 2 * (((size_t)mx * 3 * 1660 + 7) / 8) + 2 * (size_t)(my - 1) + 2);
        }
    CHECK(amuse_mjpeg_plan(64, 64, 5, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);   // every output is optional
    CHECK(amuse_mjpeg_plan(0, 64, 5, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_plan(64, -1, 5, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_plan(4097, 64, 5, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_plan(64, 4097, 5, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_plan(64, 64, 0, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL && strstr(g_err, "frames"));
    CHECK(amuse_mjpeg_plan(4096, 4096, 2147483647, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL && strstr(g_err, "index"));      // block counts beyond an int
    CHECK(amuse_mjpeg_plan(4096, 4096, 32767, &mx, &my, &hb, &ws, &worst) == 0);                                                 // 2^31 - 2^16 transform blocks
    CHECK(amuse_mjpeg_plan(4096, 4096, 32768, &mx, &my, &hb, &ws, &worst) == AMUSE_EINVAL);
    return 0;
}

static int call_checks() {
    const int W = 21, H = 19, Q = 90;
    CHECK(amuse_mjpeg_create(0, 0, H, Q) == nullptr && amuse_mjpeg_create(0, W, 4097, Q) == nullptr && amuse_mjpeg_create(0, W, H, 0) == nullptr);
    CHECK(amuse_mjpeg_create(0, W, H, 101) == nullptr && amuse_stub_live_allocations() == 0);
    amuse_mjpeg* e = amuse_mjpeg_create(0, W, H, Q);
    CHECK(e != nullptr && amuse_stub_live_allocations() == 3);                     // header, Huffman words, divisors
    const amuse::Mjpeg* m = reinterpret_cast<const amuse::Mjpeg*>(e);
    CHECK(m->W == W && m->H == H && m->quality == Q && m->reserved_frames == 0 && m->ws == nullptr && m->ws_bytes == 0);
    {   // the uploads are what the host-only calls state
        unsigned char h[700], lu[64], ch[64];
        int n = 0;
        CHECK(amuse_debug_mjpeg_header(W, H, Q, h, sizeof(h), &n) == 0 && memcmp(m->header_dev, h, n) == 0);
        CHECK(amuse_mjpeg_tables(Q, lu, ch) == 0);
        for (int k = 0; k < 64; ++k) CHECK(m->qdiv_dev[k] == (float)lu[amuse::kMjpegZigzag[k]] && m->qdiv_dev[64 + k] == (float)ch[amuse::kMjpegZigzag[k]]);
        unsigned int w[amuse::kMjpegHuffWords];
        amuse::mjpeg_huff_words(w);
        CHECK(memcmp(m->huff_dev, w, sizeof(w)) == 0);
    }
    const int Mmax = 9, mx = 3, my = 3;
    std::vector<unsigned char> rgb((size_t)Mmax * W * H * 3, 100), out(4096);
    std::vector<short> coef((size_t)Mmax * mx * my * 192);                          // exactly the announced size: a write past it is the sanitizer's to find
    std::vector<unsigned long long> offsets(Mmax);
    std::vector<unsigned int> sizes(Mmax);
    unsigned long long total = 0;
    void* st = reinterpret_cast<void*>(0x40);

    // refusals: nothing launched, nothing allocated
    CHECK(amuse_mjpeg_reserve(nullptr, 1) == AMUSE_EINVAL && amuse_mjpeg_reserve(e, 0) == AMUSE_EINVAL && amuse_mjpeg_reserve(e, -1) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(nullptr, rgb.data(), 1, out.data(), out.size(), offsets.data(), sizes.data(), &total, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, nullptr, 1, out.data(), out.size(), offsets.data(), sizes.data(), &total, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 1, nullptr, out.size(), offsets.data(), sizes.data(), &total, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 1, out.data(), out.size(), nullptr, sizes.data(), &total, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 1, out.data(), out.size(), offsets.data(), nullptr, &total, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 1, out.data(), out.size(), offsets.data(), sizes.data(), nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 0, out.data(), out.size(), offsets.data(), sizes.data(), &total, st) == AMUSE_EINVAL);
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 1, out.data(), out.size(), offsets.data(), sizes.data(), &total, st) == AMUSE_EINVAL && strstr(g_err, "reserve"));   // a call allocates nothing
    CHECK(amuse_debug_mjpeg_coefficients(nullptr, rgb.data(), 1, coef.data(), st) == AMUSE_EINVAL);
    CHECK(amuse_debug_mjpeg_coefficients(e, nullptr, 1, coef.data(), st) == AMUSE_EINVAL);
    CHECK(amuse_debug_mjpeg_coefficients(e, rgb.data(), 1, nullptr, st) == AMUSE_EINVAL);
    CHECK(amuse_debug_mjpeg_coefficients(e, rgb.data(), 0, coef.data(), st) == AMUSE_EINVAL);
    CHECK(g_transform.empty() && g_size.empty() && g_scan.empty() && g_write.empty() && m->ws == nullptr && amuse_stub_live_allocations() == 3);

    // the transform alone: the caller's array, no workspace
    CHECK(amuse_debug_mjpeg_coefficients(e, rgb.data(), Mmax, coef.data(), st) == 0);
    CHECK(g_transform.size() == 1 && g_size.empty() && g_stream == static_cast<hipStream_t>(st) && amuse_stub_live_allocations() == 3);
    CHECK(g_transform[0].rgb == rgb.data() && g_transform[0].coef == coef.data() && g_transform[0].qdiv == m->qdiv_dev && g_transform[0].W == W && g_transform[0].H == H);
    CHECK(g_transform[0].mcus_x == mx && g_transform[0].mcus_y == my && g_transform[0].mcus == (long long)Mmax * mx * my);
    g_transform.clear();

    // reserve, then calls within it: the sections lie inside the block, in order, without overlap
    size_t ws2 = 0, ws9 = 0;
    CHECK(amuse_mjpeg_plan(W, H, 2, nullptr, nullptr, nullptr, &ws2, nullptr) == 0 && amuse_mjpeg_plan(W, H, Mmax, nullptr, nullptr, nullptr, &ws9, nullptr) == 0);
    CHECK(amuse_mjpeg_reserve(e, 2) == 0 && m->reserved_frames == 2 && m->ws_bytes == ws2 && m->ws != nullptr && amuse_stub_live_allocations() == 4);
    const char* first_ws = m->ws;
    CHECK(amuse_mjpeg_reserve(e, 1) == 0 && m->ws == first_ws && m->reserved_frames == 2);                     // grows only
    CHECK(amuse_mjpeg_encode(e, rgb.data(), 3, out.data(), out.size(), offsets.data(), sizes.data(), &total, st) == AMUSE_EINVAL && g_transform.empty());
    for (int M = 1; M <= 2; ++M) {
        CHECK(amuse_mjpeg_encode(e, rgb.data(), M, out.data(), 700, offsets.data(), sizes.data(), &total, nullptr) == 0);
        CHECK(g_transform.size() == 1 && g_size.size() == 1 && g_scan.size() == 1 && g_write.size() == 1 && g_stream == nullptr);
        const amuse::MjpegEntropyArgs& a = g_write[0];
        CHECK(memcmp(&a, &g_size[0], sizeof(a)) == 0 && memcmp(&a, &g_scan[0], sizeof(a)) == 0);               // one description for the three passes
        CHECK(g_transform[0].coef == reinterpret_cast<short*>(m->ws) && a.coef == g_transform[0].coef && g_transform[0].mcus == (long long)M * mx * my);
        const char* c0 = m->ws;
        const char* i0 = reinterpret_cast<const char*>(a.interval_bytes);
        const char* o0 = reinterpret_cast<const char*>(a.interval_offset);
        const char* f0 = reinterpret_cast<const char*>(a.frame_entropy);
        CHECK(c0 + (size_t)M * mx * my * 384 <= i0 && i0 + (size_t)M * my * 4 <= o0 && o0 + (size_t)M * my * 4 <= f0 && f0 + (size_t)M * 4 <= m->ws + m->ws_bytes);
        CHECK(a.huff == m->huff_dev && a.header == m->header_dev && a.out == out.data() && a.out_capacity == 700 && a.offsets == offsets.data());
        CHECK(a.sizes == sizes.data() && a.total == &total && a.mcus_x == mx && a.mcus_y == my && a.frames == M && a.header_bytes == 629);
        CHECK(total == (unsigned long long)M * (629 + 30 + 2));
        if (M == 2) CHECK(out[699] == 0x5A && out[700] == 0);                                                  // (the stand-in stops at the capacity, as the kernel must)
        g_transform.clear(); g_size.clear(); g_scan.clear(); g_write.clear();
        memset(out.data(), 0, out.size());
    }
    CHECK(amuse_mjpeg_reserve(e, Mmax) == 0 && m->reserved_frames == Mmax && m->ws_bytes == ws9 && m->ws != first_ws);
    CHECK(m->retired.size() == 1 && m->retired[0] == first_ws && amuse_stub_live_allocations() == 5);          // the outgrown block is kept, not freed
    const long live = amuse_stub_live_allocations();
    CHECK(amuse_mjpeg_encode(e, rgb.data(), Mmax, out.data(), out.size(), offsets.data(), sizes.data(), &total, st) == 0 && amuse_stub_live_allocations() == live);
    CHECK(g_write.size() == 1 && g_write[0].frames == Mmax && offsets[Mmax - 1] == (unsigned long long)(Mmax - 1) * 661 && sizes[Mmax - 1] == 661);

    amuse_mjpeg_destroy(e);
    amuse_mjpeg_destroy(nullptr);
    CHECK(amuse_stub_live_allocations() == 0);
    return 0;
}

int main() {
    if (int e = table_checks()) return e;
    if (int e = header_checks()) return e;
    if (int e = plan_checks()) return e;
    if (int e = call_checks()) return e;
    puts("mjpeg_host ok");
    return 0;
}
