// Stand-alone program (its own main): the host half of BVH export - csrc/amuse_bvh_host.hpp through the four entry points of csrc/amuse_bvh.hip - under
// AddressSanitizer / UBSan on a machine without a GPU.  The kernels' launchers are stand-ins here that keep the argument structs, so the packing of a call's
// sequences into launches can be checked entry by entry:
//   - the layout: refused parent lists, known trees, every joint once, a parent before its children, children in ascending index, a chain and a star at the size limit
//   - the checks of the formatter, the exporter and the decoder: every refusal returns AMUSE_EINVAL and launches nothing
//   - the packing: S = 1, the per-launch capacity, one more, and several launches' worth - 64-bit row offsets (byte offsets beyond 2^36), counts, the longest sequence, the call-wide index
// tests/test_bvh_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "bvh_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../amuse_amd/csrc/amuse_bvh_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::BvhArgs> g_motion;
static std::vector<amuse::BvhDecodeArgs> g_decode;
static int g_format = 0;
static long long g_format_n = 0;
static hipStream_t g_stream = nullptr;
namespace amuse {
hipError_t launch_bvh_format(const float*, long long n, int, unsigned char*, int*, hipStream_t s) { ++g_format; g_format_n = n; g_stream = s; return hipSuccess; }
hipError_t launch_bvh_motion(const BvhArgs& a, hipStream_t s) { g_motion.push_back(a); g_stream = s; return hipSuccess; }
hipError_t launch_bvh_decode(const BvhDecodeArgs& a, hipStream_t s) { g_decode.push_back(a); g_stream = s; return hipSuccess; }
}  // namespace amuse

static int layout_checks() {
    int out[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
    const int ok4[4] = {-1, 0, 0, 1};
    CHECK(amuse_bvh_layout(ok4, 0, out) == AMUSE_EINVAL && amuse_bvh_layout(ok4, -1, out) == AMUSE_EINVAL && amuse_bvh_layout(ok4, 65537, out) == AMUSE_EINVAL);
    CHECK(amuse_bvh_layout(nullptr, 4, out) == AMUSE_EINVAL && amuse_bvh_layout(ok4, 4, nullptr) == AMUSE_EINVAL);
    const int bad[5][4] = {{0, 0, 0, 1}, {-1, 1, 0, 0}, {-1, 0, 2, 0}, {-1, 0, 0, 3}, {-1, -1, 0, 0}};
    for (const auto& b : bad) CHECK(amuse_bvh_layout(b, 4, out) == AMUSE_EINVAL);
    CHECK(out[0] == -7);                                             // a refused call writes nothing
    CHECK(amuse_bvh_layout(ok4, 4, out) == 0 && out[0] == 0 && out[1] == 1 && out[2] == 3 && out[3] == 2 && out[4] == -7);
    const int one[1] = {-1};
    CHECK(amuse_bvh_layout(one, 1, out) == 0 && out[0] == 0 && out[1] == 1);
    // a seeded random tree, a chain and a star at the size limit: a permutation, a parent before its children, siblings' subtrees in ascending index
    for (int kind = 0; kind < 3; ++kind) {
        const int n = kind == 0 ? 1000 : 65536;
        std::vector<int> p(n), d(n + 1, -7), at(n);
        unsigned x = 12345u;
        p[0] = -1;
        for (int j = 1; j < n; ++j) {
            x = x * 1664525u + 1013904223u;
            p[j] = kind == 0 ? (int)((x >> 8) % (unsigned)j) : kind == 1 ? j - 1 : 0;
        }
        CHECK(amuse_bvh_layout(p.data(), n, d.data()) == 0 && d[n] == -7 && d[0] == 0);
        std::vector<char> seen(n, 0);
        for (int c = 0; c < n; ++c) {
            CHECK(d[c] >= 0 && d[c] < n && !seen[d[c]]);
            seen[d[c]] = 1;
            at[d[c]] = c;
        }
        for (int j = 1; j < n; ++j) CHECK(at[p[j]] < at[j]);
        for (int j = 2; j < n; ++j)
            for (int k = j - 1; k >= 1 && k > j - 40; --k)
                if (p[k] == p[j]) { CHECK(at[k] < at[j]); break; }
        if (kind != 0)
            for (int c = 0; c < n; ++c) CHECK(d[c] == c);
    }
    return 0;
}

static int check_checks() {
    std::vector<float> buf(4096);
    float* f = buf.data();
    unsigned char* t = reinterpret_cast<unsigned char*>(buf.data() + 1024);
    int status[4] = {0, 0, 0, 0};
    void* st = reinterpret_cast<void*>(0x40);
    // the formatter
    CHECK(amuse_bvh_format(f, 0, 168, t, status, st) == AMUSE_EINVAL && amuse_bvh_format(f, -5, 168, t, status, st) == AMUSE_EINVAL);
    CHECK(amuse_bvh_format(f, (long long)INT_MAX * 256 + 1, 168, t, status, st) == AMUSE_EINVAL);
    CHECK(amuse_bvh_format(f, 8, 0, t, status, st) == AMUSE_EINVAL && amuse_bvh_format(f, 8, -1, t, status, st) == AMUSE_EINVAL);
    CHECK(amuse_bvh_format(nullptr, 8, 168, t, status, st) == AMUSE_EINVAL && amuse_bvh_format(f, 8, 168, nullptr, status, st) == AMUSE_EINVAL);
    CHECK(amuse_bvh_format(f, 8, 168, t, nullptr, st) == AMUSE_EINVAL);
    for (int off = 1; off < 4; ++off) CHECK(amuse_bvh_format(f, 8, 168, t + off, status, st) == AMUSE_EINVAL);
    CHECK(g_format == 0);
    CHECK(amuse_bvh_format(f, (long long)INT_MAX * 256, 1, t + 4, status, st) == 0 && g_format == 1 && g_format_n == (long long)INT_MAX * 256 && g_stream == st);
    // the exporter
    int dfs[55], F[2] = {3, 5};
    for (int c = 0; c < 55; ++c) dfs[c] = 54 - c;
    auto mo = [&](const float* poses, const float* rr, int S, const int* fr, const int* d, int order, float scale, float* e, void* tx, int* s) {
        return amuse_bvh_motion(poses, nullptr, rr, S, fr, d, order, scale, 0, e, tx, s, st);
    };
    CHECK(mo(f, f, 0, F, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL && mo(f, f, -2, F, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL);
    CHECK(mo(f, f, 2, nullptr, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL);
    {
        int f0[2] = {3, 0}, fneg[2] = {-1, 5}, fbig[2] = {3, amuse::kBvhMaxFrames + 1};
        CHECK(mo(f, f, 2, f0, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL && mo(f, f, 2, fneg, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL);
        CHECK(mo(f, f, 2, fbig, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL);
    }
    CHECK(mo(f, f, 2, F, dfs, -1, 100.f, f, t, status) == AMUSE_EINVAL && mo(f, f, 2, F, dfs, 6, 100.f, f, t, status) == AMUSE_EINVAL);
    {
        int dup[55], range[55];
        for (int c = 0; c < 55; ++c) dup[c] = range[c] = c;
        dup[54] = 0;
        range[3] = 55;
        CHECK(mo(f, f, 2, F, dup, 5, 100.f, f, t, status) == AMUSE_EINVAL && mo(f, f, 2, F, range, 5, 100.f, f, t, status) == AMUSE_EINVAL);
        range[3] = -1;
        CHECK(mo(f, f, 2, F, range, 5, 100.f, f, t, status) == AMUSE_EINVAL && mo(f, f, 2, F, nullptr, 5, 100.f, f, t, status) == AMUSE_EINVAL);
    }
    CHECK(mo(f, f, 2, F, dfs, 5, 0.f, f, t, status) == AMUSE_EINVAL && mo(f, f, 2, F, dfs, 5, -1.f, f, t, status) == AMUSE_EINVAL);
    CHECK(mo(f, f, 2, F, dfs, 5, std::numeric_limits<float>::quiet_NaN(), f, t, status) == AMUSE_EINVAL);
    CHECK(mo(f, f, 2, F, dfs, 5, std::numeric_limits<float>::infinity(), f, t, status) == AMUSE_EINVAL);
    CHECK(mo(nullptr, f, 2, F, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL && mo(f, nullptr, 2, F, dfs, 5, 100.f, f, t, status) == AMUSE_EINVAL);
    CHECK(mo(f, f, 2, F, dfs, 5, 100.f, f, t, nullptr) == AMUSE_EINVAL && mo(f, f, 2, F, dfs, 5, 100.f, nullptr, nullptr, status) == AMUSE_EINVAL);
    CHECK(mo(f, f, 2, F, dfs, 5, 100.f, f, t + 2, status) == AMUSE_EINVAL);
    CHECK(g_motion.empty());
    CHECK(mo(f, f + 8, 2, F, dfs, 4, 2.5f, nullptr, t, status) == 0 && g_motion.size() == 1);
    {
        const amuse::BvhArgs& a = g_motion[0];
        CHECK(a.poses == f && a.trans == nullptr && a.root_rest == f + 8 && a.euler == nullptr && a.text == t && a.status == status && a.scale == 2.5f);
        CHECK(a.ai == 2 && a.aj == 0 && a.ak == 1 && a.e == -1.f && a.unwrap == 0 && a.nseq == 2 && a.max_F == 5);      // ZXY: (k, j, i) = (1, 0, 2), one swap
        CHECK(a.seq[0].row0 == 0 && a.seq[0].F == 3 && a.seq[0].s == 0 && a.seq[1].row0 == 3 && a.seq[1].F == 5 && a.seq[1].s == 1);
        for (int c = 0; c < 55; ++c) CHECK(a.dfs[c] == 54 - c);
    }
    g_motion.clear();
    // the sign of every order: even for XZY, YXZ, ZYX (the reversed triple a cyclic shift of 0, 1, 2)
    const float want_e[6] = {-1.f, 1.f, 1.f, -1.f, -1.f, 1.f};
    const int want_ax[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int o = 0; o < 6; ++o) {
        CHECK(amuse_bvh_motion(f, f, f, 1, F, dfs, o, 1.f, 1, f, nullptr, status, nullptr) == 0);
        const amuse::BvhArgs& a = g_motion.back();
        CHECK(a.ai == want_ax[o][0] && a.aj == want_ax[o][1] && a.ak == want_ax[o][2] && a.e == want_e[o] && a.unwrap == 1 && a.trans == f && a.text == nullptr);
    }
    g_motion.clear();
    // the decoder
    auto de = [&](const float* ch, int S, const int* fr, const int* d, int order, float scale, const float* rr, float* po, float* to) {
        return amuse_bvh_decode(ch, S, fr, d, order, scale, rr, po, to, st);
    };
    CHECK(de(f, 0, F, dfs, 0, 1.f, f, f, f) == AMUSE_EINVAL && de(f, 2, nullptr, dfs, 0, 1.f, f, f, f) == AMUSE_EINVAL && de(f, 2, F, nullptr, 0, 1.f, f, f, f) == AMUSE_EINVAL);
    CHECK(de(f, 2, F, dfs, 6, 1.f, f, f, f) == AMUSE_EINVAL && de(f, 2, F, dfs, 0, 0.f, f, f, f) == AMUSE_EINVAL);
    CHECK(de(nullptr, 2, F, dfs, 0, 1.f, f, f, f) == AMUSE_EINVAL && de(f, 2, F, dfs, 0, 1.f, nullptr, f, f) == AMUSE_EINVAL);
    CHECK(de(f, 2, F, dfs, 0, 1.f, f, nullptr, f) == AMUSE_EINVAL && de(f, 2, F, dfs, 0, 1.f, f, f, nullptr) == AMUSE_EINVAL);
    CHECK(g_decode.empty());
    CHECK(de(f, 2, F, dfs, 3, 4.f, f + 1, f + 2, f + 3) == 0 && g_decode.size() == 1);
    {
        const amuse::BvhDecodeArgs& a = g_decode[0];
        CHECK(a.channels == f && a.root_rest == f + 1 && a.poses_out == f + 2 && a.trans_out == f + 3 && a.scale == 4.f && a.ai == 1 && a.aj == 2 && a.ak == 0);
        CHECK(a.nseq == 2 && a.max_F == 5 && a.seq[1].row0 == 3 && a.seq[1].s == 1 && a.dfs[0] == 54);
    }
    g_decode.clear();
    return 0;
}

static int packing_checks() {
    const int cap = amuse::kSeqPerLaunch;
    float in[4] = {0, 0, 0, 0};      // (never dereferenced: the launchers are stand-ins)
    int status[1] = {0};
    int dfs[55];
    for (int c = 0; c < 55; ++c) dfs[c] = c;
    for (int S : {1, cap - 1, cap, cap + 1, 2 * cap, 3 * cap + 5}) {
        std::vector<int> F(S);
        for (int s = 0; s < S; ++s) F[s] = (s % 7 == 3) ? amuse::kBvhMaxFrames : 1 + (s * 7) % 40;       // long sequences: the byte offsets pass 2^36
        CHECK(amuse_bvh_motion(in, nullptr, in, S, F.data(), dfs, 5, 100.f, 0, in, nullptr, status, nullptr) == 0);
        CHECK(amuse_bvh_decode(in, S, F.data(), dfs, 5, 100.f, in, in, in, nullptr) == 0);
        CHECK((int)g_motion.size() == (S + cap - 1) / cap && g_decode.size() == g_motion.size());
        int s = 0;
        long long row = 0;
        for (size_t k = 0; k < g_motion.size(); ++k) {
            const amuse::BvhArgs& a = g_motion[k];
            const amuse::BvhDecodeArgs& d = g_decode[k];
            CHECK(a.nseq == (k + 1 < g_motion.size() ? cap : S - (int)k * cap) && a.nseq >= 1 && d.nseq == a.nseq);
            int mx = 0;
            for (int q = 0; q < a.nseq; ++q, ++s) {
                CHECK(a.seq[q].row0 == row && a.seq[q].F == F[s] && a.seq[q].s == s);
                CHECK(d.seq[q].row0 == row && d.seq[q].F == F[s] && d.seq[q].s == s);
                row += F[s];
                if (F[s] > mx) mx = F[s];
            }
            CHECK(a.max_F == mx && d.max_F == mx);
            for (int q = a.nseq; q < cap; ++q) CHECK(a.seq[q].row0 == 0 && a.seq[q].F == 0 && d.seq[q].F == 0);   // unused slots are zero
        }
        CHECK(s == S);
        if (S > 8) CHECK(row * amuse::kBvhRowBytes > (1ll << 36));
        g_motion.clear();
        g_decode.clear();
    }
    return 0;
}

int main() {
    static_assert(sizeof(amuse::BvhArgs) <= 4096 && sizeof(amuse::BvhDecodeArgs) <= 4096, "the kernel arguments must fit the 4 KiB argument segment");
    static_assert((long long)amuse::kBvhMaxFrames * amuse::kMotionSlots + amuse::kBvhBlock <= INT_MAX, "a launch's lane index is an int");
    if (int e = layout_checks()) return e;
    if (int e = check_checks()) return e;
    if (int e = packing_checks()) return e;
    puts("bvh_host ok");
    return 0;
}
