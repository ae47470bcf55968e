// Stand-alone program (its own main): the host half of the motion metrics - csrc/amuse_motion_metrics_host.hpp through the two entry points of
// csrc/amuse_motion_metrics.hip - under AddressSanitizer / UBSan on a machine without a GPU.  The kernel's launcher is a stand-in here that keeps the argument
// struct, so what a call hands to the launch can be checked field by field:
//   - the row: 442 doubles, the block offsets of include/amuse_hip.h's table add up
//   - the checks: every refusal returns AMUSE_EINVAL, names what it refused and launches nothing - NULL pointers, N < 1, F < 2, sizes beyond an int
//   - the launch arithmetic: one launch per call whatever N is, pointers / N / F / stream passed through, the workgroup's LDS and the 4 KiB argument segment
// tests/test_motion_metrics_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "motion_metrics_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amuse_amd/csrc/amuse_motion_metrics_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::MotionMetricsArgs> g_launches;
static hipStream_t g_stream = nullptr;
static hipError_t g_result = hipSuccess;
namespace amuse {
hipError_t launch_motion_metrics(const MotionMetricsArgs& a, hipStream_t s) { g_launches.push_back(a); g_stream = s; return g_result; }
}  // namespace amuse

static int row_checks() {
    using namespace amuse;
    CHECK(amuse_motion_metrics_row() == 442 && kMetricsRow == 442);
    const int off[] = {kRowApeRoot, kRowApeTraj, kRowApePose, kRowApeJoints, kRowAveRoot, kRowAveTraj, kRowAvePose, kRowAveJoints, kRowVelGen, kRowVelRef, kRowAccGen, kRowAccRef};
    const int len[] = {1, 1, 54, 55, 1, 1, 54, 55, 55, 55, 55, 55};
    const int want[] = {0, 1, 2, 56, 111, 112, 113, 167, 222, 277, 332, 387};      // include/amuse_hip.h's table
    int at = 0;
    for (int k = 0; k < 12; ++k) {
        CHECK(off[k] == at && off[k] == want[k]);
        at += len[k];
    }
    CHECK(at == kMetricsRow);
    return 0;
}

static int refusal_checks() {
    std::vector<float> G((size_t)3 * 5 * 165), R(G.size());
    std::vector<double> rows((size_t)3 * 442);
    int len[3] = {5, 5, 5};       // (stands in for a device pointer: the host code never reads it)
    void* st = reinterpret_cast<void*>(0x40);
    auto call = [&](const float* g, const float* r, const int* l, int N, int F, double* o) { g_err[0] = 0; return amuse_motion_metrics(g, r, l, N, F, o, st); };
    CHECK(call(nullptr, R.data(), len, 3, 5, rows.data()) == AMUSE_EINVAL && strstr(g_err, "joints_gen"));
    CHECK(call(G.data(), nullptr, len, 3, 5, rows.data()) == AMUSE_EINVAL && strstr(g_err, "joints_ref"));
    CHECK(call(G.data(), R.data(), nullptr, 3, 5, rows.data()) == AMUSE_EINVAL && strstr(g_err, "lengths_dev"));
    CHECK(call(G.data(), R.data(), len, 3, 5, nullptr) == AMUSE_EINVAL && strstr(g_err, "rows_out"));
    for (int N : {0, -1, INT_MIN}) CHECK(call(G.data(), R.data(), len, N, 5, rows.data()) == AMUSE_EINVAL && strstr(g_err, "N "));
    for (int F : {1, 0, -300, INT_MIN}) CHECK(call(G.data(), R.data(), len, 3, F, rows.data()) == AMUSE_EINVAL && strstr(g_err, "F "));
    // sizes beyond an int: N F frames, and 442 N row entries (the products are formed in 64 bits: nothing here may overflow under UBSan)
    CHECK(call(G.data(), R.data(), len, INT_MAX, INT_MAX, rows.data()) == AMUSE_EINVAL && strstr(g_err, "an int"));
    CHECK(call(G.data(), R.data(), len, 1 << 20, 1 << 11, rows.data()) == AMUSE_EINVAL);                 // N F = 2^31
    CHECK(call(G.data(), R.data(), len, INT_MAX / 442 + 1, 2, rows.data()) == AMUSE_EINVAL);             // 442 N just beyond
    CHECK(g_launches.empty());                                                                            // nothing refused reached the launcher
    return 0;
}

static int launch_checks() {
    float g = 0, r = 0;
    double o = 0;
    int l = 0;                    // (never dereferenced: the launcher is the stand-in)
    void* st = reinterpret_cast<void*>(0x80);
    const struct { int N, F; } ok[] = {{1, 2}, {3, 5}, {256, 300}, {INT_MAX / 442, 2}, {INT_MAX / 442, 300}, {4, INT_MAX / 4}, {1, INT_MAX}};      // the largest N (442 N binds below F = 442); the largest F
    size_t k = 0;
    for (const auto& c : ok) {
        CHECK(amuse_motion_metrics(&g, &r, &l, c.N, c.F, &o, st) == AMUSE_OK);
        CHECK(g_launches.size() == ++k && g_stream == static_cast<hipStream_t>(st));                      // ONE launch, whatever N is: the grid is the clips
        const amuse::MotionMetricsArgs& a = g_launches.back();
        CHECK(a.gen == &g && a.ref == &r && a.lengths == &l && a.rows == &o && a.N == c.N && a.F == c.F);
        CHECK((long long)a.N * a.F <= INT_MAX && (long long)a.N * amuse::kMetricsRow <= INT_MAX);
    }
    CHECK(amuse_motion_metrics(&g, &r, &l, 2, 2, &o, nullptr) == AMUSE_OK && g_stream == nullptr);         // the null stream is a stream
    g_result = hipErrorInvalidConfiguration;                                                              // a launch the runtime refuses comes back as AMUSE_EHIP
    CHECK(amuse_motion_metrics(&g, &r, &l, 2, 2, &o, nullptr) == AMUSE_EHIP && strstr(g_err, "launch failed"));
    g_result = hipSuccess;
    g_launches.clear();
    return 0;
}

int main() {
    static_assert(sizeof(amuse::MotionMetricsArgs) <= 4096, "the kernel arguments must fit the 4 KiB argument segment");
    static_assert(amuse::kMetricsBlock == 512 && amuse::kMetricsBlock <= 1024, "a workgroup of eight waves");
    static_assert(amuse::kMetricsLdsBytes == 77824 && amuse::kMetricsLdsBytes <= 160 * 1024, "the partials of eight waves fit the 160 KiB of LDS of a CU");
    static_assert(amuse::kSmplxJoints <= 64, "a lane per joint");
    if (int e = row_checks()) return e;
    if (int e = refusal_checks()) return e;
    if (int e = launch_checks()) return e;
    puts("motion_metrics_host ok");
    return 0;
}
