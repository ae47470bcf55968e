// Stand-alone program (its own main): the host half of motion smoothing - csrc/amuse_smooth_host.hpp through the two entry points of csrc/amuse_smooth.hip -
// under AddressSanitizer / UBSan on a machine without a GPU.  The kernel's launcher is a stand-in here that keeps the argument structs, so the packing of a call's
// sequences into launches can be checked entry by entry:
//   - the bank: the refused arguments, the layout, known coefficients, rows that sum to 1, symmetry, idempotence (H H = H), H = I where the fit interpolates
//   - the filter's checks: every refusal returns AMUSE_EINVAL and launches nothing; the overlap check on every pair of an output and an input range
//   - the packing: S = 1, the per-launch capacity, one more, and several launches' worth - offsets, counts, the largest sequence, the halo, the half-windows
// tests/test_smooth_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "smooth_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "../../amuse_amd/csrc/amuse_smooth_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::SmoothArgs> g_launches;
static hipStream_t g_stream = nullptr;
namespace amuse {
hipError_t launch_smooth(const SmoothArgs& a, hipStream_t s) { g_launches.push_back(a); g_stream = s; return hipSuccess; }
}  // namespace amuse

static int bank_checks() {
    std::vector<float> bk(AMUSE_SMOOTH_BANK_FLOATS + 1, -77.f);      // (one float of guard behind the bank)
    CHECK(amuse_smooth_banks(-1, bk.data()) == AMUSE_EINVAL && amuse_smooth_banks(6, bk.data()) == AMUSE_EINVAL && amuse_smooth_banks(3, nullptr) == AMUSE_EINVAL);
    CHECK(bk[0] == -77.f);                                           // a refused call writes nothing
    for (int order = 0; order <= 5; ++order) {
        CHECK(amuse_smooth_banks(order, bk.data()) == 0 && bk[AMUSE_SMOOTH_BANK_FLOATS] == -77.f);
        int off = 0;
        for (int m = 1; m <= AMUSE_SMOOTH_MAX_HALF; ++m) {
            const int n = 2 * m + 1, pm = order < 2 * m ? order : 2 * m;
            CHECK(off == amuse::smooth_bank_offset(m));
            const float* H = bk.data() + off;
            for (int r = 0; r < n; ++r) {
                double sum = 0.0;
                for (int k = 0; k < n; ++k) {
                    sum += H[r * n + k];
                    CHECK(std::fabs(H[r * n + k] - H[k * n + r]) <= 1e-6);                           // symmetric
                    CHECK(std::fabs(H[r * n + k] - H[(n - 1 - r) * n + (n - 1 - k)]) <= 1e-6);       // and the same read from the other end
                    if (pm == 2 * m) CHECK(std::fabs(H[r * n + k] - (r == k ? 1.f : 0.f)) <= 1e-6);  // as many coefficients as points: the fit interpolates
                    double hh = 0.0;
                    for (int i = 0; i < n; ++i) hh += (double)H[r * n + i] * H[i * n + k];
                    CHECK(std::fabs(hh - H[r * n + k]) <= 1e-5);                                     // a projection
                }
                CHECK(std::fabs(sum - 1.0) <= 1e-6);
            }
            if (order == 0)
                for (int i = 0; i < n * n; ++i) CHECK(std::fabs(H[i] - 1.0 / n) <= 1e-7);            // order 0: the moving average
            off += n * n;
        }
        CHECK(off == AMUSE_SMOOTH_BANK_FLOATS);
    }
    CHECK(amuse_smooth_banks(3, bk.data()) == 0);
    const double w9[9] = {-21, 14, 39, 54, 59, 54, 39, 14, -21};     // window 9, order 3: the classic central kernel, / 231
    for (int k = 0; k < 9; ++k) CHECK(std::fabs(bk[amuse::smooth_bank_offset(4) + 4 * 9 + k] - w9[k] / 231.0) <= 1e-7);
    const double w5[5] = {-3, 12, 17, 12, -3};                       // window 5, order 2 or 3: / 35
    for (int k = 0; k < 5; ++k) CHECK(std::fabs(bk[amuse::smooth_bank_offset(2) + 2 * 5 + k] - w5[k] / 35.0) <= 1e-7);
    return 0;
}

static int smooth_checks() {
    const int total = 40;
    std::vector<float> poses((size_t)2 * total * 165), trans((size_t)2 * total * 3), banks(AMUSE_SMOOTH_BANK_FLOATS);
    float* po = poses.data() + (size_t)total * 165;      // the second half of each buffer: an output range that touches its input range without overlapping it
    float* to = trans.data() + (size_t)total * 3;
    int L[2] = {28, 12};
    unsigned char hw[56];
    for (int i = 0; i < 56; ++i) hw[i] = (unsigned char)(i % 5);
    hw[55] = 7;
    void* st = reinterpret_cast<void*>(0x40);
    auto call = [&](const float* p, const float* t, int S, const int* l, const unsigned char* h, const float* b, float* o, float* ot) {
        return amuse_smooth_motion(p, t, S, l, h, b, o, ot, st);
    };
    CHECK(call(poses.data(), trans.data(), 0, L, hw, banks.data(), po, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), -3, L, hw, banks.data(), po, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, nullptr, hw, banks.data(), po, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, nullptr, banks.data(), po, to) == AMUSE_EINVAL);
    CHECK(call(nullptr, trans.data(), 2, L, hw, banks.data(), po, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, hw, nullptr, po, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), nullptr, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), nullptr, 2, L, hw, banks.data(), po, to) == AMUSE_EINVAL);              // the trans pair: both or neither
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), po, nullptr) == AMUSE_EINVAL);
    {
        int l0[2] = {28, 0}, lneg[2] = {-1, 12};
        CHECK(call(poses.data(), trans.data(), 2, l0, hw, banks.data(), po, to) == AMUSE_EINVAL);
        CHECK(call(poses.data(), trans.data(), 2, lneg, hw, banks.data(), po, to) == AMUSE_EINVAL);
        unsigned char hbad[56];
        for (int i = 0; i < 56; ++i) hbad[i] = 15;
        hbad[55] = 16;
        CHECK(call(poses.data(), trans.data(), 2, L, hbad, banks.data(), po, to) == AMUSE_EINVAL);
        hbad[55] = 15; hbad[0] = 255;
        CHECK(call(poses.data(), trans.data(), 2, L, hbad, banks.data(), po, to) == AMUSE_EINVAL);
        int lbig[2] = {2147483647 / 56, 1}, lhuge[3] = {2147483647, 2147483647, 2147483647};         // 56 x frames beyond an int; the sum itself beyond an int
        CHECK(call(poses.data(), nullptr, 2, lbig, hw, banks.data(), po, nullptr) == AMUSE_EINVAL);
        CHECK(call(poses.data(), nullptr, 3, lhuge, hw, banks.data(), po, nullptr) == AMUSE_EINVAL);
    }
    // overlap: in place, shifted by a frame either way, the last float of one on the first of the other; an output on the OTHER input
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), poses.data(), to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), po, trans.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), poses.data() + 165, to) == AMUSE_EINVAL);
    CHECK(call(poses.data() + 165, trans.data(), 2, L, hw, banks.data(), poses.data(), to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), po - 1, to) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), po, to - 1) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data() + 3, 2, L, hw, banks.data(), po, trans.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), poses.data() + (size_t)total * 165 + 30, 2, L, hw, banks.data(), po, to) == AMUSE_EINVAL);       // trans inside poses_out
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), po, poses.data() + 5) == AMUSE_EINVAL);                      // trans_out inside poses
    CHECK(call(poses.data(), nullptr, 2, L, hw, banks.data(), poses.data(), nullptr) == AMUSE_EINVAL);
    CHECK(g_launches.empty());                                                    // nothing refused reached the launcher
    // the accepted call: ranges that touch; one launch, both sequences, offsets in frames
    CHECK(call(poses.data(), trans.data(), 2, L, hw, banks.data(), po, to) == 0);
    CHECK(g_launches.size() == 1 && g_stream == static_cast<hipStream_t>(st));
    {
        const amuse::SmoothArgs& a = g_launches[0];
        CHECK(a.poses == poses.data() && a.trans == trans.data() && a.banks == banks.data() && a.poses_out == po && a.trans_out == to);
        CHECK(a.nseq == 2 && a.max_L == 28 && a.halo == 7);
        CHECK(a.seq[0].row0 == 0 && a.seq[0].L == 28 && a.seq[1].row0 == 28 && a.seq[1].L == 12);
        for (int i = 0; i < 56; ++i) CHECK(a.hw[i] == hw[i]);
    }
    g_launches.clear();
    // poses only: the translation's half-window loads no halo; all half-windows 0 is a copy and still one launch
    CHECK(call(poses.data(), nullptr, 2, L, hw, banks.data(), po, nullptr) == 0 && g_launches.back().trans == nullptr && g_launches.back().halo == 4);
    unsigned char h0[56] = {0};
    CHECK(call(poses.data(), trans.data(), 2, L, h0, banks.data(), po, to) == 0 && g_launches.back().halo == 0 && g_launches.size() == 2);
    g_launches.clear();
    return 0;
}

static int packing_checks() {
    const int cap = amuse::kSeqPerLaunch;
    float in[4] = {0, 0, 0, 0};      // (never dereferenced: the launcher is the stand-in; the ranges are far apart)
    float* out = reinterpret_cast<float*>(static_cast<uintptr_t>(1) << 40);
    float* tout = reinterpret_cast<float*>(static_cast<uintptr_t>(1) << 41);
    const float* tin = reinterpret_cast<const float*>(static_cast<uintptr_t>(1) << 42);
    unsigned char hw[56];
    for (int i = 0; i < 56; ++i) hw[i] = 15;
    for (int S : {1, cap - 1, cap, cap + 1, 2 * cap, 3 * cap + 5}) {
        std::vector<int> L(S);
        for (int s = 0; s < S; ++s) L[s] = 1 + (s * 7) % 40;
        CHECK(amuse_smooth_motion(in, tin, S, L.data(), hw, in, out, tout, nullptr) == 0);
        CHECK((int)g_launches.size() == (S + cap - 1) / cap);
        int s = 0, row = 0;
        for (size_t k = 0; k < g_launches.size(); ++k) {
            const amuse::SmoothArgs& a = g_launches[k];
            CHECK(a.nseq == (k + 1 < g_launches.size() ? cap : S - (int)k * cap) && a.nseq >= 1 && a.halo == 15 && a.hw[55] == 15);
            int mx = 0;
            for (int q = 0; q < a.nseq; ++q, ++s) {
                CHECK(a.seq[q].row0 == row && a.seq[q].L == L[s]);
                row += L[s];
                if (L[s] > mx) mx = L[s];
            }
            CHECK(a.max_L == mx);
            for (int q = a.nseq; q < cap; ++q) CHECK(a.seq[q].row0 == 0 && a.seq[q].L == 0);   // unused slots are zero, not left over from the launch before
        }
        CHECK(s == S);
        g_launches.clear();
    }
    return 0;
}

int main() {
    static_assert(sizeof(amuse::SmoothArgs) <= 4096, "the kernel arguments must fit the 4 KiB argument segment");
    static_assert(amuse::kSmoothLdsRows * amuse::kMotionSlots * 16 <= 64 * 1024, "the quaternion tile must fit a workgroup's LDS");
    if (int e = bank_checks()) return e;
    if (int e = smooth_checks()) return e;
    if (int e = packing_checks()) return e;
    puts("smooth_host ok");
    return 0;
}
