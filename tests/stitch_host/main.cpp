// Stand-alone program (its own main): the host half of long-form inference - csrc/amuse_stitch_host.hpp through the two entry points of csrc/amuse_stitch.hip -
// under AddressSanitizer / UBSan on a machine without a GPU.  The kernel's launcher is a stand-in here that keeps the argument structs, so the packing of a call's
// sequences into launches can be checked entry by entry:
//   - the window plan: known answers, a sweep against the arithmetic written out again, the last window's audio bound, the refused arguments
//   - the join's checks: every refusal returns AMUSE_EINVAL and launches nothing
//   - the packing: S = 1, the per-launch capacity, one more, and several launches' worth - offsets, counts, the largest sequence of each launch
// tests/test_stitch_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "stitch_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../amuse_amd/csrc/amuse_stitch_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::StitchArgs> g_launches;
static hipStream_t g_stream = nullptr;
namespace amuse {
hipError_t launch_stitch(const StitchArgs& a, hipStream_t s) { g_launches.push_back(a); g_stream = s; return hipSuccess; }
}  // namespace amuse

static int plan_checks() {
    int W = 0, L = 0, hs = 0;
    const struct { long long n; int h, W, L; } known[] = {{160000, 270, 1, 300}, {160534, 270, 2, 301}, {400000, 270, 3, 750}, {400000, 300, 3, 750}, {0, 270, 1, 300}};
    for (const auto& k : known) {
        CHECK(amuse_longform_plan(k.n, k.h, &W, &L, &hs) == 0 && W == k.W && L == k.L && hs == k.h / 3 * 1600);
    }
    CHECK(amuse_longform_plan(400000, 270, nullptr, nullptr, nullptr) == 0);   // every output is optional
    for (int h : {271, 147, 303, 0, -270, 149, 301}) CHECK(amuse_longform_plan(400000, h, &W, &L, &hs) == AMUSE_EINVAL);
    CHECK(amuse_longform_plan(-1, 270, &W, &L, &hs) == AMUSE_EINVAL);
    CHECK(amuse_longform_plan(1LL << 62, 270, &W, &L, &hs) == AMUSE_EINVAL);     // 3 n would overflow
    CHECK(amuse_longform_plan((long long)2147483647 / 3 * 1600, 300, &W, &L, &hs) == 0 && L == 2147483647 / 3 * 3);
    for (int h : {150, 180, 270, 300})
        for (long long n = 0; n <= 1000000; n += 533) {
            CHECK(amuse_longform_plan(n, h, &W, &L, &hs) == 0);
            const long long fl = 3 * n / 1600, Lr = fl < 300 ? 300 : fl;
            long long Wr = 1;
            while ((Wr - 1) * h + 300 < Lr) ++Wr;                                // the fewest windows that cover L frames
            CHECK(L == Lr && W == Wr && hs * 3 == h * 1600);
            CHECK((long long)(W - 1) * h < L && L <= (long long)(W - 1) * h + 300);   // what amuse_stitch_windows asks of (W, L)
            if (W > 1) CHECK((n - (long long)(W - 1) * hs) * 3 > (long long)(300 - h) * 1600);   // the last window holds more than 300 - h frames of audio
            if (n <= 160000) CHECK(W == 1 && L == 300);
        }
    return 0;
}

static int stitch_checks() {
    std::vector<float> poses((size_t)4 * 12 * 165), trans((size_t)4 * 12 * 3), blend(3), po((size_t)40 * 165), to((size_t)40 * 3);
    int W[2] = {3, 1}, L[2] = {30, 12};
    void* st = reinterpret_cast<void*>(0x40);
    auto call = [&](const float* p, const float* t, int S, const int* w, const int* l, int F, int hop, const float* b, float* o, float* ot) {
        return amuse_stitch_windows(p, t, S, w, l, F, hop, b, o, ot, st);
    };
    CHECK(call(poses.data(), trans.data(), 0, W, L, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, W, L, 1, 1, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, W, L, 12, 5, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);     // hop < F / 2
    CHECK(call(poses.data(), trans.data(), 2, W, L, 12, 13, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);    // hop > F
    CHECK(call(poses.data(), trans.data(), 2, nullptr, L, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, W, nullptr, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(call(nullptr, trans.data(), 2, W, L, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, W, L, 12, 9, blend.data(), nullptr, to.data()) == AMUSE_EINVAL);
    CHECK(call(poses.data(), trans.data(), 2, W, L, 12, 9, nullptr, po.data(), to.data()) == AMUSE_EINVAL);           // an overlap needs its weights
    CHECK(call(poses.data(), nullptr, 2, W, L, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);           // the trans pair: both or neither
    CHECK(call(poses.data(), trans.data(), 2, W, L, 12, 9, blend.data(), po.data(), nullptr) == AMUSE_EINVAL);
    {
        int w0[2] = {0, 1}, l18[2] = {18, 12}, l31[2] = {31, 12}, l0[2] = {30, 0}, l13[2] = {30, 13}, wneg[2] = {3, -1};
        CHECK(call(poses.data(), trans.data(), 2, w0, L, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
        CHECK(call(poses.data(), trans.data(), 2, wneg, L, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
        CHECK(call(poses.data(), trans.data(), 2, W, l18, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);   // L == (W - 1) hop: the last window would be empty
        CHECK(call(poses.data(), trans.data(), 2, W, l31, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);   // one frame more than the windows hold
        CHECK(call(poses.data(), trans.data(), 2, W, l0, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
        CHECK(call(poses.data(), trans.data(), 2, W, l13, 12, 9, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);
        int wmid[1] = {200000}, lmid[1] = {199999 * 200 + 1};
        CHECK(call(poses.data(), trans.data(), 1, wmid, lmid, 400, 200, blend.data(), po.data(), to.data()) == AMUSE_EINVAL);     // 56 threads per frame beyond an int
    }
    CHECK(g_launches.empty());                                                    // nothing refused reached the launcher
    // the accepted call: one launch, both sequences, offsets in windows and frames
    CHECK(call(poses.data(), trans.data(), 2, W, L, 12, 9, blend.data(), po.data(), to.data()) == 0);
    CHECK(g_launches.size() == 1 && g_stream == static_cast<hipStream_t>(st));
    {
        const amuse::StitchArgs& a = g_launches[0];
        CHECK(a.poses == poses.data() && a.trans == trans.data() && a.blend == blend.data() && a.poses_out == po.data() && a.trans_out == to.data());
        CHECK(a.F == 12 && a.hop == 9 && a.nseq == 2 && a.max_L == 30);
        CHECK(a.seq[0].win0 == 0 && a.seq[0].out0 == 0 && a.seq[0].W == 3 && a.seq[0].L == 30);
        CHECK(a.seq[1].win0 == 3 && a.seq[1].out0 == 30 && a.seq[1].W == 1 && a.seq[1].L == 12);
    }
    g_launches.clear();
    // the shortest and the longest L a window count takes; poses only; hop == F needs no weights
    int w3[1] = {3}, lmin[1] = {19}, lmax[1] = {30}, l36[1] = {36};
    CHECK(call(poses.data(), nullptr, 1, w3, lmin, 12, 9, blend.data(), po.data(), nullptr) == 0 && g_launches.back().trans == nullptr && g_launches.back().max_L == 19);
    CHECK(call(poses.data(), nullptr, 1, w3, lmax, 12, 9, blend.data(), po.data(), nullptr) == 0);
    CHECK(call(poses.data(), nullptr, 1, w3, l36, 12, 12, nullptr, po.data(), nullptr) == 0 && g_launches.size() == 3);
    g_launches.clear();
    return 0;
}

static int packing_checks() {
    const int cap = amuse::kSeqPerLaunch;
    float dummy[4] = {0, 0, 0, 0};   // (never dereferenced: the launcher is the stand-in)
    for (int S : {1, cap - 1, cap, cap + 1, 2 * cap, 3 * cap + 5}) {
        std::vector<int> W(S), L(S);
        for (int s = 0; s < S; ++s) { W[s] = 1 + s % 4; L[s] = (W[s] - 1) * 2 + 1 + (s * 7) % 4; }   // F = 4, hop = 2: (W - 1) 2 < L <= (W - 1) 2 + 4
        CHECK(amuse_stitch_windows(dummy, dummy, S, W.data(), L.data(), 4, 2, dummy, dummy, dummy, nullptr) == 0);
        CHECK((int)g_launches.size() == (S + cap - 1) / cap);
        int s = 0, win = 0, out = 0;
        for (size_t k = 0; k < g_launches.size(); ++k) {
            const amuse::StitchArgs& a = g_launches[k];
            CHECK(a.nseq == (k + 1 < g_launches.size() ? cap : S - (int)k * cap) && a.nseq >= 1 && a.F == 4 && a.hop == 2);
            int mx = 0;
            for (int q = 0; q < a.nseq; ++q, ++s) {
                CHECK(a.seq[q].win0 == win && a.seq[q].out0 == out && a.seq[q].W == W[s] && a.seq[q].L == L[s]);
                win += W[s]; out += L[s];
                if (L[s] > mx) mx = L[s];
            }
            CHECK(a.max_L == mx);
            for (int q = a.nseq; q < cap; ++q) CHECK(a.seq[q].W == 0 && a.seq[q].L == 0);   // unused slots are zero, not left over from the launch before
        }
        CHECK(s == S);
        g_launches.clear();
    }
    return 0;
}

int main() {
    static_assert(sizeof(amuse::StitchArgs) <= 4096, "the kernel arguments must fit the 4 KiB argument segment");
    if (int e = plan_checks()) return e;
    if (int e = stitch_checks()) return e;
    if (int e = packing_checks()) return e;
    puts("stitch_host ok");
    return 0;
}
