// Stand-alone program (its own main): the host half of the long-form candidates - csrc/amuse_seam_host.hpp through the four entry points of csrc/amuse_seam.hip -
// under AddressSanitizer / UBSan on a machine without a GPU.  The kernels' launchers are stand-ins here that keep the argument structs, so the packing of a
// call's sequences into launches can be checked entry by entry:
//   - the plan: seams and workspace bytes, known answers and the refused arguments
//   - the checks of cost / path / select: every refusal returns AMUSE_EINVAL and launches nothing
//   - the packing: S = 1, the per-launch capacity, one more, and several launches' worth - offsets in windows and in seams, the largest seam count of each
//     launch, unused seq[] slots zero; K = 1; single-window sequences mixed in; a call without any seam
// tests/test_seam_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "seam_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amuse_amd/csrc/amuse_seam_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::SeamArgs> g_cost;
static std::vector<amuse::PathArgs> g_path;
static std::vector<amuse::SelectArgs> g_select;
static hipStream_t g_stream = nullptr;
namespace amuse {
hipError_t launch_seam_cost(const SeamArgs& a, hipStream_t s) { g_cost.push_back(a); g_stream = s; return hipSuccess; }
hipError_t launch_seam_path(const PathArgs& a, hipStream_t s) { g_path.push_back(a); g_stream = s; return hipSuccess; }
hipError_t launch_seam_select(const SelectArgs& a, hipStream_t s) { g_select.push_back(a); g_stream = s; return hipSuccess; }
}  // namespace amuse

static bool launched() { return !g_cost.empty() || !g_path.empty() || !g_select.empty(); }

static int plan_checks() {
    long long seams = -1;
    size_t bytes = 1;
    int W2[2] = {3, 1}, W1[1] = {1}, W40[1] = {40}, W3[3] = {3, 2, 4};
    CHECK(amuse_seam_plan(2, W2, 2, 12, 9, &seams, &bytes) == 0 && seams == 2 && bytes == (size_t)2 * 2 * 2 * 3 * 55 * 16);
    CHECK(amuse_seam_plan(1, W1, 4, 300, 270, &seams, &bytes) == 0 && seams == 0 && bytes == 0);
    CHECK(amuse_seam_plan(1, W1, 4, 300, 300, &seams, &bytes) == 0 && seams == 0 && bytes == 0);       // no seam: hop == F is the join's concatenation
    CHECK(amuse_seam_plan(1, W40, 64, 300, 270, &seams, &bytes) == 0 && seams == 39 && bytes == (size_t)39 * 2 * 64 * 30 * 55 * 16);
    CHECK(amuse_seam_plan(3, W3, 5, 300, 150, &seams, &bytes) == 0 && seams == 6 && bytes == (size_t)6 * 2 * 5 * 150 * 55 * 16);
    CHECK(amuse_seam_plan(3, W3, 5, 300, 150, nullptr, nullptr) == 0);                                 // either output is optional
    CHECK(amuse_seam_plan(0, W2, 2, 12, 9, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "S 0"));
    CHECK(amuse_seam_plan(2, nullptr, 2, 12, 9, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "windows"));
    for (int K : {0, -1, 65}) CHECK(amuse_seam_plan(2, W2, K, 12, 9, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "candidates"));
    CHECK(amuse_seam_plan(2, W2, 64, 12, 9, &seams, &bytes) == 0);
    CHECK(amuse_seam_plan(2, W2, 2, 1, 1, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "F 1"));
    for (int hop : {5, 12, 13, 0, -9}) CHECK(amuse_seam_plan(2, W2, 2, 12, hop, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "hop"));   // a seam needs an overlap
    CHECK(amuse_seam_plan(1, W1, 2, 12, 13, &seams, &bytes) == AMUSE_EINVAL && amuse_seam_plan(1, W1, 2, 12, 5, &seams, &bytes) == AMUSE_EINVAL);
    int w0[2] = {3, 0}, wneg[1] = {-2}, wbig[1] = {32769}, wmax[1] = {32768};
    CHECK(amuse_seam_plan(2, w0, 2, 12, 9, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "sequence 1"));
    CHECK(amuse_seam_plan(1, wneg, 2, 12, 9, &seams, &bytes) == AMUSE_EINVAL && amuse_seam_plan(1, wbig, 2, 12, 9, &seams, &bytes) == AMUSE_EINVAL);
    CHECK(amuse_seam_plan(1, wmax, 2, 12, 9, &seams, &bytes) == 0 && seams == 32767);
    int wmax4[4] = {32768, 32768, 32768, 32768};
    CHECK(amuse_seam_plan(4, wmax4, 64, 300, 270, &seams, &bytes) == AMUSE_EINVAL && strstr(g_err, "int indices"));      // 4 x 32768 x 64 x 300 batch frames
    CHECK(!launched());
    return 0;
}

static int cost_checks() {
    std::vector<float> poses((size_t)8 * 12 * 165), trans((size_t)8 * 12 * 3), u(3), w(55);
    std::vector<double> cost(2 * 2 * 2);
    alignas(16) static char ws[2 * 2 * 2 * 3 * 55 * 16];
    int W[2] = {3, 1}, L[2] = {30, 12};
    void* st = reinterpret_cast<void*>(0x40);
    auto call = [&](const float* p, const float* t, int S, const int* wi, const int* l, int K, int F, int hop, const float* rw, const float* jw, float tw, void* work,
                    double* out) { return amuse_seam_cost(p, t, S, wi, l, K, F, hop, rw, jw, tw, work, out, st); };
    const float *P = poses.data(), *T = trans.data(), *U = u.data(), *Jw = w.data();
    CHECK(call(P, T, 0, W, L, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, nullptr, L, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, W, nullptr, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "frames"));
    CHECK(call(P, T, 2, W, L, 0, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, W, L, 65, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, W, L, 2, 1, 1, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, W, L, 2, 12, 5, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);                 // hop < F / 2
    CHECK(call(P, T, 2, W, L, 2, 12, 12, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL);                // hop == F with a seam
    {
        int l18[2] = {18, 12}, l31[2] = {31, 12}, l13[2] = {30, 13}, l0[2] = {30, 0};
        for (const int* l : {l18, l31, l13, l0}) CHECK(call(P, T, 2, W, l, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "do not fit"));
    }
    CHECK(call(nullptr, T, 2, W, L, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "poses"));
    CHECK(call(P, nullptr, 2, W, L, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "trans_weight"));   // no translation: its weight must be 0
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, -1.f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "finite"));
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, __builtin_nanf(""), ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, __builtin_inff(), ws, cost.data()) == AMUSE_EINVAL);
    CHECK(call(P, T, 2, W, L, 2, 12, 9, nullptr, Jw, 0.5f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "row_weight"));
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, nullptr, 0.5f, ws, cost.data()) == AMUSE_EINVAL && strstr(g_err, "joint_weight"));
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, 0.5f, nullptr, cost.data()) == AMUSE_EINVAL && strstr(g_err, "workspace"));
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, 0.5f, ws + 4, cost.data()) == AMUSE_EINVAL && strstr(g_err, "aligned"));
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, 0.5f, ws, nullptr) == AMUSE_EINVAL && strstr(g_err, "cost_out"));
    CHECK(!launched());
    // the accepted call: one launch, both sequences, offsets in windows and in seams
    CHECK(call(P, T, 2, W, L, 2, 12, 9, U, Jw, 0.5f, ws, cost.data()) == 0);
    CHECK(g_cost.size() == 1 && g_stream == static_cast<hipStream_t>(st));
    {
        const amuse::SeamArgs& a = g_cost[0];
        CHECK(a.poses == P && a.trans == T && a.row_weight == U && a.joint_weight == Jw && (void*)a.quats == (void*)ws && a.cost == cost.data() && a.trans_weight == 0.5f);
        CHECK(a.K == 2 && a.F == 12 && a.hop == 9 && a.nseq == 2 && a.max_seams == 2);
        CHECK(a.seq[0].win0 == 0 && a.seq[0].seam0 == 0 && a.seq[0].W == 3 && a.seq[0].L == 30);
        CHECK(a.seq[1].win0 == 3 && a.seq[1].seam0 == 2 && a.seq[1].W == 1 && a.seq[1].L == 12);
    }
    g_cost.clear();
    CHECK(call(P, nullptr, 2, W, L, 1, 12, 9, U, Jw, 0.f, ws, cost.data()) == 0 && g_cost.size() == 1 && g_cost[0].K == 1 && g_cost[0].trans == nullptr);   // K = 1, poses only
    g_cost.clear();
    // no seam in the call: accepted, nothing launched, and nothing but poses and joint_weight asked for
    int w11[2] = {1, 1}, l11[2] = {12, 7};
    CHECK(call(P, nullptr, 2, w11, l11, 2, 12, 9, nullptr, Jw, 0.f, nullptr, nullptr) == 0 && !launched());
    CHECK(call(P, nullptr, 2, w11, l11, 2, 12, 12, nullptr, Jw, 0.f, nullptr, nullptr) == 0 && !launched());
    return 0;
}

static int path_and_select_checks() {
    std::vector<double> cost(8), total(2);
    std::vector<int> choice(8);
    int W[2] = {3, 1};
    CHECK(amuse_seam_path(cost.data(), 0, W, 2, choice.data(), total.data(), nullptr) == AMUSE_EINVAL);
    CHECK(amuse_seam_path(cost.data(), 2, nullptr, 2, choice.data(), total.data(), nullptr) == AMUSE_EINVAL);
    CHECK(amuse_seam_path(cost.data(), 2, W, 0, choice.data(), total.data(), nullptr) == AMUSE_EINVAL && strstr(g_err, "candidates"));
    CHECK(amuse_seam_path(cost.data(), 2, W, 65, choice.data(), total.data(), nullptr) == AMUSE_EINVAL);
    CHECK(amuse_seam_path(nullptr, 2, W, 2, choice.data(), total.data(), nullptr) == AMUSE_EINVAL && strstr(g_err, "cost is NULL"));
    CHECK(amuse_seam_path(cost.data(), 2, W, 2, nullptr, total.data(), nullptr) == AMUSE_EINVAL);
    CHECK(amuse_seam_path(cost.data(), 2, W, 2, choice.data(), nullptr, nullptr) == AMUSE_EINVAL);
    int w0[2] = {3, 0};
    CHECK(amuse_seam_path(cost.data(), 2, w0, 2, choice.data(), total.data(), nullptr) == AMUSE_EINVAL && strstr(g_err, "sequence 1"));
    CHECK(!launched());
    CHECK(amuse_seam_path(cost.data(), 2, W, 2, choice.data(), total.data(), nullptr) == 0 && g_path.size() == 1);
    CHECK(g_path[0].cost == cost.data() && g_path[0].choice == choice.data() && g_path[0].total == total.data() && g_path[0].K == 2 && g_path[0].nseq == 2 && g_path[0].seq0 == 0);
    CHECK(g_path[0].seq[1].win0 == 3 && g_path[0].seq[1].seam0 == 2 && g_path[0].seq[1].W == 1);
    g_path.clear();
    int w11[2] = {1, 1};
    CHECK(amuse_seam_path(nullptr, 2, w11, 4, choice.data(), total.data(), nullptr) == 0 && g_path.size() == 1);    // no seam: no matrix needed, candidate 0 is still written
    g_path.clear();

    // the gather: rows of F = 2 frames
    const int F = 2, per = F * 165;
    std::vector<float> poses((size_t)6 * per), trans((size_t)6 * F * 3), po((size_t)3 * per), to((size_t)3 * F * 3);
    int ch[3] = {1, 2, 5};
    auto sel = [&](const float* p, const float* t, const int* c, int n, int n_in, int f, float* o, float* ot) { return amuse_seam_select(p, t, c, n, n_in, f, o, ot, nullptr); };
    CHECK(sel(poses.data(), trans.data(), ch, 0, 6, F, po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), trans.data(), ch, 3, 0, F, po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, 0, po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(sel(nullptr, trans.data(), ch, 3, 6, F, po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), trans.data(), nullptr, 3, 6, F, po.data(), to.data()) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, nullptr, to.data()) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), nullptr, ch, 3, 6, F, po.data(), to.data()) == AMUSE_EINVAL && strstr(g_err, "NULL together"));
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, po.data(), nullptr) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, poses.data(), to.data()) == AMUSE_EINVAL && strstr(g_err, "overlaps"));           // in place
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, poses.data() + 5 * per + per - 1, to.data()) == AMUSE_EINVAL);                       // the input's last float
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, po.data(), trans.data() + 3) == AMUSE_EINVAL);
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, po.data(), po.data() + per) == AMUSE_EINVAL && strstr(g_err, "poses_out and trans_out"));
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, reinterpret_cast<float*>(ch), to.data()) == AMUSE_EINVAL);                           // over the choice
    CHECK(sel(poses.data(), trans.data(), ch, 2000000, 6, 2000, po.data(), to.data()) == AMUSE_EINVAL && strstr(g_err, "int indices"));
    CHECK(!launched());
    CHECK(sel(poses.data(), trans.data(), ch, 3, 6, F, po.data(), to.data()) == 0 && g_select.size() == 1);
    CHECK(g_select[0].poses == poses.data() && g_select[0].trans == trans.data() && g_select[0].choice == ch && g_select[0].poses_out == po.data() &&
          g_select[0].trans_out == to.data() && g_select[0].n == 3 && g_select[0].n_in == 6 && g_select[0].F == F);
    CHECK(sel(poses.data(), nullptr, ch, 3, 6, F, po.data(), nullptr) == 0 && g_select.size() == 2 && g_select[1].trans == nullptr);
    // adjacent, not overlapping: the output right behind the input
    std::vector<float> both((size_t)9 * per);
    CHECK(sel(both.data(), nullptr, ch, 3, 6, F, both.data() + 6 * per, nullptr) == 0);
    g_select.clear();
    return 0;
}

static int packing_checks() {
    const int cap = amuse::kSeqPerLaunch;
    alignas(16) static float dummy[4] = {0, 0, 0, 0};   // (never dereferenced: the launchers are the stand-ins)
    double ddummy[1] = {0};
    int idummy[1] = {0};
    for (int S : {1, cap - 1, cap, cap + 1, 2 * cap, 3 * cap + 5}) {
        std::vector<int> W(S), L(S);
        for (int s = 0; s < S; ++s) { W[s] = 1 + s % 4; L[s] = (W[s] - 1) * 2 + 1 + (s * 7) % 4; }   // F = 4, hop = 2; every fourth sequence has ONE window
        if (S >= cap) for (int s = cap; s < 2 * cap && s < S; ++s) { W[s] = 1; L[s] = 1 + s % 4; }   // the second launch: single windows only
        CHECK(amuse_seam_cost(dummy, dummy, S, W.data(), L.data(), 3, 4, 2, dummy, dummy, 1.f, dummy, ddummy, nullptr) == 0);
        CHECK(amuse_seam_path(ddummy, S, W.data(), 3, idummy, ddummy, nullptr) == 0);
        const size_t launches = S == 1 ? 0 : (size_t)(S + cap - 1) / cap;    // S = 1 is one window: no seam, the entry point returns before packing
        CHECK(g_cost.size() == launches && g_path.size() == (size_t)(S + cap - 1) / cap);
        int s = 0, win = 0, seam = 0;
        for (size_t k = 0; k < g_path.size(); ++k) {
            const amuse::PathArgs& p = g_path[k];
            CHECK(p.nseq == (k + 1 < g_path.size() ? cap : S - (int)k * cap) && p.nseq >= 1 && p.K == 3 && p.seq0 == (int)k * cap);
            int mx = 0;
            for (int q = 0; q < p.nseq; ++q, ++s) {
                CHECK(p.seq[q].win0 == win && p.seq[q].seam0 == seam && p.seq[q].W == W[s] && p.seq[q].L == 0);
                if (launches) {
                    const amuse::SeamArgs& a = g_cost[k];
                    CHECK(a.seq[q].win0 == win && a.seq[q].seam0 == seam && a.seq[q].W == W[s] && a.seq[q].L == L[s]);
                }
                win += W[s]; seam += W[s] - 1;
                if (W[s] - 1 > mx) mx = W[s] - 1;
            }
            if (launches) {
                const amuse::SeamArgs& a = g_cost[k];
                CHECK(a.nseq == p.nseq && a.K == 3 && a.F == 4 && a.hop == 2 && a.max_seams == mx);
                if (k == 1) CHECK(mx == 0);                                                       // the launcher skips such a launch (k_seam.hip)
                for (int q = a.nseq; q < cap; ++q) CHECK(a.seq[q].W == 0 && a.seq[q].L == 0 && a.seq[q].win0 == 0 && a.seq[q].seam0 == 0);
            }
            for (int q = p.nseq; q < cap; ++q) CHECK(p.seq[q].W == 0 && p.seq[q].win0 == 0 && p.seq[q].seam0 == 0);   // unused slots are zero
        }
        CHECK(s == S);
        g_cost.clear();
        g_path.clear();
    }
    return 0;
}

int main() {
    static_assert(sizeof(amuse::SeamArgs) <= 4096 && sizeof(amuse::PathArgs) <= 4096, "the kernel arguments must fit the 4 KiB argument segment");
    if (int e = plan_checks()) return e;
    if (int e = cost_checks()) return e;
    if (int e = path_and_select_checks()) return e;
    if (int e = packing_checks()) return e;
    puts("seam_host ok");
    return 0;
}
