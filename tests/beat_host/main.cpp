// Stand-alone program (its own main): the host half of the beat alignment - csrc/amuse_beat_host.hpp through the entry points of csrc/amuse_beat.hip - under
// AddressSanitizer / UBSan on a machine without a GPU, on the stubbed HIP runtime of tests/host_asan.  The kernels' launchers are stand-ins here that keep the
// argument structs, so what a call hands to its launches can be checked field by field:
//   - amuse_beat_plan on its edge values; the defaults; the row: 166 doubles, the block offsets of include/amuse_hip.h's table add up
//   - every AMUSE_EINVAL of the parameter checks (through each of the three calls that take parameters) and of the argument checks; nothing refused launches
//   - the context: create / reserve / destroy leave nothing behind (LeakSanitizer), reserve grows only and keeps what it outgrew until destroy
//   - the launch arithmetic: runs = ceil(T / 16), the pick stage fed with the envelope the call wrote, T == 0 launches nothing
// tests/test_beat_host_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "beat_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../amuse_amd/csrc/amuse_beat_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::BeatEnvArgs> g_env;
static std::vector<amuse::BeatPickArgs> g_pick;
static std::vector<amuse::BeatAlignArgs> g_align;
static hipStream_t g_stream = nullptr;
static hipError_t g_result = hipSuccess;
namespace amuse {
hipError_t launch_beat_envelope(const BeatEnvArgs& a, hipStream_t s) { g_env.push_back(a); g_stream = s; return g_result; }
hipError_t launch_beat_pick(const BeatPickArgs& a, hipStream_t s) { g_pick.push_back(a); g_stream = s; return g_result; }
hipError_t launch_beat_align(const BeatAlignArgs& a, hipStream_t s) { g_align.push_back(a); g_stream = s; return g_result; }
}  // namespace amuse

static size_t launches() { return g_env.size() + g_pick.size() + g_align.size(); }

static int plan_and_row_checks() {
    using namespace amuse;
    const struct { long long n; int T; } plan[] = {{0, 0}, {1, 0}, {399, 0}, {400, 1}, {559, 1}, {560, 2}, {3120, 18}, {32000, 198}, {160000, 998}, {170000, 1061},
                                                   {1920000, 11998}, {400LL + 160LL * (INT_MAX - 1LL), INT_MAX}};
    for (const auto& c : plan) {
        int T = -7;
        CHECK(amuse_beat_plan(c.n, &T) == AMUSE_OK && T == c.T);
        CHECK(amuse_beat_plan(c.n, nullptr) == AMUSE_OK);
    }
    int T = -7;
    CHECK(amuse_beat_plan(-1, &T) == AMUSE_EINVAL && T == -7 && strstr(g_err, "n_samples"));
    CHECK(amuse_beat_plan(400LL + 160LL * (long long)INT_MAX, &T) == AMUSE_EINVAL && strstr(g_err, "an int"));
    CHECK(amuse_beat_plan(LLONG_MAX, &T) == AMUSE_EINVAL);
    amuse_beat_params p;
    CHECK(amuse_beat_default_params(nullptr) == AMUSE_EINVAL);
    CHECK(amuse_beat_default_params(&p) == AMUSE_OK);
    CHECK(p.sigma_s == 0.1 && p.onset_delta == 0.07 && p.onset_window == 3 && p.onset_avg_window == 10 && p.motion_order == 3 && p.fps == 30.0);
    CHECK(amuse_beat_align_row() == 166 && kBeatRow == 166);
    const int off[] = {kBeatRowOnsets, kBeatRowBeats, kBeatRowA2M, kBeatRowM2A}, len[] = {1, 55, 55, 55}, want[] = {0, 1, 56, 111};   // include/amuse_hip.h's table
    int at = 0;
    for (int k = 0; k < 4; ++k) {
        CHECK(off[k] == at && off[k] == want[k]);
        at += len[k];
    }
    CHECK(at == kBeatRow);
    return 0;
}

// every refusal of the parameter checks, through a call that would otherwise launch
template <class Call>
static int param_refusals(Call call) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    amuse_beat_params d;
    amuse_beat_default_params(&d);
    auto bad = [&](amuse_beat_params p, const char* word) { g_err[0] = 0; return call(&p) == AMUSE_EINVAL && strstr(g_err, word) != nullptr; };
    amuse_beat_params p;
    for (double v : {0.0, -0.1, nan, inf}) { p = d; p.sigma_s = v; CHECK(bad(p, "sigma_s")); }
    for (double v : {-1e-9, nan, inf}) { p = d; p.onset_delta = v; CHECK(bad(p, "onset_delta")); }
    for (int v : {0, -1, INT_MIN}) { p = d; p.onset_window = v; CHECK(bad(p, "onset_window")); }
    for (int v : {0, -1, INT_MIN}) { p = d; p.onset_avg_window = v; CHECK(bad(p, "onset_avg_window")); }
    for (int v : {0, -1, 33, INT_MAX}) { p = d; p.motion_order = v; CHECK(bad(p, "motion_order")); }
    for (double v : {0.0, -30.0, nan, inf}) { p = d; p.fps = v; CHECK(bad(p, "fps")); }
    p = d; p.onset_delta = 0.0; p.onset_window = INT_MAX; p.onset_avg_window = INT_MAX; p.motion_order = 32;      // the edges that pass
    g_err[0] = 0;
    CHECK(call(&p) == AMUSE_OK);
    CHECK(call(nullptr) == AMUSE_OK);                                                                             // NULL: the defaults
    return 0;
}

static int refusal_checks(amuse_beat* ctx) {
    float x = 0;
    unsigned char m = 0;
    int i = 0;
    double r = 0;                 // (stand in for device pointers: the host code never reads them)
    void* st = reinterpret_cast<void*>(0x40);
    // ---- onsets
    CHECK(amuse_beat_onsets(nullptr, &x, nullptr, 400, 1, nullptr, &x, &m, st) == AMUSE_EINVAL && strstr(g_err, "ctx"));
    CHECK(amuse_beat_onsets(ctx, nullptr, nullptr, 400, 1, nullptr, &x, &m, st) == AMUSE_EINVAL && strstr(g_err, "waves_dev"));
    CHECK(amuse_beat_onsets(ctx, &x, nullptr, 400, 1, nullptr, nullptr, nullptr, st) == AMUSE_EINVAL && strstr(g_err, "both NULL"));
    for (int B : {0, -1, INT_MIN}) CHECK(amuse_beat_onsets(ctx, &x, nullptr, 400, B, nullptr, &x, &m, st) == AMUSE_EINVAL && strstr(g_err, "B "));
    for (int n : {0, -1, INT_MIN}) CHECK(amuse_beat_onsets(ctx, &x, nullptr, n, 1, nullptr, &x, &m, st) == AMUSE_EINVAL && strstr(g_err, "n_samples"));
    CHECK(amuse_beat_onsets(ctx, &x, nullptr, INT_MAX, 1024, nullptr, &x, &m, st) == AMUSE_EINVAL && strstr(g_err, "an int"));
    CHECK(amuse_beat_onsets(ctx, &x, nullptr, 400, 1, nullptr, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "amuse_beat_reserve"));      // nothing reserved yet
    // ---- pick
    CHECK(amuse_beat_pick(nullptr, &i, 1, 5, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "envelope_dev"));
    CHECK(amuse_beat_pick(&x, nullptr, 1, 5, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "frames_dev"));
    CHECK(amuse_beat_pick(&x, &i, 1, 5, nullptr, nullptr, st) == AMUSE_EINVAL && strstr(g_err, "onset_mask_out"));
    for (int B : {0, -1}) CHECK(amuse_beat_pick(&x, &i, B, 5, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "B "));
    for (int T : {0, -1}) CHECK(amuse_beat_pick(&x, &i, 1, T, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "T "));
    CHECK(amuse_beat_pick(&x, &i, 1 << 16, 1 << 15, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "an int"));
    // ---- align
    auto al = [&](const unsigned char* om, const int* af, int T, const float* J, const int* L, int N, int F, double* rows) {
        g_err[0] = 0;
        return amuse_beat_align(om, af, T, J, L, N, F, nullptr, rows, nullptr, st);
    };
    CHECK(al(nullptr, &i, 5, &x, &i, 1, 2, &r) == AMUSE_EINVAL && strstr(g_err, "onset_mask_dev"));
    CHECK(al(&m, nullptr, 5, &x, &i, 1, 2, &r) == AMUSE_EINVAL && strstr(g_err, "audio_frames_dev"));
    CHECK(al(&m, &i, 5, nullptr, &i, 1, 2, &r) == AMUSE_EINVAL && strstr(g_err, "joints"));
    CHECK(al(&m, &i, 5, &x, nullptr, 1, 2, &r) == AMUSE_EINVAL && strstr(g_err, "lengths_dev"));
    CHECK(al(&m, &i, 5, &x, &i, 1, 2, nullptr) == AMUSE_EINVAL && strstr(g_err, "rows_out"));
    for (int N : {0, -1}) CHECK(al(&m, &i, 5, &x, &i, N, 2, &r) == AMUSE_EINVAL && strstr(g_err, "N "));
    for (int F : {1, 0, -300}) CHECK(al(&m, &i, 5, &x, &i, 1, F, &r) == AMUSE_EINVAL && strstr(g_err, "F "));
    for (int T : {-1, amuse::kBeatMaxAudioFrames + 1, INT_MAX}) CHECK(al(&m, &i, T, &x, &i, 1, 2, &r) == AMUSE_EINVAL && strstr(g_err, "T "));
    CHECK(al(&m, &i, 5, &x, &i, 1 << 20, 1 << 11, &r) == AMUSE_EINVAL && strstr(g_err, "an int"));            // N F = 2^31
    CHECK(al(&m, &i, amuse::kBeatMaxAudioFrames, &x, &i, 1 << 15, 2, &r) == AMUSE_EINVAL);                     // N T = 2^32
    CHECK(al(&m, &i, 5, &x, &i, INT_MAX / 166 + 1, 2, &r) == AMUSE_EINVAL);                                    // 166 N just beyond
    CHECK(launches() == 0);                                                                                    // nothing refused reached a launcher
    // ---- the parameter checks, through each call
    if (int e = param_refusals([&](const amuse_beat_params* p) { return amuse_beat_onsets(ctx, &x, nullptr, 560, 2, p, &x, &m, st); })) return e;
    if (int e = param_refusals([&](const amuse_beat_params* p) { return amuse_beat_pick(&x, &i, 2, 5, p, &m, st); })) return e;
    if (int e = param_refusals([&](const amuse_beat_params* p) { return amuse_beat_align(&m, &i, 5, &x, &i, 1, 2, p, &r, nullptr, st); })) return e;
    CHECK(g_env.size() == 2 && g_pick.size() == 4 && g_align.size() == 2);                                     // only the two passing calls of each launched
    g_env.clear(); g_pick.clear(); g_align.clear();
    return 0;
}

static int launch_checks(amuse_beat* ctx) {
    using namespace amuse;
    float w = 0, env = 0;
    unsigned char m = 0;
    int nv = 0;
    double r = 0;
    void* st = reinterpret_cast<void*>(0x80);
    const Beat* c = reinterpret_cast<const Beat*>(ctx);
    amuse_beat_params p;
    amuse_beat_default_params(&p);
    p.onset_window = 5;
    const struct { int n, B, T, runs; } ok[] = {{400, 1, 1, 1}, {560, 3, 2, 1}, {2800, 1, 16, 1}, {2960, 1, 17, 2}, {3120, 3, 18, 2}, {170000, 3, 1061, 67}, {1920000, 256, 11998, 750}};
    for (const auto& k : ok) {
        g_env.clear(); g_pick.clear();
        CHECK(amuse_beat_onsets(ctx, &w, &nv, k.n, k.B, &p, &env, &m, st) == AMUSE_OK);
        CHECK(g_env.size() == 1 && g_pick.size() == 1 && g_stream == static_cast<hipStream_t>(st));
        const BeatEnvArgs& e = g_env[0];
        CHECK(e.waves == &w && e.n_valid == &nv && e.envelope == &env && e.n_samples == k.n && e.B == k.B && e.T == k.T && e.runs == k.runs);
        CHECK(e.window == c->window && e.melw_t == c->melw_t && e.mel_range == c->mel_range && (long long)e.runs * kBeatRun >= e.T && (long long)(e.runs - 1) * kBeatRun < e.T);
        const BeatPickArgs& q = g_pick[0];                                                                       // exactly the pick stage, on the call's own envelope
        CHECK(q.envelope == &env && q.frames == nullptr && q.n_valid == &nv && q.mask == &m && q.B == k.B && q.T == k.T && q.n_samples == k.n && q.p.onset_window == 5);
    }
    g_env.clear(); g_pick.clear();
    CHECK(amuse_beat_onsets(ctx, &w, nullptr, 560, 1, nullptr, &env, nullptr, st) == AMUSE_OK && g_env.size() == 1 && g_pick.empty());   // the envelope alone
    CHECK(amuse_beat_onsets(ctx, &w, nullptr, 399, 2, nullptr, &env, &m, st) == AMUSE_OK && g_env.size() == 1 && g_pick.empty());        // T == 0: nothing to launch
    // the reserved envelope: grows only, keeps what it outgrew, and feeds the pick
    CHECK(amuse_beat_reserve(nullptr, 1, 560) == AMUSE_EINVAL);
    CHECK(amuse_beat_reserve(ctx, 0, 560) == AMUSE_EINVAL && amuse_beat_reserve(ctx, 1, 0) == AMUSE_EINVAL);
    CHECK(amuse_beat_reserve(ctx, 2, 560) == AMUSE_OK && c->env && c->env_floats == 4 && c->retired.empty());
    float* first = c->env;
    CHECK(amuse_beat_reserve(ctx, 1, 560) == AMUSE_OK && c->env == first);
    CHECK(amuse_beat_reserve(ctx, 3, 3120) == AMUSE_OK && c->env != first && c->env_floats == 54 && c->retired.size() == 1 && c->retired[0] == first);
    g_env.clear(); g_pick.clear();
    CHECK(amuse_beat_onsets(ctx, &w, nullptr, 3120, 3, nullptr, nullptr, &m, st) == AMUSE_OK && g_env[0].envelope == c->env && g_pick[0].envelope == c->env);
    CHECK(amuse_beat_onsets(ctx, &w, nullptr, 3280, 3, nullptr, nullptr, &m, st) == AMUSE_EINVAL && strstr(g_err, "amuse_beat_reserve"));
    // pick and align pass their arguments through, one launch each
    g_pick.clear();
    CHECK(amuse_beat_pick(&env, &nv, 4, 65, &p, &m, nullptr) == AMUSE_OK && g_pick.size() == 1 && g_stream == nullptr);
    CHECK(g_pick[0].envelope == &env && g_pick[0].frames == &nv && g_pick[0].n_valid == nullptr && g_pick[0].B == 4 && g_pick[0].T == 65);
    p.motion_order = 32; p.fps = 25.0; p.sigma_s = 0.2;
    CHECK(amuse_beat_align(&m, &nv, 198, &w, &nv, 3, 60, &p, &r, &m, st) == AMUSE_OK && g_align.size() == 1);
    const BeatAlignArgs& a = g_align[0];
    CHECK(a.onset_mask == &m && a.audio_frames == &nv && a.joints == &w && a.lengths == &nv && a.rows == &r && a.beat_mask == &m && a.T == 198 && a.N == 3 && a.F == 60);
    CHECK(a.p.motion_order == 32 && a.p.fps == 25.0 && a.p.sigma_s == 0.2 && 2 * a.p.motion_order + 1 <= kBeatRing);
    CHECK(amuse_beat_align(nullptr, &nv, 0, &w, &nv, 1, 2, nullptr, &r, nullptr, st) == AMUSE_OK);                // T == 0 needs no mask
    CHECK(amuse_beat_align(&m, &nv, kBeatMaxAudioFrames, &w, &nv, 1, INT_MAX / 2, nullptr, &r, nullptr, st) == AMUSE_OK);
    g_result = hipErrorInvalidConfiguration;                                                                     // a launch the runtime refuses comes back as AMUSE_EHIP
    CHECK(amuse_beat_align(&m, &nv, 5, &w, &nv, 1, 2, nullptr, &r, nullptr, st) == AMUSE_EHIP && strstr(g_err, "launch failed"));
    CHECK(amuse_beat_pick(&env, &nv, 1, 5, nullptr, &m, st) == AMUSE_EHIP && strstr(g_err, "launch failed"));
    CHECK(amuse_beat_onsets(ctx, &w, nullptr, 560, 1, nullptr, &env, &m, st) == AMUSE_EHIP && strstr(g_err, "envelope launch failed"));
    g_result = hipSuccess;
    return 0;
}

int main() {
    using namespace amuse;
    static_assert(sizeof(BeatEnvArgs) <= 4096 && sizeof(BeatPickArgs) <= 4096 && sizeof(BeatAlignArgs) <= 4096, "the kernel arguments must fit the 4 KiB argument segment");
    static_assert(kBeatEnvBlock == 256 && kBeatEnvLdsBytes == 4136, "the FFT shape of k_fbank: re, im, the mean's and the flux's wave sums");
    static_assert(kBeatPickLdsBytes == 16 && kBeatAlignBlock == 64 && kSmplxJoints <= kBeatAlignBlock, "a lane per joint in one wave");
    static_assert(kBeatAlignLdsBytes == 49664 && kBeatAlignLdsBytes <= 64 * 1024, "the speed ring and the onset bits fit a workgroup's 64 KiB");
    static_assert((kBeatMaxAudioFrames / 64) * 2 == kBeatMaxAudioFrames / 32, "a ballot fills two whole words of the onset bits");
    if (int e = plan_and_row_checks()) return e;
    CHECK(amuse_beat_create(0, nullptr, nullptr) == nullptr && strstr(g_err, "mel_banks"));
    std::vector<float> banks((size_t)128 * 257, 0.f), window(400, 0.5f);
    for (int m = 0; m < 128; ++m)
        for (int k = 2 * m; k < 2 * m + 3; ++k) banks[(size_t)m * 257 + k] = 0.5f;
    CHECK(amuse_beat_create(-1, banks.data(), window.data()) == nullptr && strstr(g_err, "device"));
    amuse_beat* ctx = amuse_beat_create(0, banks.data(), window.data());
    CHECK(ctx != nullptr);
    {   // the device image of the bank: transposed, with each filter's support (the stub's device memory is host memory)
        const Beat* c = reinterpret_cast<const Beat*>(ctx);
        CHECK(c->melw_t[(size_t)4 * 128 + 2] == 0.5f && c->melw_t[(size_t)4 * 128 + 3] == 0.f && c->mel_range[2 * 5] == 10 && c->mel_range[2 * 5 + 1] == 13 && c->window[399] == 0.5f);
    }
    if (int e = refusal_checks(ctx)) return e;
    if (int e = launch_checks(ctx)) return e;
    amuse_beat_destroy(ctx);
    amuse_beat_destroy(nullptr);
    puts("beat_host ok");
    return 0;
}
