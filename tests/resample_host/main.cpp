// Stand-alone program (its own main): the host half of the resampler - csrc/amuse_resample_host.hpp through the entry points of csrc/amuse_resample.hip - under
// AddressSanitizer / UBSan on a machine without a GPU.  The kernel's launcher is a stand-in here that keeps the argument structs, the HIP runtime is the stub of
// tests/host_asan (hipMalloc = malloc, so the uploaded bank can be read back):
//   - the plan: the six known rows, equal rates, a sweep of n_in against the arithmetic written out again, the refused arguments
//   - the bank of each row: its size (written to an exactly-sized heap block), the DC gain of every phase, the identity of equal rates
//   - the call: every refusal returns AMUSE_EINVAL and launches nothing; the accepted call's arguments; create / destroy leave nothing behind
// tests/test_resample_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "resample_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../amuse_amd/csrc/amuse_resample_host.hpp"
#include "../../include/amuse_hip.h"

#include "../host_check.hpp"

static std::vector<amuse::ResampleArgs> g_launches;
static hipStream_t g_stream = nullptr;
namespace amuse {
hipError_t launch_resample(const ResampleArgs& a, hipStream_t s) { g_launches.push_back(a); g_stream = s; return hipSuccess; }
}  // namespace amuse

static const struct { int rate, M, L, Hw, K; } kRows[] = {{48000, 3, 1, 19, 40}, {44100, 441, 160, 17, 36}, {22050, 441, 320, 9, 20},
                                                          {8000, 1, 2, 7, 16},   {96000, 6, 1, 37, 76},     {11025, 441, 640, 7, 16}};

static int plan_checks() {
    int up = 0, down = 0, taps = 0;
    long long n_out = 0;
    for (const auto& r : kRows) {
        CHECK(amuse_resample_plan(r.rate, 16000, 1000, &up, &down, &taps, &n_out) == 0 && up == r.L && down == r.M && taps == r.K && taps == 2 * r.Hw + 2);
        for (long long n = 1; n <= 2000; ++n) {
            CHECK(amuse_resample_plan(r.rate, 16000, n, nullptr, nullptr, nullptr, &n_out) == 0);
            long long want = n * r.L / r.M;
            if (want * r.M < n * r.L) ++want;                                  // the ceiling, written out again
            CHECK(n_out == want);
            // the last output's first tap position lies inside the waveform: floor((n_out - 1) M / L) <= n - 1
            CHECK((n_out - 1) * r.M / r.L <= n - 1);
        }
    }
    CHECK(amuse_resample_plan(16000, 16000, 777, &up, &down, &taps, &n_out) == 0 && up == 1 && down == 1 && taps == 1 && n_out == 777);   // equal rates: the identity
    CHECK(amuse_resample_plan(48000, 16000, 3, nullptr, nullptr, nullptr, nullptr) == 0);   // every output is optional
    CHECK(amuse_resample_plan(4000, 384000, 10, &up, &down, &taps, &n_out) == 0 && up == 96 && down == 1 && n_out == 960);
    CHECK(amuse_resample_plan(384000, 4000, 10, &up, &down, &taps, &n_out) == 0 && up == 1 && down == 96 && n_out == 1);
    for (int bad : {3999, 384001, 0, -16000}) {
        CHECK(amuse_resample_plan(bad, 16000, 10, &up, &down, &taps, &n_out) == AMUSE_EINVAL);
        CHECK(amuse_resample_plan(16000, bad, 10, &up, &down, &taps, &n_out) == AMUSE_EINVAL);
    }
    CHECK(amuse_resample_plan(44101, 16000, 10, &up, &down, &taps, &n_out) == AMUSE_EINVAL && strstr(g_err, "cap"));      // 16000 phases of 36 taps: 2.2 MiB
    CHECK(amuse_resample_plan(48000, 16000, 0, &up, &down, &taps, &n_out) == AMUSE_EINVAL);
    CHECK(amuse_resample_plan(48000, 16000, -5, &up, &down, &taps, &n_out) == AMUSE_EINVAL);
    CHECK(amuse_resample_plan(48000, 16000, 1LL << 40, &up, &down, &taps, &n_out) == AMUSE_EINVAL);
    CHECK(amuse_resample_plan(8000, 16000, 2000000000LL, &up, &down, &taps, &n_out) == AMUSE_EINVAL);     // n_out beyond an int
    CHECK(amuse_resample_plan(48000, 16000, 2147483647LL, &up, &down, &taps, &n_out) == 0 && n_out == 715827883LL);
    return 0;
}

static int bank_checks() {
    for (const auto& r : kRows) {
        std::vector<float> h((size_t)r.L * r.K);                               // exactly the announced size: a write past it is the sanitizer's to find
        CHECK(amuse_debug_resample_bank(r.rate, 16000, h.data()) == 0);
        for (int i = 0; i < r.L; ++i) {
            double dc = 0;
            for (int k = 0; k < r.K; ++k) dc += h[(size_t)i * r.K + k];
            CHECK(dc > 1.00004 - 2e-6 && dc < 1.00088 + 2e-6);                 // (the range of the float64 bank, with room for the fp32 rounding of K taps)
        }
    }
    float one = 0.f;
    CHECK(amuse_debug_resample_bank(16000, 16000, &one) == 0 && one == 1.f);
    CHECK(amuse_debug_resample_bank(44101, 16000, &one) == AMUSE_EINVAL);
    CHECK(amuse_debug_resample_bank(48000, 16000, nullptr) == AMUSE_EINVAL);
    return 0;
}

static int call_checks() {
    CHECK(amuse_resampler_create(0, 3999, 16000) == nullptr);
    CHECK(amuse_resampler_create(0, 44101, 16000) == nullptr);
    amuse_resampler* r = amuse_resampler_create(0, 44100, 16000);
    CHECK(r != nullptr);
    {   // the uploaded bank is the debug entry point's
        std::vector<float> h((size_t)160 * 36);
        CHECK(amuse_debug_resample_bank(44100, 16000, h.data()) == 0);
        const amuse::Resampler* rr = reinterpret_cast<const amuse::Resampler*>(r);
        CHECK(rr->plan.M == 441 && rr->plan.L == 160 && rr->plan.Hw == 17 && rr->plan.K == 36);
        CHECK(memcmp(rr->bank_dev, h.data(), h.size() * sizeof(float)) == 0);
    }
    std::vector<short> pcm(2 * 700);
    std::vector<float> out(254);                                               // ceil(700 x 160 / 441) = 254
    void* st = reinterpret_cast<void*>(0x40);
    CHECK(amuse_resample(nullptr, pcm.data(), AMUSE_PCM_S16, 2, 700, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), AMUSE_PCM_S16, 2, 0, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), AMUSE_PCM_S16, 0, 700, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), AMUSE_PCM_S16, 9, 700, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), 4, 2, 700, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), -1, 2, 700, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), AMUSE_PCM_S16, 2, 700, out.data(), 253, st) == AMUSE_EINVAL && strstr(g_err, "out_capacity"));
    CHECK(amuse_resample(r, nullptr, AMUSE_PCM_S16, 2, 700, out.data(), 254, st) == AMUSE_EINVAL);
    CHECK(amuse_resample(r, pcm.data(), AMUSE_PCM_S16, 2, 700, nullptr, 254, st) == AMUSE_EINVAL);
    CHECK(g_launches.empty());                                                 // nothing refused reached the launcher
    CHECK(amuse_resample(r, pcm.data(), AMUSE_PCM_S16, 2, 700, out.data(), 300, st) == 0);
    CHECK(g_launches.size() == 1 && g_stream == static_cast<hipStream_t>(st));
    {
        const amuse::ResampleArgs& a = g_launches[0];
        CHECK(a.pcm == pcm.data() && a.out == out.data() && a.bank == reinterpret_cast<const amuse::Resampler*>(r)->bank_dev);
        CHECK(a.n_in == 700 && a.n_out == 254 && a.format == AMUSE_PCM_S16 && a.channels == 2 && a.M == 441 && a.L == 160 && a.Hw == 17 && a.K == 36);
    }
    g_launches.clear();
    amuse_resampler_destroy(r);
    amuse_resampler_destroy(nullptr);
    amuse_resampler* id = amuse_resampler_create(0, 16000, 16000);
    CHECK(id != nullptr);
    CHECK(amuse_resample(id, pcm.data(), AMUSE_PCM_S16, 1, 1400, out.data(), 1399, nullptr) == AMUSE_EINVAL);
    std::vector<float> big(1400);
    CHECK(amuse_resample(id, pcm.data(), AMUSE_PCM_S16, 1, 1400, big.data(), 1400, nullptr) == 0 && g_launches.back().K == 1 && g_launches.back().n_out == 1400);
    g_launches.clear();
    amuse_resampler_destroy(id);
    return 0;
}

int main() {
    if (int e = plan_checks()) return e;
    if (int e = bank_checks()) return e;
    if (int e = call_checks()) return e;
    puts("resample_host ok");
    return 0;
}
