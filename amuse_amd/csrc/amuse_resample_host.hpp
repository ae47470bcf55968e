// Sample-rate conversion in front of the audio front-end (include/amuse_hip.h amuse_resample_plan / amuse_resampler_create / amuse_resample): everything the
// resampler needs on the host, shared by k_resample.hip (the kernel and its launcher), amuse_resample.hip (the C entry points) and tests/resample_host (the same
// host code on a stand-in launcher, under sanitizers):
//   - the plan: the ONE statement of the polyphase filter - up / down factors, half width, taps per phase, output count - and of its bank of coefficients;
//   - every argument check, made before any HIP call;
//   - the resampler object: the bank in device memory, built and uploaded once per rate pair.
// AN EXTENSION: the reference never resamples (scripts/trainer.py:520 drops the file's rate).  The filter - a Hann-windowed sinc, 6 zero crossings, roll-off 0.99 -
// is a recollection of torchaudio.functional.resample's defaults and is pinned against nothing but its own restatement (tests/resample_ref.py).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kResampleBlock = 256;                  // one thread per output sample
constexpr int kResampleMinRate = 4000, kResampleMaxRate = 384000;
constexpr int kResampleLpw = 6;                      // zero crossings of the sinc on each side
constexpr double kResampleRolloff = 0.99;
constexpr long long kResampleMaxBankBytes = 2ll << 20;   // 2 MiB of coefficients (L x K floats): 44100 -> 16000 takes 22.5 KiB, 44101 -> 16000 would take 2.2 MiB
constexpr int kResampleMaxChannels = 8;

struct ResamplePlan {
    int M, L;      // rate_in / g, rate_out / g: L output samples per M input samples
    int Hw, K;     // input samples on each side of an output's position; taps per phase
};

struct ResampleArgs {
    const void* pcm;      // [n_in][channels] interleaved frames, `format`
    const float* bank;    // [L][K]
    float* out;           // [n_out]
    long long n_in, n_out;
    int format, channels;
    int M, L, Hw, K;
};

// k_resample.hip (tests/resample_host: a stand-in that records the arguments)
hipError_t launch_resample(const ResampleArgs& a, hipStream_t stream);

inline int resample_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// ---- the plan.  Equal rates: the identity (one tap of 1, no neighbours), so that the output is the format conversion itself.
inline int resample_plan_rates(int rate_in, int rate_out, ResamplePlan* p) {
    if (rate_in < kResampleMinRate || rate_in > kResampleMaxRate || rate_out < kResampleMinRate || rate_out > kResampleMaxRate)
        return amuse_failf(AMUSE_EINVAL, "amuse_resample: rates %d -> %d outside %d..%d Hz", rate_in, rate_out, kResampleMinRate, kResampleMaxRate);
    const int g = resample_gcd(rate_in, rate_out);
    p->M = rate_in / g;
    p->L = rate_out / g;
    if (rate_in == rate_out) {
        p->Hw = 0;
        p->K = 1;
        return AMUSE_OK;
    }
    const double base = kResampleRolloff * (p->M < p->L ? p->M : p->L);
    p->Hw = (int)std::ceil(kResampleLpw * (double)p->M / base);
    p->K = 2 * p->Hw + 2;
    const long long bytes = (long long)p->L * p->K * (long long)sizeof(float);
    if (bytes > kResampleMaxBankBytes)
        return amuse_failf(AMUSE_EINVAL, "amuse_resample: %d -> %d Hz needs %d phases of %d taps = %lld bytes of coefficients, above the cap of %lld (rates with a larger "
                                         "common divisor give a smaller bank)", rate_in, rate_out, p->L, p->K, bytes, kResampleMaxBankBytes);
    return AMUSE_OK;
}

inline int resample_plan(int rate_in, int rate_out, long long n_in, int* up, int* down, int* taps, long long* n_out) {
    ResamplePlan p{};
    if (int rc = resample_plan_rates(rate_in, rate_out, &p)) return rc;
    if (n_in < 1) return amuse_failf(AMUSE_EINVAL, "amuse_resample: n_in %lld < 1", n_in);
    if (n_in > INT_MAX) return amuse_failf(AMUSE_EINVAL, "amuse_resample: n_in %lld is more samples than an int holds", n_in);
    const long long no = (n_in * p.L + p.M - 1) / p.M;
    if (no > INT_MAX) return amuse_failf(AMUSE_EINVAL, "amuse_resample: n_in %lld at %d -> %d Hz gives more output samples than an int holds", n_in, rate_in, rate_out);
    if (up) *up = p.L;
    if (down) *down = p.M;
    if (taps) *taps = p.K;
    if (n_out) *n_out = no;
    return AMUSE_OK;
}

// ---- the bank, in double, rounded to fp32: h[i][k] = (base / M) sinc(pi t) cos^2(pi t / (2 lpw)) for |t| < lpw, t = base ((floor(i M / L) - Hw + k) / M - i / L)
inline void resample_bank(const ResamplePlan& p, float* h) {
    if (p.M == p.L) { h[0] = 1.f; return; }
    const double pi = 3.14159265358979323846;
    const double base = kResampleRolloff * (p.M < p.L ? p.M : p.L), scale = base / p.M;
    for (int i = 0; i < p.L; ++i) {
        const long long off = (long long)i * p.M / p.L - p.Hw;
        const double frac = (double)i / p.L;
        for (int k = 0; k < p.K; ++k) {
            const double t = base * ((double)(off + k) / p.M - frac);
            double v = 0.0;
            if (std::fabs(t) < kResampleLpw) {
                const double pt = pi * t;
                const double s = pt == 0.0 ? 1.0 : std::sin(pt) / pt;
                const double c = std::cos(pt / (2.0 * kResampleLpw));
                v = scale * s * (c * c);
            }
            h[(size_t)i * p.K + k] = (float)v;
        }
    }
}

struct Resampler {
    int device, rate_in, rate_out;
    ResamplePlan plan;
    float* bank_dev;
};

// ---- the call's checks: everything that can be refused without touching the GPU
inline int resample_check(const Resampler* r, const void* pcm, int format, int channels, long long n_in, const float* out, long long out_capacity, long long* n_out) {
    if (!r) return amuse_failf(AMUSE_EINVAL, "amuse_resample: resampler is NULL");
    if (int rc = resample_plan(r->rate_in, r->rate_out, n_in, nullptr, nullptr, nullptr, n_out)) return rc;
    if (channels < 1 || channels > kResampleMaxChannels) return amuse_failf(AMUSE_EINVAL, "amuse_resample: channels %d outside 1..%d", channels, kResampleMaxChannels);
    if (format != AMUSE_PCM_U8 && format != AMUSE_PCM_S16 && format != AMUSE_PCM_S32 && format != AMUSE_PCM_F32)
        return amuse_failf(AMUSE_EINVAL, "amuse_resample: unknown format %d (AMUSE_PCM_U8 / _S16 / _S32 / _F32)", format);
    if (out_capacity < *n_out) return amuse_failf(AMUSE_EINVAL, "amuse_resample: out_capacity %lld below n_out %lld", out_capacity, *n_out);
    if (!pcm || !out) return amuse_failf(AMUSE_EINVAL, "amuse_resample: pcm and out must be given");
    return AMUSE_OK;
}

inline int resample_run(const Resampler* r, const void* pcm, int format, int channels, long long n_in, float* out, long long out_capacity, hipStream_t stream) {
    long long n_out = 0;
    if (int rc = resample_check(r, pcm, format, channels, n_in, out, out_capacity, &n_out)) return rc;
    const ResampleArgs a{pcm, r->bank_dev, out, n_in, n_out, format, channels, r->plan.M, r->plan.L, r->plan.Hw, r->plan.K};
    hipError_t e = hipSetDevice(r->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_resample: hipSetDevice(%d): %s", r->device, hipGetErrorString(e));
    e = launch_resample(a, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_resample: launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

inline Resampler* resampler_create(int device, int rate_in, int rate_out) {
    ResamplePlan p{};
    if (resample_plan_rates(rate_in, rate_out, &p)) return nullptr;
    std::vector<float> h((size_t)p.L * p.K);
    resample_bank(p, h.data());
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { amuse_failf(AMUSE_EHIP, "amuse_resampler_create: hipSetDevice(%d): %s", device, hipGetErrorString(e)); return nullptr; }
    float* d = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&d), h.size() * sizeof(float));
    if (e != hipSuccess) { amuse_failf(AMUSE_ENOMEM, "amuse_resampler_create: %zu bytes of coefficients: %s", h.size() * sizeof(float), hipGetErrorString(e)); return nullptr; }
    e = hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        amuse_failf(AMUSE_EHIP, "amuse_resampler_create: upload of the coefficients: %s", hipGetErrorString(e));
        return nullptr;
    }
    return new Resampler{device, rate_in, rate_out, p, d};
}

inline void resampler_destroy(Resampler* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipFree(r->bank_dev);
    delete r;
}

}  // namespace amuse
