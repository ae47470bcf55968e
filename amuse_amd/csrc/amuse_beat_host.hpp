// Beat alignment (include/amuse_hip.h amuse_beat_*): everything the calls need on the host, shared by k_beat.hip (the three kernels and their launchers),
// amuse_beat.hip (the C entry points) and tests/beat_host (the same host code on stand-in launchers, under sanitizers):
//   - the definitions' constants, the frame plan (T stated once) and the row layout: the ONE statement of where each block of a clip's 166 doubles begins
//     (amuse_amd/beat_align.py ROW_BLOCKS restates the table and a test holds its total to amuse_beat_align_row());
//   - the parameter and argument checks, made before any HIP call;
//   - the context (the fbank tables on the device, the optional envelope buffer) and the launches.
// The metric is this project's own statement, in the manner of BEAT's `alignment` and librosa's spectral-flux onset detector; nothing here is pinned against
// either (include/amuse_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kBeatMel = 128, kBeatBins = 257;           // the fbank tables of audio.kaldi_tables()
constexpr int kBeatWin = 400, kBeatHop = 160, kBeatFft = 512, kBeatRate = 16000;
constexpr int kBeatRun = 16;                             // consecutive frames of one clip a workgroup of the envelope kernel takes (+ the one before them)
constexpr int kBeatEnvBlock = 256;                       // the FFT shape of k_fbank: a butterfly per thread
constexpr int kBeatEnvLdsBytes = (2 * kBeatFft + 8 + 2) * 4;   // re, im, the four wave sums of the DC mean (8 slots), the two wave sums of the flux
constexpr int kBeatPickBlock = 256;
constexpr int kBeatPickLdsBytes = (kBeatPickBlock / 64) * 4;   // the waves' maxima
constexpr int kBeatMaxOrder = 32;                        // motion_order: a lane's ring of 2 order + 1 speeds lives in LDS
constexpr int kBeatRing = 2 * kBeatMaxOrder + 1;
constexpr int kBeatMaxAudioFrames = 131072;              // T of amuse_beat_align: one onset bit per frame in LDS (16 KiB)
constexpr int kBeatAlignBlock = 64;                      // one wave per clip: a lane per joint walks the clip in time
constexpr int kBeatAlignLdsBytes = kBeatRing * 64 * 8 + kBeatMaxAudioFrames / 8;

// the row: block offsets in doubles (include/amuse_hip.h states the same table)
enum : int {
    kBeatRowOnsets = 0,                                  // 1
    kBeatRowBeats = 1,                                   // 55
    kBeatRowA2M = kBeatRowBeats + 55,                    // 55
    kBeatRowM2A = kBeatRowA2M + 55,                      // 55
    kBeatRow = kBeatRowM2A + 55,
};
static_assert(kBeatRow == 166, "the row of include/amuse_hip.h");

// the parameters as the kernels take them (by value)
struct BeatParams {
    double sigma_s, onset_delta, fps;
    int onset_window, onset_avg_window, motion_order;
};

struct BeatEnvArgs {
    const float* waves;      // dev [B][n_samples]
    const int* n_valid;      // dev [B] or NULL
    const float* window;     // dev [400]
    const float* melw_t;     // dev [257][128]: the filter bank transposed
    const int* mel_range;    // dev [128][2]: first / end bin of each filter's support
    float* envelope;         // dev [B][T]
    int n_samples, B, T, runs;   // runs = ceil(T / kBeatRun) workgroups per clip
};

struct BeatPickArgs {
    const float* envelope;   // dev [B][T]
    const int* frames;       // dev [B] or NULL (every clip has T; amuse_beat_onsets passes n_valid instead)
    const int* n_valid;      // dev [B] or NULL: when given, the clip's frames are the plan of its samples (clamped to 0..n_samples)
    unsigned char* mask;     // dev [B][T]
    int B, T, n_samples;
    BeatParams p;
};

struct BeatAlignArgs {
    const unsigned char* onset_mask;   // dev [N][T]
    const int* audio_frames;           // dev [N]
    const float* joints;               // dev [N][F][55][3]
    const int* lengths;                // dev [N]
    double* rows;                      // dev [N][166]
    unsigned char* beat_mask;          // dev [N][F][55] or NULL
    int T, N, F;
    BeatParams p;
};

// k_beat.hip (tests/beat_host: stand-ins that record the arguments)
hipError_t launch_beat_envelope(const BeatEnvArgs& a, hipStream_t stream);
hipError_t launch_beat_pick(const BeatPickArgs& a, hipStream_t stream);
hipError_t launch_beat_align(const BeatAlignArgs& a, hipStream_t stream);

// ---- T, stated once (host and device)
__host__ __device__ inline long long beat_frames_ll(long long n) { return n < kBeatWin ? 0 : 1 + (n - kBeatWin) / kBeatHop; }

inline int beat_plan(long long n_samples, int* frames) {
    if (n_samples < 0) return amuse_failf(AMUSE_EINVAL, "amuse_beat_plan: n_samples %lld < 0", n_samples);
    const long long T = beat_frames_ll(n_samples);
    if (T > INT_MAX) return amuse_failf(AMUSE_EINVAL, "amuse_beat_plan: n_samples %lld gives more frames than an int holds", n_samples);
    if (frames) *frames = (int)T;
    return AMUSE_OK;
}

inline int beat_default_params(amuse_beat_params* p) {
    if (!p) return amuse_failf(AMUSE_EINVAL, "amuse_beat_default_params: params is NULL");
    p->sigma_s = 0.1;
    p->onset_delta = 0.07;
    p->onset_window = 3;
    p->onset_avg_window = 10;
    p->motion_order = 3;
    p->fps = 30.0;
    return AMUSE_OK;
}

// ---- the parameter checks (NULL: the defaults)
inline int beat_params_check(const char* who, const amuse_beat_params* in, BeatParams* out) {
    amuse_beat_params d;
    if (!in) {
        beat_default_params(&d);
        in = &d;
    }
    if (!(in->sigma_s > 0.0) || !std::isfinite(in->sigma_s)) return amuse_failf(AMUSE_EINVAL, "%s: sigma_s %g must be positive and finite", who, in->sigma_s);
    if (!(in->onset_delta >= 0.0) || !std::isfinite(in->onset_delta)) return amuse_failf(AMUSE_EINVAL, "%s: onset_delta %g must be >= 0 and finite", who, in->onset_delta);
    if (in->onset_window < 1) return amuse_failf(AMUSE_EINVAL, "%s: onset_window %d < 1", who, in->onset_window);
    if (in->onset_avg_window < 1) return amuse_failf(AMUSE_EINVAL, "%s: onset_avg_window %d < 1", who, in->onset_avg_window);
    if (in->motion_order < 1 || in->motion_order > kBeatMaxOrder) return amuse_failf(AMUSE_EINVAL, "%s: motion_order %d outside 1..%d", who, in->motion_order, kBeatMaxOrder);
    if (!(in->fps > 0.0) || !std::isfinite(in->fps)) return amuse_failf(AMUSE_EINVAL, "%s: fps %g must be positive and finite", who, in->fps);
    *out = BeatParams{in->sigma_s, in->onset_delta, in->fps, in->onset_window, in->onset_avg_window, in->motion_order};
    return AMUSE_OK;
}

// ---- the context
struct Beat {
    int device = 0;
    float *melw_t = nullptr, *window = nullptr;
    int* mel_range = nullptr;
    float* env = nullptr;                 // amuse_beat_reserve's buffer: the current one
    size_t env_floats = 0;
    std::vector<float*> retired;          // smaller buffers an earlier call (or a captured graph) may still write: freed at destroy
};

inline void beat_destroy(Beat* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->melw_t) (void)hipFree(c->melw_t);
    if (c->window) (void)hipFree(c->window);
    if (c->mel_range) (void)hipFree(c->mel_range);
    if (c->env) (void)hipFree(c->env);
    for (float* p : c->retired) (void)hipFree(p);
    delete c;
}

inline Beat* beat_create(int device, const float* mel_banks, const float* window) {
    if (!mel_banks || !window) {
        amuse_failf(AMUSE_EINVAL, "amuse_beat_create: mel_banks and window must be given");
        return nullptr;
    }
    if (device < 0) {
        amuse_failf(AMUSE_EINVAL, "amuse_beat_create: device %d < 0", device);
        return nullptr;
    }
    // device image of the filter bank, as amuse_audio_create builds it: transposed (a bin's 128 weights contiguous) + each filter's support
    std::vector<float> mel_t((size_t)kBeatBins * kBeatMel);
    std::vector<int> rng(2 * kBeatMel);
    for (int m = 0; m < kBeatMel; ++m) {
        int k0 = kBeatBins, k1 = 0;
        for (int k = 0; k < kBeatBins; ++k) {
            const float w = mel_banks[(size_t)m * kBeatBins + k];
            mel_t[(size_t)k * kBeatMel + m] = w;
            if (w != 0.f) {
                if (k < k0) k0 = k;
                k1 = k + 1;
            }
        }
        rng[2 * m] = k0 < k1 ? k0 : 0;
        rng[2 * m + 1] = k0 < k1 ? k1 : 0;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        amuse_failf(AMUSE_EHIP, "amuse_beat_create: hipSetDevice(%d): %s", device, hipGetErrorString(e));
        return nullptr;
    }
    Beat* c = new Beat();
    c->device = device;
    auto up = [&](void** dst, const void* src, size_t bytes) {
        hipError_t r = hipMalloc(dst, bytes);
        if (r == hipSuccess) r = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return r;
    };
    e = up(reinterpret_cast<void**>(&c->melw_t), mel_t.data(), mel_t.size() * sizeof(float));
    if (e == hipSuccess) e = up(reinterpret_cast<void**>(&c->window), window, kBeatWin * sizeof(float));
    if (e == hipSuccess) e = up(reinterpret_cast<void**>(&c->mel_range), rng.data(), rng.size() * sizeof(int));
    if (e != hipSuccess) {
        amuse_failf(AMUSE_EHIP, "amuse_beat_create: upload of the fbank tables: %s", hipGetErrorString(e));
        beat_destroy(c);
        return nullptr;
    }
    return c;
}

// ---- the shape checks shared by reserve and onsets
inline int beat_wave_shape(const char* who, int B, int n_samples, int* T) {
    if (B < 1) return amuse_failf(AMUSE_EINVAL, "%s: B %d < 1", who, B);
    if (n_samples < 1) return amuse_failf(AMUSE_EINVAL, "%s: n_samples %d < 1", who, n_samples);
    *T = (int)beat_frames_ll(n_samples);
    const long long runs = (*T + kBeatRun - 1) / kBeatRun;
    if ((long long)B * (*T > 0 ? *T : 1) > INT_MAX || (long long)B * runs > INT_MAX)
        return amuse_failf(AMUSE_EINVAL, "%s: B %d x %d frames: more frames in one call than an int holds", who, B, *T);
    return AMUSE_OK;
}

inline int beat_reserve(Beat* c, int B, int n_samples) {
    if (!c) return amuse_failf(AMUSE_EINVAL, "amuse_beat_reserve: ctx is NULL");
    int T = 0;
    if (int rc = beat_wave_shape("amuse_beat_reserve", B, n_samples, &T)) return rc;
    const size_t need = (size_t)B * (size_t)T;
    if (need <= c->env_floats) return AMUSE_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_beat_reserve: hipSetDevice(%d): %s", c->device, hipGetErrorString(e));
    float* p = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(float));
    if (e != hipSuccess) return amuse_failf(AMUSE_ENOMEM, "amuse_beat_reserve: %zu bytes of envelope: %s", need * sizeof(float), hipGetErrorString(e));
    if (c->env) c->retired.push_back(c->env);
    c->env = p;
    c->env_floats = need;
    return AMUSE_OK;
}

// ---- amuse_beat_pick: checks, then one launch
inline int beat_pick(const float* envelope, const int* frames_dev, int B, int T, const amuse_beat_params* params, unsigned char* mask, hipStream_t stream) {
    BeatParams p;
    if (int rc = beat_params_check("amuse_beat_pick", params, &p)) return rc;
    if (!envelope) return amuse_failf(AMUSE_EINVAL, "amuse_beat_pick: envelope_dev must be given");
    if (!frames_dev) return amuse_failf(AMUSE_EINVAL, "amuse_beat_pick: frames_dev must be given");
    if (!mask) return amuse_failf(AMUSE_EINVAL, "amuse_beat_pick: onset_mask_out must be given");
    if (B < 1) return amuse_failf(AMUSE_EINVAL, "amuse_beat_pick: B %d < 1", B);
    if (T < 1) return amuse_failf(AMUSE_EINVAL, "amuse_beat_pick: T %d < 1", T);
    if ((long long)B * T > INT_MAX) return amuse_failf(AMUSE_EINVAL, "amuse_beat_pick: B %d x T %d: more frames in one call than an int holds", B, T);
    const BeatPickArgs a{envelope, frames_dev, nullptr, mask, B, T, 0, p};
    const hipError_t e = launch_beat_pick(a, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_beat_pick: launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

// ---- amuse_beat_onsets: checks, then the envelope launch and the pick launch
inline int beat_onsets(Beat* c, const float* waves, const int* n_valid, int n_samples, int B, const amuse_beat_params* params, float* envelope_out,
                       unsigned char* mask_out, hipStream_t stream) {
    BeatParams p;
    if (int rc = beat_params_check("amuse_beat_onsets", params, &p)) return rc;
    if (!c) return amuse_failf(AMUSE_EINVAL, "amuse_beat_onsets: ctx is NULL");
    if (!waves) return amuse_failf(AMUSE_EINVAL, "amuse_beat_onsets: waves_dev must be given");
    if (!envelope_out && !mask_out) return amuse_failf(AMUSE_EINVAL, "amuse_beat_onsets: envelope_out and onset_mask_out are both NULL");
    int T = 0;
    if (int rc = beat_wave_shape("amuse_beat_onsets", B, n_samples, &T)) return rc;
    float* env = envelope_out;
    if (!env) {
        if ((size_t)B * (size_t)T > c->env_floats)
            return amuse_failf(AMUSE_EINVAL, "amuse_beat_onsets: envelope_out is NULL and amuse_beat_reserve has not covered B %d x %d frames (nothing is allocated here)", B, T);
        env = c->env;
    }
    if (T == 0) return AMUSE_OK;                          // nothing to write: both outputs are [B][0]
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_beat_onsets: hipSetDevice(%d): %s", c->device, hipGetErrorString(e));
    const BeatEnvArgs ea{waves, n_valid, c->window, c->melw_t, c->mel_range, env, n_samples, B, T, (T + kBeatRun - 1) / kBeatRun};
    e = launch_beat_envelope(ea, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_beat_onsets: envelope launch failed: %s", hipGetErrorString(e));
    if (!mask_out) return AMUSE_OK;
    const BeatPickArgs pa{env, nullptr, n_valid, mask_out, B, T, n_samples, p};
    e = launch_beat_pick(pa, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_beat_onsets: pick launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

// ---- amuse_beat_align: checks, then one launch (the lengths and audio frame counts live on the device: the kernel clamps / answers a bad length with NaN)
inline int beat_align(const unsigned char* onset_mask, const int* audio_frames, int T, const float* joints, const int* lengths, int N, int F,
                      const amuse_beat_params* params, double* rows, unsigned char* beat_mask, hipStream_t stream) {
    BeatParams p;
    if (int rc = beat_params_check("amuse_beat_align", params, &p)) return rc;
    if (T < 0 || T > kBeatMaxAudioFrames) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: T %d outside 0..%d", T, kBeatMaxAudioFrames);
    if (!onset_mask && T > 0) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: onset_mask_dev must be given");
    if (!audio_frames) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: audio_frames_dev must be given");
    if (!joints) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: joints must be given");
    if (!lengths) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: lengths_dev must be given");
    if (!rows) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: rows_out must be given");
    if (N < 1) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: N %d < 1", N);
    if (F < 2) return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: F %d < 2", F);
    if ((long long)N * F > INT_MAX || (long long)N * T > INT_MAX || (long long)N * kBeatRow > INT_MAX)
        return amuse_failf(AMUSE_EINVAL, "amuse_beat_align: N %d x F %d x T %d: more frames or row entries in one call than an int holds", N, F, T);
    const BeatAlignArgs a{onset_mask, audio_frames, joints, lengths, rows, beat_mask, T, N, F, p};
    const hipError_t e = launch_beat_align(a, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_beat_align: launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

}  // namespace amuse
