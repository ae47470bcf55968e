// Sample-rate conversion (include/amuse_hip.h amuse_resample): raw PCM frames in device memory -> fp32 at the front-end's rate, one polyphase FIR tap row per
// output sample.  One thread per output sample m: phase i = m mod L picks the row h[i][0..K-1] of the bank, j0 = floor(m M / L) - Hw the first input sample; the
// sum runs k = 0 .. K - 1 in fp32 (one fma per tap), taps that fall outside the waveform are skipped (x is zero there).  Every index is a 64-bit integer.
// No LDS staging: neighbouring threads read neighbouring input samples and rows (one row for all when L = 1), each input sample is re-read by about K L / M
// threads of the same or the next workgroup and those reads are served by the vector L1 / L2 - a 60 s clip is 5.8 MB of int16 in and 3.8 MB out, the launch
// costs more than the traffic.  Channel 0 only: lane addresses step by `channels` elements, the other channels' values are never loaded.
#include "amuse_resample_host.hpp"

#include <cstdint>

namespace amuse {

namespace {

// the WAV loader's conversions (amuse_amd/trainer.py load_wav); the divisors are powers of two, so multiplying by the reciprocal is the same rounding
__device__ __forceinline__ float pcm_to_float(uint8_t v) { return ((float)v - 128.0f) * (1.0f / 128.0f); }
__device__ __forceinline__ float pcm_to_float(int16_t v) { return (float)v * (1.0f / 32768.0f); }
__device__ __forceinline__ float pcm_to_float(int32_t v) { return (float)v * (1.0f / 2147483648.0f); }
__device__ __forceinline__ float pcm_to_float(float v) { return v; }

template <typename T>
__device__ __forceinline__ float resample_one(const T* __restrict__ x, const float* __restrict__ h, long long j0, int K, long long n_in, int channels) {
    // the taps whose sample exists: k in [k_lo, k_hi)
    const int k_lo = j0 < 0 ? (int)(-j0 < (long long)K ? -j0 : (long long)K) : 0;
    const long long left = n_in - j0;                  // samples from j0 to the waveform's end (may be <= 0 or > K)
    const int k_hi = left < (long long)K ? (left > 0 ? (int)left : 0) : K;
    if (k_lo >= k_hi) return 0.f;
    const T* p = x + (j0 + k_lo) * (long long)channels;
    float acc = h[k_lo] * pcm_to_float(*p);            // (not fma(h, x, 0): a float sample of -0 stays -0 through the identity bank)
    for (int k = k_lo + 1; k < k_hi; ++k) {
        p += channels;
        acc = fmaf(h[k], pcm_to_float(*p), acc);
    }
    return acc;
}

__global__ void __launch_bounds__(kResampleBlock) k_resample(const ResampleArgs a) {
    const long long m = (long long)blockIdx.x * kResampleBlock + threadIdx.x;
    if (m >= a.n_out) return;
    const long long q = m / a.L;
    const int i = (int)(m - q * a.L);
    const long long j0 = q * a.M + (long long)i * a.M / a.L - a.Hw;         // floor(m M / L) - Hw, m = q L + i
    const float* h = a.bank + (size_t)i * a.K;
    float y;
    switch (a.format) {                                                    // uniform over the grid
    case AMUSE_PCM_U8: y = resample_one(static_cast<const uint8_t*>(a.pcm), h, j0, a.K, a.n_in, a.channels); break;
    case AMUSE_PCM_S16: y = resample_one(static_cast<const int16_t*>(a.pcm), h, j0, a.K, a.n_in, a.channels); break;
    case AMUSE_PCM_S32: y = resample_one(static_cast<const int32_t*>(a.pcm), h, j0, a.K, a.n_in, a.channels); break;
    default: y = resample_one(static_cast<const float*>(a.pcm), h, j0, a.K, a.n_in, a.channels); break;
    }
    a.out[m] = y;
}

}  // namespace

hipError_t launch_resample(const ResampleArgs& a, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a.n_out + kResampleBlock - 1) / kResampleBlock);     // n_out <= INT_MAX by the plan's check
    hipLaunchKernelGGL(k_resample, dim3(blocks), dim3(kResampleBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
