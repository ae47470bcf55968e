// Beat alignment (include/amuse_hip.h amuse_beat_*): speech onsets of the 16 kHz waveform against the motion beats of the SMPL-X joints.  Three kernels:
//   k_beat_envelope  one workgroup per run of kBeatRun = 16 consecutive frames of one clip, 256 threads.  Each frame's kaldi log-mel is computed with the FFT shape
//                    of k_fbank (k_audio.hip: DC removal, pre-emphasis, window, 512-point radix-2 in LDS, a butterfly per thread, 128 mel filters on threads
//                    0..127) WITHOUT its normalisation; a thread keeps its filter's value of the previous frame in a register, so the positive spectral flux
//                    needs no [T][128] intermediate: a run recomputes only the one frame before it (17 FFTs for 16 envelope values), reads its 2960 samples
//                    once and writes 16 floats.  T is whatever the waveform gives: nothing here is sized by it.
//   k_beat_pick      one workgroup per clip looping over T: the clip maximum is a workgroup reduction, the three tests read the neighbours from the (L2-resident)
//                    envelope; double after the fp32 load, the products and sums that decide a frame written as single roundings (no contraction into an fma).
//   k_beat_align     one wave per clip, a lane per joint (55 of 64), walking the clip in time: a frame's 660 bytes are one coalesced load; the last
//                    2 motion_order + 1 speeds of a lane sit in an LDS ring; the clip's kept onsets are one bit per audio frame in LDS (built with a ballot).  A
//                    lane holds its last beat and a cursor into the onset bits: when it meets a beat it settles the onsets since its last one (each is nearest to
//                    one of the two) and the beat itself (nearest to the onset before or after the cursor), so the work is O(T + F) per joint, every sum runs in
//                    ascending time in the lane that owns it, in double, and nothing is shared between lanes: no atomics, no scratch, the same bits at any N.
// The butterflies of the first FFT stages touch LDS at a stride of 2, 4, ... floats - 2-way bank conflicts, as in k_fbank; the envelope kernel's time is the
// transcendental twiddles and the barriers, not LDS (profiles/beat_align_cost.txt).
#include "amuse_beat_host.hpp"

namespace amuse {

namespace {

// ---------------------------------------------------------------------------------------------- envelope
// the log-mel of one frame (valid in threads 0..127): k_fbank's arithmetic, step for step
__device__ __forceinline__ float frame_logmel(const float* __restrict__ src, const BeatEnvArgs& a, float* re, float* im, float* red, int t) {
    const float x0 = t < kBeatWin ? src[t] : 0.f, x1 = t + 256 < kBeatWin ? src[t + 256] : 0.f;
    float s = x0 + x1;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) * (1.0f / 400.0f);
    re[t] = x0 - mean;
    re[t + 256] = (t + 256 < kBeatWin) ? x1 - mean : 0.f;
    __syncthreads();
    // pre-emphasis against the previous sample (the first against itself), window, bit-reversed scatter for the FFT
    float y[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = t + 256 * h;
        y[h] = 0.f;
        if (i < kBeatWin) y[h] = (re[i] - 0.97f * re[i > 0 ? i - 1 : 0]) * a.window[i];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = t + 256 * h;
        const int r = __brev((unsigned)i) >> 23;   // 9-bit reversal
        re[r] = y[h];
        im[r] = 0.f;
    }
    __syncthreads();
    for (int len = 2; len <= kBeatFft; len <<= 1) {
        const int half = len >> 1, k = t & (half - 1), base = ((t - k) << 1) + k;
        float sn, cs;
        sincospif(-2.0f * (float)k / (float)len, &sn, &cs);
        const float ur = re[base], ui = im[base], vr = re[base + half], vi = im[base + half];
        const float tr = vr * cs - vi * sn, ti = vr * sn + vi * cs;
        __syncthreads();
        re[base] = ur + tr; im[base] = ui + ti;
        re[base + half] = ur - tr; im[base + half] = ui - ti;
        __syncthreads();
    }
    // power spectrum (bins 0..256) in place, then the mel filters: bins in ascending order over the filter's support
    const float p0 = re[t] * re[t] + im[t] * im[t];
    const float p256 = re[256] * re[256] + im[256] * im[256];
    __syncthreads();
    re[t] = p0;
    if (t == 0) re[256] = p256;
    __syncthreads();
    float S = 0.f;
    if (t < kBeatMel) {
        const int k0 = a.mel_range[2 * t], k1 = a.mel_range[2 * t + 1];
        float e = 0.f;
        for (int k = k0; k < k1; ++k) e += re[k] * a.melw_t[k * kBeatMel + t];
        S = logf(fmaxf(e, 1.1920929e-07f));
    }
    return S;   // (the next frame's first barrier stands between these reads of re[] and its writes)
}

__global__ void __launch_bounds__(kBeatEnvBlock) k_beat_envelope(const BeatEnvArgs a) {
    __shared__ float re[kBeatFft], im[kBeatFft], red[8], flux[2];
    const int t = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.runs), run = (int)(blockIdx.x - (unsigned)b * (unsigned)a.runs);
    int nv = a.n_valid ? a.n_valid[b] : a.n_samples;
    nv = nv < 0 ? 0 : (nv > a.n_samples ? a.n_samples : nv);
    const int Tb = (int)beat_frames_ll(nv);                                   // <= a.T
    const int t0 = run * kBeatRun, t1 = t0 + kBeatRun < a.T ? t0 + kBeatRun : a.T;
    float* __restrict__ env = a.envelope + (size_t)b * a.T;
    for (int f = (t0 > Tb ? t0 : Tb) + t; f < t1; f += kBeatEnvBlock) env[f] = 0.f;   // frames beyond the clip's own
    if (t0 >= Tb) return;                                                    // (uniform over the workgroup: nobody is left waiting at a barrier)
    const int tl = t1 < Tb ? t1 : Tb;
    const float* __restrict__ wave = a.waves + (size_t)b * a.n_samples;       // every frame below Tb lies inside the clip's nv samples
    float prev = 0.f;
    for (int f = t0 > 0 ? t0 - 1 : 0; f < tl; ++f) {
        const float S = frame_logmel(wave + (size_t)f * kBeatHop, a, re, im, red, t);
        if (f >= t0) {
            float d = (f > 0 && t < kBeatMel) ? fmaxf(S - prev, 0.f) : 0.f;    // e[0] = 0
            for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
            if (t == 0 || t == 64) flux[t >> 6] = d;
            __syncthreads();
            if (t == 0) env[f] = (flux[0] + flux[1]) * (1.0f / 128.0f);
        }
        prev = S;
    }
}

// ---------------------------------------------------------------------------------------------- pick
__global__ void __launch_bounds__(kBeatPickBlock) k_beat_pick(const BeatPickArgs a) {
    __shared__ float wmax[kBeatPickBlock / 64];
    const int b = blockIdx.x, tid = threadIdx.x, T = a.T;
    int Tb = T;
    if (a.n_valid) {
        int nv = a.n_valid[b];
        nv = nv < 0 ? 0 : (nv > a.n_samples ? a.n_samples : nv);
        Tb = (int)beat_frames_ll(nv);
    } else if (a.frames) {
        Tb = a.frames[b];
    }
    Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const float* __restrict__ e = a.envelope + (size_t)b * T;
    unsigned char* __restrict__ m = a.mask + (size_t)b * T;
    float mx = -__builtin_huge_valf();
    for (int t = tid; t < Tb; t += kBeatPickBlock) mx = fmaxf(mx, e[t]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    const double M = (double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const double thr = __dmul_rn(a.p.onset_delta, M);
    const int w = a.p.onset_window < T ? a.p.onset_window : T, aw = a.p.onset_avg_window < T ? a.p.onset_avg_window : T;   // (a window beyond the clip tests nothing more)
    for (int t = tid; t < T; t += kBeatPickBlock) {
        bool on = false;
        if (t < Tb && M > 0.0) {
            const double c = (double)e[t];
            on = true;
            for (int i = 1; i <= w && on && t - i >= 0; ++i) on = c > (double)e[t - i];
            for (int i = 1; i <= w && on && t + i < Tb; ++i) on = c >= (double)e[t + i];
            if (on) {
                const int lo = t - aw < 0 ? 0 : t - aw, hi = t + aw > Tb - 1 ? Tb - 1 : t + aw;
                double s = 0.0;
                for (int k = lo; k <= hi; ++k) s = __dadd_rn(s, (double)e[k]);
                on = c >= __dadd_rn(__ddiv_rn(s, (double)(hi - lo + 1)), thr);
            }
        }
        m[t] = on ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------- align
__device__ __forceinline__ double tau_audio(int t) { return (double)(kBeatHop * t + kBeatWin / 2) / (double)kBeatRate; }

// the first kept onset at or after ptr (t_end when there is none): bits at or beyond t_end are never set
__device__ __forceinline__ int next_onset(const unsigned* bits, int ptr, int t_end) {
    while (ptr < t_end) {
        const unsigned w = bits[ptr >> 5] >> (ptr & 31);
        if (w) return ptr + __ffs((int)w) - 1;
        ptr = (ptr | 31) + 1;
    }
    return t_end;
}

__global__ void __launch_bounds__(kBeatAlignBlock) k_beat_align(const BeatAlignArgs a) {
    __shared__ double ring[kBeatRing][64];
    __shared__ unsigned bits[kBeatMaxAudioFrames / 32];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int L = a.lengths[n];
    double* __restrict__ row = a.rows + (size_t)n * kBeatRow;
    unsigned char* __restrict__ bm = a.beat_mask ? a.beat_mask + (size_t)n * a.F * kSmplxJoints : nullptr;
    if (L < 2 || L > a.F) {                              // (uniform over the workgroup)
        for (int i = lane; i < kBeatRow; i += kBeatAlignBlock) row[i] = __builtin_nan("");
        if (bm)
            for (size_t i = lane; i < (size_t)a.F * kSmplxJoints; i += kBeatAlignBlock) bm[i] = 0;
        return;
    }
    const double fps = a.p.fps, two_s2 = 2.0 * a.p.sigma_s * a.p.sigma_s;
    int Ta = a.audio_frames[n];
    Ta = Ta < 0 ? 0 : (Ta > a.T ? a.T : Ta);
    // the onsets kept: frames t < t_end, the count of frames with tau_a <= (L - 1) / fps (tau_a ascends with t: a guess, then the exact comparison decides)
    const double lim = (double)(L - 1) / fps;
    const double guess = floor((lim * (double)kBeatRate - (double)(kBeatWin / 2)) / (double)kBeatHop) + 1.0;
    int t_end = !(guess > 0.0) ? 0 : (guess > (double)Ta ? Ta : (int)guess);
    while (t_end < Ta && tau_audio(t_end) <= lim) ++t_end;
    while (t_end > 0 && tau_audio(t_end - 1) > lim) --t_end;
    int n_on = 0;
    const unsigned char* __restrict__ om = a.onset_mask + (size_t)n * a.T;
    for (int base = 0; base < t_end; base += 64) {
        const int t = base + lane;
        const bool on = t < t_end && om[t] != 0;
        const unsigned long long bal = __ballot(on);
        if (lane == 0) {
            bits[base >> 5] = (unsigned)bal;
            bits[(base >> 5) + 1] = (unsigned)(bal >> 32);
        }
        n_on += __popcll(bal);
    }
    __syncthreads();

    const bool live = lane < kSmplxJoints;
    const int j = live ? lane : 0;                       // the nine idle lanes walk joint 0 and write nothing
    const float* __restrict__ X = a.joints + (size_t)n * a.F * (kSmplxJoints * 3) + j * 3;
    const int k = a.p.motion_order, R = 2 * k + 1, last = L - 2;
    double x0 = (double)X[0], y0 = (double)X[1], z0 = (double)X[2];
    int ptr = next_onset(bits, 0, t_end);                // the lane's next unsettled onset
    int prev_on = -1, last_beat = -1, nb = 0;
    double a2m = 0.0, m2a = 0.0;
    for (int f = 0; f <= last + k; ++f) {
        if (f <= last) {                                 // frames below L only: anything may sit beyond
            const float* __restrict__ p = X + (size_t)(f + 1) * (kSmplxJoints * 3);
            const double x1 = (double)p[0], y1 = (double)p[1], z1 = (double)p[2];
            const double dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
            ring[f % R][lane] = sqrt(dx * dx + dy * dy + dz * dz) * fps;
            x0 = x1; y0 = y1; z0 = z1;
        }
        const int g = f - k;                             // the frame whose 2 k neighbours are all in the ring now
        if (g < 0) continue;
        const double c = ring[g % R][lane];
        bool beat = true;
        for (int i = 1; i <= k; ++i) {
            const int lo = g - i < 0 ? 0 : g - i, hi = g + i > last ? last : g + i;     // clipped onto g itself: c < c fails
            beat = beat && c < ring[lo % R][lane] && c < ring[hi % R][lane];
        }
        if (bm && live) bm[(size_t)g * kSmplxJoints + j] = beat ? 1 : 0;
        if (!beat) continue;
        const double tm = ((double)g + 0.5) / fps;
        while (ptr < t_end) {                            // the onsets since the last beat, up to this one: each is nearest to one of the two
            const double ta = tau_audio(ptr);
            if (ta > tm) break;
            double d = tm - ta;
            if (last_beat >= 0) d = fmin(d, ta - ((double)last_beat + 0.5) / fps);
            a2m += exp(-(d * d) / two_s2);
            prev_on = ptr;
            ptr = next_onset(bits, ptr + 1, t_end);
        }
        if (n_on > 0) {                                  // the beat: nearest to the onset before or after the cursor
            double d = __builtin_huge_val();
            if (prev_on >= 0) d = tm - tau_audio(prev_on);
            if (ptr < t_end) d = fmin(d, tau_audio(ptr) - tm);
            m2a += exp(-(d * d) / two_s2);
        }
        last_beat = g;
        ++nb;
    }
    if (last_beat >= 0) {                                // the onsets after the last beat
        const double tl = ((double)last_beat + 0.5) / fps;
        while (ptr < t_end) {
            const double d = tau_audio(ptr) - tl;
            a2m += exp(-(d * d) / two_s2);
            ptr = next_onset(bits, ptr + 1, t_end);
        }
    }
    if (bm)
        for (size_t i = (size_t)(L - 1) * kSmplxJoints + lane; i < (size_t)a.F * kSmplxJoints; i += kBeatAlignBlock) bm[i] = 0;
    if (!live) return;
    if (j == 0) row[kBeatRowOnsets] = (double)n_on;
    row[kBeatRowBeats + j] = (double)nb;
    row[kBeatRowA2M + j] = nb > 0 ? a2m : 0.0;
    row[kBeatRowM2A + j] = m2a;
}

}  // namespace

hipError_t launch_beat_envelope(const BeatEnvArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_beat_envelope, dim3((unsigned)a.B * (unsigned)a.runs), dim3(kBeatEnvBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_beat_pick(const BeatPickArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_beat_pick, dim3((unsigned)a.B), dim3(kBeatPickBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_beat_align(const BeatAlignArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_beat_align, dim3((unsigned)a.N), dim3(kBeatAlignBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
