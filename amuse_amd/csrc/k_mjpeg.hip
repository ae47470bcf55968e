// Preview video (include/amuse_hip.h amuse_mjpeg_encode): RGB frames in device memory -> baseline JPEG files, back to back.  The format, the arithmetic and the
// passes are stated in amuse_mjpeg_host.hpp; this file holds the five kernels and their launchers.
//
// k_mjpeg_transform: 256 threads = 4 MCUs, one thread per pixel of an MCU.  The pixel (edge pixels repeated past the image) becomes Y - 128, Cb, Cr in fp32; the
// three 8 x 8 blocks go through the orthonormal DCT-II as two passes of 8-term fma chains over LDS (rows, then columns: D s D^T), are divided by the table,
// rounded half away from zero, clamped and stored as int16 at their zigzag position.  Bandwidth-trivial; no matrix core (fp32-input MFMA runs at the vector rate).
// k_mjpeg_size / k_mjpeg_write: ONE LANE PER INTERVAL (one MCU row).  The lane walks its 3 mcus_x blocks in order, 16 bytes of coefficients per load, and
// pushes (code, length) pairs through a 64-bit accumulator; the size kernel only counts the bytes, the write kernel stores each one at its exact place.  The
// work is serial and divergent inside a lane: the simple first form (a wave per interval with a prefix sum over its blocks is the next step).
// The Huffman words sit in LDS (2,176 bytes), where divergent lookups cost least.
// k_mjpeg_scan_intervals (one block per frame) and k_mjpeg_scan_frames (one block) turn sizes into offsets: exclusive sums in a fixed order, no atomics, so the
// same frame gives the same bytes at any position of any batch.
// Bounds: every store to `out` is `if (pos < out_capacity)`; the pixel index is clamped to the image; coefficient and interval indices are formed in size_t /
// long long from counts the host checked; no per-lane array is indexed at run time, so nothing goes to scratch.
#include "amuse_mjpeg_host.hpp"

#include <cstdint>

namespace amuse {

namespace {

// D[u][x] = 1/2 c(u) cos((2 x + 1) u pi / 16), c(0) = 1 / sqrt 2: F = D s D^T is the orthonormal DCT-II
__constant__ float kMjpegDct[64] = {
    0.353553385f, 0.353553385f,  0.353553385f,  0.353553385f,  0.353553385f,  0.353553385f,  0.353553385f,  0.353553385f,
    0.490392625f, 0.415734798f,  0.277785122f,  0.097545162f,  -0.097545162f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f,  -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f,  0.461939752f,
    0.415734798f, -0.097545162f, -0.490392625f, -0.277785122f, 0.277785122f,  0.490392625f,  0.097545162f,  -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,  0.353553385f,  -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.097545162f,  0.415734798f,  -0.415734798f, -0.097545162f, 0.490392625f,  -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f,  -0.191341713f, -0.191341713f, 0.461939752f,  -0.461939752f, 0.191341713f,
    0.097545162f, -0.277785122f, 0.415734798f,  -0.490392625f, 0.490392625f,  -0.415734798f, 0.277785122f,  -0.097545162f};
// natural index -> zigzag position (the inverse of kMjpegZigzag)
__constant__ unsigned char kMjpegUnzigzag[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                                 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__global__ void __launch_bounds__(kMjpegTransformMcus * 64) k_mjpeg_transform(const MjpegTransformArgs a) {
    __shared__ float s_dct[64];
    __shared__ float s_px[kMjpegTransformMcus][3][64];
    __shared__ float s_row[kMjpegTransformMcus][3][64];
    const int m = threadIdx.x >> 6, t = threadIdx.x & 63, x = t & 7, y = t >> 3;
    if (threadIdx.x < 64) s_dct[t] = kMjpegDct[t];
    const long long mcu = (long long)blockIdx.x * kMjpegTransformMcus + m;
    const bool live = mcu < a.mcus;
    if (live) {
        const long long per_frame = (long long)a.mcus_x * a.mcus_y;
        const long long f = mcu / per_frame;
        const int r = (int)(mcu - f * per_frame), my = r / a.mcus_x, mx = r - my * a.mcus_x;
        const int px = min(mx * 8 + x, a.W - 1), py = min(my * 8 + y, a.H - 1);      // the last column / row repeated
        const unsigned char* p = a.rgb + (((size_t)f * a.H + py) * a.W + px) * 3;
        const float R = (float)p[0], G = (float)p[1], B = (float)p[2];
        s_px[m][0][t] = fmaf(0.299f, R, fmaf(0.587f, G, fmaf(0.114f, B, -128.f)));
        s_px[m][1][t] = fmaf(-0.168735892f, R, fmaf(-0.331264108f, G, 0.5f * B));
        s_px[m][2][t] = fmaf(0.5f, R, fmaf(-0.418687589f, G, -0.081312411f * B));
    }
    __syncthreads();
    float dx[8], dy[8];                                  // row x and row y of D (indexed by the unrolled k only)
#pragma unroll
    for (int k = 0; k < 8; ++k) { dx[k] = s_dct[x * 8 + k]; dy[k] = s_dct[y * 8 + k]; }
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {                    // rows: this thread is (row y, horizontal frequency u = x)
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fmaf(s_px[m][c][y * 8 + k], dx[k], acc);
            s_row[m][c][t] = acc;
        }
    }
    __syncthreads();
    if (!live) return;
    const int zz = kMjpegUnzigzag[t];                   // natural index t = 8 v + u -> zigzag position
    short* out = a.coef + (size_t)mcu * 192;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                        // columns: (vertical frequency v = y, horizontal frequency u = x)
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = fmaf(dy[k], s_row[m][c][k * 8 + x], acc);
        const float q = acc / a.qdiv[(c ? 64 : 0) + zz];
        float r = truncf(q + copysignf(0.5f, q));        // half away from zero
        const float lo = t == 0 ? -1024.f : -1023.f, hi = 1023.f;
        r = fminf(fmaxf(r, lo), hi);
        out[c * 64 + zz] = (short)(int)r;
    }
}

// ------------------------------------------------------------------ entropy coding: one lane codes one interval, counting (WRITE = false) or storing
template <bool WRITE>
__device__ __forceinline__ void put_byte(unsigned b, unsigned char* out, unsigned long long cap, unsigned long long& pos) {
    if (WRITE) {
        if (pos < cap) out[pos] = (unsigned char)b;
    }
    ++pos;
    if (b == 0xFFu) {                                    // a data byte 0xFF is followed by 0x00
        if (WRITE) {
            if (pos < cap) out[pos] = 0;
        }
        ++pos;
    }
}

template <bool WRITE>
__device__ __forceinline__ void put_bits(unsigned long long& acc, int& n, unsigned bits, int len, unsigned char* out, unsigned long long cap,
                                         unsigned long long& pos) {
    acc = (acc << len) | bits;                           // len <= 26; at most 7 bits are pending, so the low 33 bits hold everything not yet emitted
    n += len;
    while (n >= 8) {
        n -= 8;
        put_byte<WRITE>((unsigned)(acc >> n) & 0xFFu, out, cap, pos);
    }
}

// the (code, length) of a value behind its run / size symbol: the category's code, then the value's low `cat` bits (negative: value - 1)
template <bool WRITE>
__device__ __forceinline__ void put_value(const unsigned int* huff, int symbol_hi, int v, unsigned long long& acc, int& n, unsigned char* out, unsigned long long cap,
                                          unsigned long long& pos) {
    const int av = v < 0 ? -v : v;
    const int cat = 32 - __clz(av);                      // 0 for v = 0 (DC only)
    const unsigned w = huff[symbol_hi | cat];
    const unsigned mag = (unsigned)(v - (v < 0 ? 1 : 0)) & ((1u << cat) - 1u);
    put_bits<WRITE>(acc, n, ((w & 0xFFFFu) << cat) | mag, (int)(w >> 16) + cat, out, cap, pos);
}

template <bool WRITE>
__device__ __forceinline__ unsigned long long code_interval(const short* coef, const unsigned int* s_huff, int mcus_x, unsigned char* out, unsigned long long cap,
                                                            unsigned long long pos) {
    unsigned long long acc = 0;
    int n = 0, pred0 = 0, pred1 = 0, pred2 = 0;
    const int blocks = mcus_x * 3;
    int c = 0;
    for (int b = 0; b < blocks; ++b) {
        const uint4* p = reinterpret_cast<const uint4*>(coef + (size_t)b * 64);
        const unsigned int* ac = s_huff + (c ? 256 : 0);
        const unsigned int* dc = s_huff + (c ? 528 : 512);
        int run = 0;
        for (int q = 0; q < 8; ++q) {
            const uint4 v = p[q];
            const unsigned long long lo = ((unsigned long long)v.y << 32) | v.x, hi = ((unsigned long long)v.w << 32) | v.z;
            for (int j = 0; j < 8; ++j) {
                const int val = (int)(short)(unsigned short)((j < 4 ? lo : hi) >> (16 * (j & 3)));
                if (q == 0 && j == 0) {
                    const int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
                    put_value<WRITE>(dc, 0, val - pred, acc, n, out, cap, pos);
                    if (c == 0) pred0 = val; else if (c == 1) pred1 = val; else pred2 = val;
                } else if (val == 0) {
                    ++run;
                } else {
                    while (run >= 16) {                  // ZRL: sixteen zeros
                        const unsigned w = ac[0xF0];
                        put_bits<WRITE>(acc, n, w & 0xFFFFu, (int)(w >> 16), out, cap, pos);
                        run -= 16;
                    }
                    put_value<WRITE>(ac, run << 4, val, acc, n, out, cap, pos);
                    run = 0;
                }
            }
        }
        if (run > 0) {                                   // EOB, unless coefficient 63 is non-zero
            const unsigned w = ac[0];
            put_bits<WRITE>(acc, n, w & 0xFFFFu, (int)(w >> 16), out, cap, pos);
        }
        c = c == 2 ? 0 : c + 1;
    }
    if (n > 0) put_byte<WRITE>((((unsigned)acc << (8 - n)) | ((1u << (8 - n)) - 1u)) & 0xFFu, out, cap, pos);      // padded with 1-bits
    return pos;
}

__device__ __forceinline__ void load_huff(unsigned int* s_huff, const unsigned int* huff) {
    for (int i = threadIdx.x; i < kMjpegHuffWords; i += kMjpegWave) s_huff[i] = huff[i];
    __syncthreads();
}

__global__ void __launch_bounds__(kMjpegWave) k_mjpeg_size(const MjpegEntropyArgs a) {
    __shared__ unsigned int s_huff[kMjpegHuffWords];
    load_huff(s_huff, a.huff);
    const long long i = (long long)blockIdx.x * kMjpegWave + threadIdx.x;      // frame x mcus_y + interval
    if (i >= (long long)a.frames * a.mcus_y) return;
    const int k = (int)(i % a.mcus_y);
    const unsigned long long bytes = code_interval<false>(a.coef + (size_t)i * a.mcus_x * 192, s_huff, a.mcus_x, nullptr, 0, k ? 2 : 0);   // (RSTm in front of k >= 1)
    a.interval_bytes[i] = (unsigned int)bytes;
}

// inclusive sum over the block's 256 lanes (Hillis-Steele in LDS); every lane of the block calls it
template <typename T>
__device__ __forceinline__ T block_inclusive(T v, T* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < kMjpegScanBlock; d <<= 1) {
        const T add = t >= d ? s[t - d] : (T)0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const T r = s[t];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kMjpegScanBlock) k_mjpeg_scan_intervals(const MjpegEntropyArgs a) {
    __shared__ unsigned int s[kMjpegScanBlock];
    const size_t base = (size_t)blockIdx.x * a.mcus_y;
    unsigned int carry = 0;
    for (int k0 = 0; k0 < a.mcus_y; k0 += kMjpegScanBlock) {
        const int k = k0 + threadIdx.x;
        const unsigned int v = k < a.mcus_y ? a.interval_bytes[base + k] : 0u;
        const unsigned int inc = block_inclusive(v, s);
        if (k < a.mcus_y) a.interval_offset[base + k] = carry + inc - v;
        s[threadIdx.x] = inc;
        __syncthreads();
        carry += s[kMjpegScanBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.frame_entropy[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kMjpegScanBlock) k_mjpeg_scan_frames(const MjpegEntropyArgs a) {
    __shared__ unsigned long long s[kMjpegScanBlock];
    unsigned long long carry = 0;
    for (int f0 = 0; f0 < a.frames; f0 += kMjpegScanBlock) {
        const int f = f0 + threadIdx.x;
        const unsigned int v = f < a.frames ? (unsigned int)a.header_bytes + a.frame_entropy[f] + 2u : 0u;      // SOI .. SOS, the intervals, EOI
        const unsigned long long inc = block_inclusive((unsigned long long)v, s);
        if (f < a.frames) {
            a.offsets[f] = carry + inc - v;
            a.sizes[f] = v;
        }
        s[threadIdx.x] = inc;
        __syncthreads();
        carry += s[kMjpegScanBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.total = carry;
}

__global__ void __launch_bounds__(kMjpegWave) k_mjpeg_write(const MjpegEntropyArgs a) {
    __shared__ unsigned int s_huff[kMjpegHuffWords];
    const int groups = (a.mcus_y + kMjpegWave - 1) / kMjpegWave;                // waves of intervals per frame; one more block per frame for header and EOI
    const int f = blockIdx.x / (groups + 1), g = blockIdx.x - f * (groups + 1);
    const unsigned long long at = a.offsets[f], cap = a.out_capacity;
    if (g == groups) {
        for (int i = threadIdx.x; i < a.header_bytes; i += kMjpegWave)
            if (at + i < cap) a.out[at + i] = a.header[i];
        if (threadIdx.x < 2) {
            const unsigned long long e = at + a.sizes[f] - 2 + threadIdx.x;
            if (e < cap) a.out[e] = threadIdx.x ? 0xD9 : 0xFF;
        }
        return;
    }
    load_huff(s_huff, a.huff);
    const int k = g * kMjpegWave + threadIdx.x;
    if (k >= a.mcus_y) return;
    const size_t i = (size_t)f * a.mcus_y + k;
    unsigned long long pos = at + (unsigned)a.header_bytes + a.interval_offset[i];
    if (k) {                                             // RSTm, m = (k - 1) mod 8: a marker, not stuffed
        if (pos < cap) a.out[pos] = 0xFF;
        if (pos + 1 < cap) a.out[pos + 1] = (unsigned char)(0xD0 + ((k - 1) & 7));
        pos += 2;
    }
    code_interval<true>(a.coef + i * a.mcus_x * 192, s_huff, a.mcus_x, a.out, cap, pos);
}

}  // namespace

hipError_t launch_mjpeg_transform(const MjpegTransformArgs& a, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a.mcus + kMjpegTransformMcus - 1) / kMjpegTransformMcus);      // the plan holds this below 2^31
    hipLaunchKernelGGL(k_mjpeg_transform, dim3(blocks), dim3(kMjpegTransformMcus * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mjpeg_size(const MjpegEntropyArgs& a, hipStream_t stream) {
    const long long n = (long long)a.frames * a.mcus_y;
    hipLaunchKernelGGL(k_mjpeg_size, dim3((unsigned)((n + kMjpegWave - 1) / kMjpegWave)), dim3(kMjpegWave), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mjpeg_scan(const MjpegEntropyArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_mjpeg_scan_intervals, dim3((unsigned)a.frames), dim3(kMjpegScanBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mjpeg_scan_frames, dim3(1), dim3(kMjpegScanBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mjpeg_write(const MjpegEntropyArgs& a, hipStream_t stream) {
    const long long groups = (a.mcus_y + kMjpegWave - 1) / kMjpegWave;
    hipLaunchKernelGGL(k_mjpeg_write, dim3((unsigned)((long long)a.frames * (groups + 1))), dim3(kMjpegWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
