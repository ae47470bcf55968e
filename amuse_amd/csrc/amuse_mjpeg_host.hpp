// Preview video (include/amuse_hip.h amuse_mjpeg_*): everything the baseline JPEG encoder needs on the host, shared by k_mjpeg.hip (the kernels and their
// launchers), amuse_mjpeg.hip (the C entry points) and tests/mjpeg_host (the same host code on stand-in launchers, under sanitizers).
// AN EXTENSION: the reference hands its frames to ffmpeg; this writes Motion-JPEG frames for an AVI (amuse_amd/video.py) and is compared with libjpeg through
// PIL only (tests/mjpeg_ref.py restates it).
//
// THE FORMAT, stated once.  Baseline sequential DCT (SOF0), 8 bit, three components Y Cb Cr with H = V = 1 (no chroma subsampling), interleaved in one scan: one
// MCU is one 8 x 8 block per component, in the order Y, Cb, Cr.  Segments, in this order: SOI, APP0 (JFIF 1.01, aspect 1:1), DQT luma, DQT chroma, SOF0 with the
// true width and height, DHT DC luma, DHT AC luma, DHT DC chroma, DHT AC chroma (the "typical" tables of ITU-T T.81 Annex K.3), DRI, SOS, entropy data, EOI.
// The restart interval is one MCU row, Ri = mcus_x = ceil(W / 8): interval k >= 1 is preceded by RSTm, m = (k - 1) mod 8; the DC predictors are 0 at the start
// of every interval; every interval is padded to a byte with 1-bits; every 0xFF data byte is followed by 0x00.  So every interval is byte-aligned and independent
// of the others, which is what the entropy kernels divide the work by.
// Quantisation tables from quality 1..100 by libjpeg's rule on the Annex K.1 / K.2 tables: s = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((base s + 50) / 100, 1,
// 255) (integer arithmetic).
// THE PASSES of a call (all on the caller's stream, nothing allocated, nothing synchronised):
//   transform  RGB -> Y Cb Cr (fp32, not rounded) -> 8 x 8 DCT-II -> F / t rounded half away from zero, clamped -> int16 [M][mcus_y][mcus_x][3][64], zigzag order
//   size       one lane per interval: the bytes its entropy coding takes (the RST marker in front of intervals >= 1 included)
//   scan       per frame the exclusive sum of its intervals; over the frames the exclusive sum of the frame sizes (64 bit) -> offsets, sizes, total
//   write      one lane per interval codes it again and stores every byte at its exact place, each store checked against out_capacity; one more wave per
//              frame copies the header and writes EOI
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"

namespace amuse {

constexpr int kMjpegMaxSide = 4096;
constexpr int kMjpegBlockBits = 1660;         // the most one block can take: DC 11 + 11 bits, 63 AC of 16 + 10 bits
constexpr int kMjpegTransformMcus = 4;        // MCUs per block of the transform kernel (64 threads each)
constexpr int kMjpegWave = 64;                // threads per block of the entropy kernels: one lane per interval
constexpr int kMjpegScanBlock = 256;
constexpr int kMjpegHuffWords = 2 * 256 + 2 * 16;   // AC luma, AC chroma, DC luma, DC chroma: (length << 16) | code

// ITU-T T.81 Annex K.1 / K.2, natural (row-major) order
constexpr unsigned char kMjpegBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                              14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kMjpegBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                                47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zigzag position k -> natural index
constexpr unsigned char kMjpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.3: the number of codes of each length 1..16, then the symbols in code order
constexpr unsigned char kMjpegDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kMjpegDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kMjpegDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kMjpegAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr unsigned char kMjpegAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1,
    0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
    0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
constexpr unsigned char kMjpegAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr unsigned char kMjpegAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1,
    0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
    0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
    0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

struct MjpegTransformArgs {
    const unsigned char* rgb;    // [frames][H][W][3]
    short* coef;                 // [frames][mcus_y][mcus_x][3][64], zigzag order
    const float* qdiv;           // [2][64]: luma, chroma divisors in zigzag order
    int W, H, mcus_x, mcus_y;
    long long mcus;              // frames x mcus_y x mcus_x
};

struct MjpegEntropyArgs {
    const short* coef;
    const unsigned int* huff;           // [kMjpegHuffWords]
    const unsigned char* header;        // [header_bytes]
    unsigned int* interval_bytes;       // [frames][mcus_y]
    unsigned int* interval_offset;      // [frames][mcus_y]: exclusive sum inside the frame
    unsigned int* frame_entropy;        // [frames]: the sum of a frame's intervals
    unsigned char* out;
    unsigned long long out_capacity;
    unsigned long long* offsets;        // [frames]
    unsigned int* sizes;                // [frames]
    unsigned long long* total;
    int mcus_x, mcus_y, frames, header_bytes;
};

// k_mjpeg.hip (tests/mjpeg_host: stand-ins that record the arguments)
hipError_t launch_mjpeg_transform(const MjpegTransformArgs& a, hipStream_t stream);
hipError_t launch_mjpeg_size(const MjpegEntropyArgs& a, hipStream_t stream);
hipError_t launch_mjpeg_scan(const MjpegEntropyArgs& a, hipStream_t stream);
hipError_t launch_mjpeg_write(const MjpegEntropyArgs& a, hipStream_t stream);

inline size_t mjpeg_align(size_t n) { return (n + 255) & ~(size_t)255; }

inline int mjpeg_tables(int quality, unsigned char* luma, unsigned char* chroma) {
    if (quality < 1 || quality > 100) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg: quality %d outside 1..100", quality);
    if (!luma || !chroma) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg_tables: luma_q64 and chroma_q64 must be given");
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (kMjpegBaseLuma[i] * s + 50) / 100, c = (kMjpegBaseChroma[i] * s + 50) / 100;
        luma[i] = (unsigned char)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[i] = (unsigned char)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    return AMUSE_OK;
}

inline int mjpeg_check_size(int width, int height) {
    if (width < 1 || width > kMjpegMaxSide || height < 1 || height > kMjpegMaxSide)
        return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg: %d x %d outside 1..%d per axis", width, height, kMjpegMaxSide);
    return AMUSE_OK;
}

inline void mjpeg_segment(std::vector<unsigned char>& h, int marker, const std::vector<unsigned char>& body) {
    const size_t n = body.size() + 2;
    h.push_back(0xFF); h.push_back((unsigned char)marker);
    h.push_back((unsigned char)(n >> 8)); h.push_back((unsigned char)(n & 255));
    h.insert(h.end(), body.begin(), body.end());
}

inline void mjpeg_dht(std::vector<unsigned char>& h, int tc_th, const unsigned char* bits, const unsigned char* vals, int n) {
    std::vector<unsigned char> b;
    b.push_back((unsigned char)tc_th);
    b.insert(b.end(), bits, bits + 16);
    b.insert(b.end(), vals, vals + n);
    mjpeg_segment(h, 0xC4, b);
}

// SOI .. SOS of a frame: the same bytes for every frame of an encoder
inline std::vector<unsigned char> mjpeg_header(int width, int height, const unsigned char* luma, const unsigned char* chroma) {
    std::vector<unsigned char> h = {0xFF, 0xD8};
    mjpeg_segment(h, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        std::vector<unsigned char> b(65);
        b[0] = (unsigned char)t;
        for (int k = 0; k < 64; ++k) b[1 + k] = (t ? chroma : luma)[kMjpegZigzag[k]];
        mjpeg_segment(h, 0xDB, b);
    }
    mjpeg_segment(h, 0xC0, {8, (unsigned char)(height >> 8), (unsigned char)(height & 255), (unsigned char)(width >> 8), (unsigned char)(width & 255), 3,
                            1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    mjpeg_dht(h, 0x00, kMjpegDcLumaBits, kMjpegDcVals, 12);
    mjpeg_dht(h, 0x10, kMjpegAcLumaBits, kMjpegAcLumaVals, 162);
    mjpeg_dht(h, 0x01, kMjpegDcChromaBits, kMjpegDcVals, 12);
    mjpeg_dht(h, 0x11, kMjpegAcChromaBits, kMjpegAcChromaVals, 162);
    const int ri = (width + 7) / 8;
    mjpeg_segment(h, 0xDD, {(unsigned char)(ri >> 8), (unsigned char)(ri & 255)});
    mjpeg_segment(h, 0xDA, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return h;
}

inline size_t mjpeg_header_bytes() {
    return 2 + 18 + 2 * 69 + 19 + 2 * (4 + 17 + 12) + 2 * (4 + 17 + 162) + 6 + 14;
}

// (length << 16) | code of every symbol, by Annex C: codes of one length are consecutive, the first of a length is the last of the shorter one, plus 1, doubled
inline void mjpeg_codes(const unsigned char* bits, const unsigned char* vals, unsigned int* out, int slots) {
    for (int i = 0; i < slots; ++i) out[i] = 0;
    unsigned int code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((unsigned)len << 16) | code++;
        code <<= 1;
    }
}

inline void mjpeg_huff_words(unsigned int* w) {
    mjpeg_codes(kMjpegAcLumaBits, kMjpegAcLumaVals, w, 256);
    mjpeg_codes(kMjpegAcChromaBits, kMjpegAcChromaVals, w + 256, 256);
    mjpeg_codes(kMjpegDcLumaBits, kMjpegDcVals, w + 512, 16);
    mjpeg_codes(kMjpegDcChromaBits, kMjpegDcVals, w + 528, 16);
}

struct MjpegPlan {
    int mcus_x, mcus_y, header_bytes;
    size_t coef_bytes, interval_bytes, frame_bytes, workspace_bytes, worst_case_bytes_per_frame;   // the sections of the workspace: coefficients | interval
                                                                                                   // sizes | interval offsets | frame sums
};

inline int mjpeg_plan(int width, int height, int frames, MjpegPlan* p) {
    if (int rc = mjpeg_check_size(width, height)) return rc;
    if (frames < 1) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg: frames %d < 1", frames);
    p->mcus_x = (width + 7) / 8;
    p->mcus_y = (height + 7) / 8;
    p->header_bytes = (int)mjpeg_header_bytes();
    const long long mcus = (long long)frames * p->mcus_x * p->mcus_y;
    // the launches index blocks with 32 bits: the transform takes mcus / 4 of them, the entropy passes at most frames x (mcus_y / 64 + 2)
    if ((mcus + kMjpegTransformMcus - 1) / kMjpegTransformMcus > INT_MAX || (long long)frames * ((p->mcus_y + kMjpegWave - 1) / kMjpegWave + 1) > INT_MAX)
        return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg: %d frames of %d x %d MCUs are more than one call's launches can index", frames, p->mcus_x, p->mcus_y);
    p->coef_bytes = mjpeg_align((size_t)mcus * 3 * 64 * sizeof(short));
    p->interval_bytes = mjpeg_align((size_t)frames * p->mcus_y * sizeof(unsigned int));
    p->frame_bytes = mjpeg_align((size_t)frames * sizeof(unsigned int));
    p->workspace_bytes = p->coef_bytes + 2 * p->interval_bytes + p->frame_bytes;
    const size_t interval_worst = 2 * (((size_t)p->mcus_x * 3 * kMjpegBlockBits + 7) / 8);      // every byte 0xFF and stuffed
    p->worst_case_bytes_per_frame = (size_t)p->header_bytes + (size_t)p->mcus_y * interval_worst + 2 * (size_t)(p->mcus_y - 1) + 2;
    return AMUSE_OK;
}

struct Mjpeg {
    int device, W, H, quality, reserved_frames;
    unsigned char* header_dev;   // [header_bytes]
    unsigned int* huff_dev;      // [kMjpegHuffWords]
    float* qdiv_dev;             // [2][64]
    char* ws;
    size_t ws_bytes;
    std::vector<void*> retired;   // workspaces outgrown by a later reserve: kept until destroy
};

inline Mjpeg* mjpeg_create(int device, int width, int height, int quality) {
    unsigned char luma[64], chroma[64];
    if (mjpeg_check_size(width, height) || mjpeg_tables(quality, luma, chroma)) return nullptr;
    const std::vector<unsigned char> header = mjpeg_header(width, height, luma, chroma);
    unsigned int huff[kMjpegHuffWords];
    mjpeg_huff_words(huff);
    float qdiv[128];
    for (int k = 0; k < 64; ++k) { qdiv[k] = (float)luma[kMjpegZigzag[k]]; qdiv[64 + k] = (float)chroma[kMjpegZigzag[k]]; }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { amuse_failf(AMUSE_EHIP, "amuse_mjpeg_create: hipSetDevice(%d): %s", device, hipGetErrorString(e)); return nullptr; }
    Mjpeg* m = new Mjpeg{device, width, height, quality, 0, nullptr, nullptr, nullptr, nullptr, 0, {}};
    struct { void** dst; const void* src; size_t bytes; } up[3] = {{reinterpret_cast<void**>(&m->header_dev), header.data(), header.size()},
                                                                  {reinterpret_cast<void**>(&m->huff_dev), huff, sizeof(huff)},
                                                                  {reinterpret_cast<void**>(&m->qdiv_dev), qdiv, sizeof(qdiv)}};
    for (auto& u : up) {
        e = hipMalloc(u.dst, u.bytes);
        if (e == hipSuccess) e = hipMemcpy(*u.dst, u.src, u.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            amuse_failf(AMUSE_ENOMEM, "amuse_mjpeg_create: %zu bytes of tables: %s", u.bytes, hipGetErrorString(e));
            (void)hipFree(m->header_dev); (void)hipFree(m->huff_dev); (void)hipFree(m->qdiv_dev);
            delete m;
            return nullptr;
        }
    }
    return m;
}

inline void mjpeg_destroy(Mjpeg* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipFree(m->header_dev); (void)hipFree(m->huff_dev); (void)hipFree(m->qdiv_dev);
    (void)hipFree(m->ws);
    for (void* p : m->retired) (void)hipFree(p);
    delete m;
}

// the workspace for calls of up to `frames` frames: grows only; an outgrown block is kept until destroy, so that work already queued on it stays valid
inline int mjpeg_reserve(Mjpeg* m, int frames) {
    if (!m) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg_reserve: encoder is NULL");
    MjpegPlan p{};
    if (int rc = mjpeg_plan(m->W, m->H, frames, &p)) return rc;
    if (frames <= m->reserved_frames) return AMUSE_OK;
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_mjpeg_reserve: hipSetDevice(%d): %s", m->device, hipGetErrorString(e));
    char* ws = nullptr;
    e = hipMalloc(reinterpret_cast<void**>(&ws), p.workspace_bytes);
    if (e != hipSuccess) return amuse_failf(AMUSE_ENOMEM, "amuse_mjpeg_reserve: %zu bytes of workspace: %s", p.workspace_bytes, hipGetErrorString(e));
    if (m->ws) m->retired.push_back(m->ws);
    m->ws = ws;
    m->ws_bytes = p.workspace_bytes;
    m->reserved_frames = frames;
    return AMUSE_OK;
}

inline int mjpeg_transform(Mjpeg* m, const unsigned char* rgb, int M, short* coef, const MjpegPlan& p, hipStream_t stream, const char* who) {
    MjpegTransformArgs ta{};
    ta.rgb = rgb; ta.coef = coef; ta.qdiv = m->qdiv_dev;
    ta.W = m->W; ta.H = m->H; ta.mcus_x = p.mcus_x; ta.mcus_y = p.mcus_y;
    ta.mcus = (long long)M * p.mcus_x * p.mcus_y;
    const hipError_t e = launch_mjpeg_transform(ta, stream);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "%s: transform launch failed: %s", who, hipGetErrorString(e));
    return AMUSE_OK;
}

inline int mjpeg_encode(Mjpeg* m, const unsigned char* rgb, int M, unsigned char* out, size_t out_capacity, unsigned long long* offsets, unsigned int* sizes,
                        unsigned long long* total, hipStream_t stream) {
    if (!m) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg_encode: encoder is NULL");
    if (!rgb || !out || !offsets || !sizes || !total) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg_encode: rgb, out, offsets, sizes and total must be given");
    if (M < 1) return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg_encode: M %d < 1", M);
    if (M > m->reserved_frames)
        return amuse_failf(AMUSE_EINVAL, "amuse_mjpeg_encode: M %d above the %d frames reserved (amuse_mjpeg_reserve first: a call allocates nothing)", M, m->reserved_frames);
    MjpegPlan p{};
    if (int rc = mjpeg_plan(m->W, m->H, M, &p)) return rc;
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_mjpeg_encode: hipSetDevice(%d): %s", m->device, hipGetErrorString(e));
    short* coef = reinterpret_cast<short*>(m->ws);
    if (int rc = mjpeg_transform(m, rgb, M, coef, p, stream, "amuse_mjpeg_encode")) return rc;
    MjpegEntropyArgs ea{};
    ea.coef = coef; ea.huff = m->huff_dev; ea.header = m->header_dev;
    ea.interval_bytes = reinterpret_cast<unsigned int*>(m->ws + p.coef_bytes);
    ea.interval_offset = reinterpret_cast<unsigned int*>(m->ws + p.coef_bytes + p.interval_bytes);
    ea.frame_entropy = reinterpret_cast<unsigned int*>(m->ws + p.coef_bytes + 2 * p.interval_bytes);
    ea.out = out; ea.out_capacity = out_capacity; ea.offsets = offsets; ea.sizes = sizes; ea.total = total;
    ea.mcus_x = p.mcus_x; ea.mcus_y = p.mcus_y; ea.frames = M; ea.header_bytes = p.header_bytes;
    if ((e = launch_mjpeg_size(ea, stream)) != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_mjpeg_encode: size launch failed: %s", hipGetErrorString(e));
    if ((e = launch_mjpeg_scan(ea, stream)) != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_mjpeg_encode: scan launch failed: %s", hipGetErrorString(e));
    if ((e = launch_mjpeg_write(ea, stream)) != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_mjpeg_encode: write launch failed: %s", hipGetErrorString(e));
    return AMUSE_OK;
}

// tests: the transform alone, into the caller's array (no workspace)
inline int mjpeg_coefficients(Mjpeg* m, const unsigned char* rgb, int M, short* coef, hipStream_t stream) {
    if (!m) return amuse_failf(AMUSE_EINVAL, "amuse_debug_mjpeg_coefficients: encoder is NULL");
    if (!rgb || !coef) return amuse_failf(AMUSE_EINVAL, "amuse_debug_mjpeg_coefficients: rgb and coef must be given");
    if (M < 1) return amuse_failf(AMUSE_EINVAL, "amuse_debug_mjpeg_coefficients: M %d < 1", M);
    MjpegPlan p{};
    if (int rc = mjpeg_plan(m->W, m->H, M, &p)) return rc;
    const hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return amuse_failf(AMUSE_EHIP, "amuse_debug_mjpeg_coefficients: hipSetDevice(%d): %s", m->device, hipGetErrorString(e));
    return mjpeg_transform(m, rgb, M, coef, p, stream, "amuse_debug_mjpeg_coefficients");
}

}  // namespace amuse
