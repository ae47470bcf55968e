// Stand-ins for the launchers of csrc/k_audio_tail.hip (amuse_audio_tail.hpp), beside tests/host_asan/hip_stub.cpp: the host code of AST_EVP's tail
// (amuse_audio_tail.hip: parameter walk, weight-stream packer, workspace, launch sequence) runs under ASan / UBSan without a GPU.  Launches are counted and
// their shapes checked against the workspace the host code allocates; "device" memory is host memory, so every pointer a launcher is handed is touched.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../amuse_amd/csrc/amuse_audio_tail.hpp"

static long g_launches = 0;
long amuse_tail_stub_launches() { return g_launches; }
static volatile float g_sink;
static void touch(const float* p, size_t n) { if (p && n) g_sink = p[0] + p[n - 1]; }   // ASan checks both ends of the range

namespace amuse {
hipError_t launch_tail_gemm(const TailGemmArgs& a, int precision, hipStream_t) {
    ++g_launches;
    if (a.B < 1 || a.B > kTailRows || a.N % kTailSpan || a.K % 64 || a.K > kTailMaxK) return hipErrorInvalidValue;
    touch(a.A, (size_t)a.B * a.K);
    touch(a.bias, a.N);
    const unsigned short* w = static_cast<const unsigned short*>(a.W);
    g_sink = (float)(w[0] + w[(size_t)a.N * a.K * (precision == 2 ? 2 : 1) - 1]);
    for (int b = 0; b < a.B; ++b) a.out[(size_t)b * a.N] = a.out[(size_t)b * a.N + a.N - 1] = 0.f;
    return hipSuccess;
}
hipError_t launch_tail_linear(const float* A, const float* W, const float* bias, int B, int N, int K, int, float* out, hipStream_t) {
    ++g_launches;
    touch(A, (size_t)B * K); touch(W, (size_t)N * K); touch(bias, N);
    out[0] = out[(size_t)B * N - 1] = 0.f;
    return hipSuccess;
}
hipError_t launch_tail_attn(const float* qkv, int B, int S, int D, float* out, hipStream_t) {
    ++g_launches;
    if (S < 1 || S > kTailMaxGroup || B % S) return hipErrorInvalidValue;
    touch(qkv, (size_t)B * 3 * D);
    out[0] = out[(size_t)B * D - 1] = 0.f;
    return hipSuccess;
}
hipError_t launch_tail_add_ln(const float* x, const float* y, const float* gamma, const float* beta, int B, int D, float* out, hipStream_t) {
    ++g_launches;
    touch(x, (size_t)B * D); touch(y, y ? (size_t)B * D : 0); touch(gamma, D); touch(beta, D);
    out[0] = out[(size_t)B * D - 1] = 0.f;
    return hipSuccess;
}
hipError_t launch_tail_cat(const float* emo, const float* sty, const float* con, int B, float* out, hipStream_t) {
    ++g_launches;
    touch(emo, (size_t)B * 256); touch(sty, (size_t)B * 256); touch(con, (size_t)B * 256);
    out[0] = out[(size_t)B * 768 - 1] = 0.f;
    return hipSuccess;
}
hipError_t launch_tail_head(const float* in, int slices, float, int D, const float* gamma, const float* beta, const float* W, const float* bias, int L, float* out, int B,
                            hipStream_t) {
    ++g_launches;
    touch(in, (size_t)B * (slices > 0 ? slices : 1) * D); touch(gamma, D); touch(beta, D); touch(W, (size_t)L * D); touch(bias, L);
    out[0] = out[(size_t)B * L - 1] = 0.f;
    return hipSuccess;
}
}  // namespace amuse
