// Stand-ins for the HIP runtime and for the kernel launchers, so that the library's HOST code (context construction, weight
// packing into MFMA-fragment streams, workspace management, argument checking: amuse_api.hip, amuse_audio_api.hip) can run under
// AddressSanitizer / UBSan on a machine without a GPU.  "Device" memory is host memory; launches are no-ops.  Test
// infrastructure only (tests/test_host_asan.py builds it) - never linked into libamuse_hip.so.
//
// The image log (amuse_stub_log(1), off by default; tests/test_pack_images_cpu.py): every host-to-"device" hipMemcpy prints its size, a 64-bit FNV-1a digest
// and its first word; every launcher that takes a weight stream prints the digest of the image behind `wstream` and the stage / unit tables it is handed;
// launch_repack prints element count, kind, the image it overwrites and a digest of its gather map.  That pins every byte the packers produce on any machine.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../amuse_amd/csrc/amuse_audio.hpp"
#include "../../amuse_amd/csrc/amuse_kernels.hpp"

static long g_live = 0;
long amuse_stub_live_allocations() { return g_live; }

static bool g_log = false;
static std::map<const void*, uint64_t> g_image;   // "device" pointer -> digest of the last upload to it (while the log is on)
void amuse_stub_log(int on) { g_log = on != 0; }
static uint64_t fnv1a(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
static unsigned long long image_of(const void* p) {
    const auto it = g_image.find(p);
    return it == g_image.end() ? 0ull : (unsigned long long)it->second;
}
static void log_upload(const void* d, const void* s, size_t n) {
    uint32_t first = 0;
    memcpy(&first, s, n < 4 ? n : 4);
    const uint64_t h = fnv1a(s, n);
    g_image[d] = h;
    printf("upload bytes=%zu digest=%016llx first=%08x\n", n, (unsigned long long)h, first);
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); ++g_live; return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { if (p) { if (g_log) g_image.erase(p); free(p); --g_live; } return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) {
    if (g_log && k == hipMemcpyHostToDevice) log_upload(d, s, n);
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = reinterpret_cast<hipStream_t>(malloc(8)); ++g_live; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); --g_live; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(malloc(8)); ++g_live; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); --g_live; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
}

namespace amuse {
static hipError_t log_sample(const char* name, const SampleArgs& a, int prec) {
    if (g_log) printf("%s prec=%d image=%016llx wave_units=%u a=%u b=%u\n", name, prec, image_of(a.wstream), a.wave_units, a.wave_units_a, a.wave_units_b);
    return hipSuccess;
}
static hipError_t log_rows(const char* name, const VaeRowsArgs& a, int prec, int mode) {
    if (g_log)
        printf("%s prec=%d mode=%d stage=%d image=%016llx stage_base=%016llx stage_units=%016llx\n", name, prec, mode, a.stage, image_of(a.wstream),
               (unsigned long long)fnv1a(a.stage_base, sizeof(a.stage_base)), (unsigned long long)fnv1a(a.stage_units, sizeof(a.stage_units)));
    return hipSuccess;
}
static hipError_t log_stream(const char* name, const void* wstream) {
    if (g_log) printf("%s image=%016llx\n", name, image_of(wstream));
    return hipSuccess;
}
hipError_t launch_sample(const SampleArgs& a, int prec, hipStream_t) { return log_sample("launch_sample", a, prec); }
hipError_t launch_sample8(const SampleArgs& a, hipStream_t) { return log_sample("launch_sample8", a, -1); }
hipError_t launch_sample8x(const SampleArgs& a, hipStream_t) { return log_sample("launch_sample8x", a, -1); }
hipError_t launch_sample8h(const SampleArgs& a, hipStream_t) { return log_sample("launch_sample8h", a, -1); }
hipError_t launch_time_tokens(const int*, int, const float*, const float*, const float*, const float*, const float*, const float*, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_cond_tokens(const CondArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_repack(const float*, const int* map, void* dst, size_t n, int kind, hipStream_t) {   // (the gather map is host memory here)
    if (g_log) printf("launch_repack n=%zu kind=%d image=%016llx map=%016llx\n", n, kind, image_of(dst), (unsigned long long)fnv1a(map, n * sizeof(int)));
    return hipSuccess;
}
hipError_t launch_add_noise(const float*, const float*, const float*, const float*, float*, int, hipStream_t, int) { return hipSuccess; }
hipError_t launch_counter_normal(uint64_t, uint64_t, int, int, int, float*, hipStream_t, int) { return hipSuccess; }
hipError_t launch_vae_rows(const VaeRowsArgs& a, int prec, int mode, hipStream_t) { return log_rows("launch_vae_rows", a, prec, mode); }
hipError_t launch_vae_rows8x(const VaeRowsArgs& a, hipStream_t, int mode) { return log_rows("launch_vae_rows8x", a, -1, mode); }
hipError_t launch_vae_attn(const VaeAttnArgs&, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_vae_fused(const VaeFusedArgs& a, hipStream_t) { return log_stream("launch_vae_fused", a.wstream); }
hipError_t launch_vae_fusedh(const VaeFusedArgs& a, hipStream_t) { return log_stream("launch_vae_fusedh", a.wstream); }
hipError_t launch_den_fused(const DenFusedArgs& a, hipStream_t) { return log_stream("launch_den_fused", a.wstream); }
hipError_t launch_den_fusedh(const DenFusedArgs& a, hipStream_t) { return log_stream("launch_den_fusedh", a.wstream); }
hipError_t launch_vae_fusedx(const VaeFusedXArgs& a, hipStream_t) { return log_stream("launch_vae_fusedx", a.wstream); }
hipError_t launch_den_fusedx(const DenFusedXArgs& a, hipStream_t) { return log_stream("launch_den_fusedx", a.wstream); }
hipError_t launch_sample_dec(const SampleDecArgs& a, int prec, hipStream_t) {
    if (g_log) printf("launch_sample_dec prec=%d image=%016llx wave_units=%u\n", prec, image_of(a.wstream), a.wave_units);
    return hipSuccess;
}
hipError_t launch_mem_kv(const float*, int, const float*, const float*, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_feats_to_smplx(const float*, size_t, int, float*, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_smplx_to_feats(const float*, const float*, size_t, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_vae_latent(const float*, const float*, float*, float*, float*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_vae_ca(const float*, const float*, const float*, const float*, const float*, float*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_gemm(const GemmArgs&, int, hipStream_t) { return hipSuccess; }
hipError_t launch_fbank(const float*, int, int, const float*, const float*, const int*, float, float, float*, hipStream_t) { return hipSuccess; }
hipError_t launch_im2col(const float*, unsigned short*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_ast_tokens(const float*, const float*, const float*, float*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_ln_bf16(const float*, const float*, const float*, float, unsigned short*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_tile_bf16(const unsigned short*, unsigned short*, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_untile_bf16(const unsigned short*, unsigned short*, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_untile_f32(const float*, float*, int, int, int, int, hipStream_t) { return hipSuccess; }
hipError_t launch_ast_attn(const unsigned short*, const unsigned short*, unsigned short*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_ast_pool(const float*, const float*, const float*, int, float*, int, hipStream_t) { return hipSuccess; }
hipError_t launch_ast_head(const float*, int, const float*, const float*, const unsigned short*, const float*, float*, int, hipStream_t) { return hipSuccess; }
}  // namespace amuse
