// Stand-ins for the HIP runtime and for the kernel launchers, so that the library's HOST code (context construction, weight
// packing into MFMA-fragment streams, workspace management, argument checking: amuse_api.hip, amuse_audio_api.hip) can run under
// AddressSanitizer / UBSan on a machine without a GPU.  "Device" memory is host memory; launches are no-ops.  Test
// infrastructure only (tests/test_host_asan.py builds it) - never linked into libamuse_hip.so.
//
// The image log (amuse_stub_log(1), off by default; tests/test_pack_images_cpu.py): every host-to-"device" hipMemcpy prints its size, a 64-bit FNV-1a digest
// and its first word; every launcher that takes a weight stream prints the digest of the image behind `wstream` and the stage / unit tables it is handed;
// launch_repack prints element count, kind, the image it overwrites and a digest of its gather map.  That pins every byte the packers produce on any machine.
//
// The launch log (amuse_stub_log(2); tests/test_launch_args_cpu.py): one line per runtime call and per launch, in order - every launcher prints its name, its stream and
// every field of its argument struct, hipMalloc / hipFree the block's size, the copies and memsets kind, size and pointers, hipEventRecord / hipStreamWaitEvent their
// event and stream.  Pointers are printed so that the text is the same on any machine: `0`, `dev#<n>+<offset>/<block size>` inside the process's n-th hipMalloc block while it is live,
// `<name>+<offset>` inside a buffer the driver registered (amuse_stub_name), `host` otherwise; streams and events by their order of creation; weight streams also
// by image digest, stage tables as digests.  That pins what the image log leaves open: workspace carving, chunk offsets, the hoist launches and launch order.
// The raw launch log (amuse_stub_log(3); tests/test_train_launch_args_cpu.py): the launch log, and beneath the launchers: the training step's translation units are
// linked as they are, so their kernels register here (__hipRegisterFunction hands over each kernel's mangled name) and every <<< >>> arrives as hipLaunchKernel -
// one line with the kernel's name, grid, block, dynamic LDS, stream and, through the driver's table of parameter letters (amuse_stub_kernel_params), its arguments.
// Stream / event creation, hipFuncSetAttribute and hipDeviceSynchronize print a line at this level too.  amuse_stub_fail_at(n) makes the n-th of these calls and
// launches fail (a failed launch is what the next hipGetLastError returns).
// The audio front-end's launchers print into the launch log only (tests/test_audio_launch_args_cpu.py); the line itself, struct Line, is in stub_log.hpp.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../amuse_amd/csrc/amuse_audio.hpp"
#include "../../amuse_amd/csrc/amuse_kernels.hpp"
#include "stub_log.hpp"

static long g_live = 0;
long amuse_stub_live_allocations() { return g_live; }

static int g_level = 0;        // 0 off | 1 image log | 2 launch log
static bool g_log = false;     // the image log's lines
static bool g_raw = false;     // the raw launch log's lines (level 3: the launch log + raw launches, creations, function attributes)
static std::map<const void*, uint64_t> g_image;   // "device" pointer -> digest of the last upload to it (while a log is on)
void amuse_stub_log(int on) { g_level = on == 3 ? 2 : on; g_log = on == 1; g_raw = on == 3; }
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
    if (g_log) printf("upload bytes=%zu digest=%016llx first=%08x\n", n, (unsigned long long)h, first);
}

// ---- the launch log's vocabulary
struct Range { size_t bytes; std::string name; };
struct Block { size_t bytes; int id; };
static std::map<const char*, Block> g_blocks;    // live hipMalloc blocks; id = the n-th hipMalloc of the process
static int g_nblocks = 0;
static std::map<const char*, Range> g_named;      // the driver's buffers (amuse_stub_name)
static std::map<const void*, int> g_streams, g_events;
static int g_nstreams = 0, g_nevents = 0;
void amuse_stub_name(const char* name, const void* p, size_t bytes) {
    if (bytes) g_named[static_cast<const char*>(p)] = {bytes, name};
    else g_named.erase(static_cast<const char*>(p));
}
static std::string ptr_text(const void* pv) {
    const char* p = static_cast<const char*>(pv);
    if (!p) return "0";
    char buf[96];
    auto b = g_blocks.upper_bound(p);
    if (b != g_blocks.begin() && (size_t)(p - (--b)->first) <= b->second.bytes) {   // (one past the end is still that block: the tail of a carve)
        snprintf(buf, sizeof(buf), "dev#%d+%zu/%zu", b->second.id, (size_t)(p - b->first), b->second.bytes);
        return buf;
    }
    auto r = g_named.upper_bound(p);
    if (r != g_named.begin() && (size_t)(p - (--r)->first) <= r->second.bytes) {
        snprintf(buf, sizeof(buf), "%s+%zu", r->second.name.c_str(), (size_t)(p - r->first));
        return buf;
    }
    return "host";
}
static std::string handle_text(const std::map<const void*, int>& ids, const void* h) {
    if (!h) return "0";
    const auto it = ids.find(h);
    return it == ids.end() ? "?" : "#" + std::to_string(it->second);
}
// one line of the launch log: struct Line of stub_log.hpp, which reads this file's tables through these four
int amuse_stub_log_level() { return g_level; }
std::string amuse_stub_ptr_text(const void* p) { return ptr_text(p); }
std::string amuse_stub_stream_text(hipStream_t s) { return handle_text(g_streams, s); }
unsigned long long amuse_stub_image_of(const void* p) { return image_of(p); }
static const char* kind_text(hipMemcpyKind k) {
    return k == hipMemcpyHostToDevice ? "h2d" : k == hipMemcpyDeviceToHost ? "d2h" : k == hipMemcpyDeviceToDevice ? "d2d" : k == hipMemcpyHostToHost ? "h2h" : "default";
}
static void log_copy(const char* name, void* d, const void* s, size_t n, hipMemcpyKind k) { Line(name).kv("kind", kind_text(k)).u("bytes", n).p("dst", d).p("src", s); }

// ---- failure injection: the n-th runtime call / launch after amuse_stub_fail_at(n) fails (n = 0: none); amuse_stub_steps() = how many there have been since
static long g_fail_at = 0, g_steps = 0;
static hipError_t g_last_error = hipSuccess;
void amuse_stub_fail_at(long n) { g_fail_at = n; g_steps = 0; }
long amuse_stub_steps() { return g_steps; }
static std::vector<std::string>* g_capture_lines = nullptr;
void amuse_stub_capture(std::vector<std::string>* lines) { g_capture_lines = lines; }
void amuse_stub_emit(const std::string& line) {
    puts(line.c_str());
    if (g_capture_lines) g_capture_lines->push_back(line);
}
static bool step_fails() {
    if (++g_steps != g_fail_at) return false;
    amuse_stub_emit("-- injected failure");
    return true;
}
// ---- kernels by host handle (filled during static initialisation, hence created on first use) and the driver's parameter letters
static std::map<const void*, std::string>& kernels() {
    static std::map<const void*, std::string>* m = new std::map<const void*, std::string>;
    return *m;
}
static const char* (*g_params)(const char*) = nullptr;
void amuse_stub_kernel_params(const char* (*lookup)(const char* mangled)) { g_params = lookup; }
static std::string kernel_text(const void* f) {
    const auto it = kernels().find(f);
    return it == kernels().end() ? "?" : it->second;
}
struct CallConfig { dim3 grid, block; size_t lds; hipStream_t stream; };
static thread_local CallConfig g_config;

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    if (step_fails()) { *p = nullptr; if (g_level == 2) Line("hipMalloc").u("bytes", n).kv("ptr", "failed"); return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    ++g_live;
    if (*p) g_blocks[static_cast<const char*>(*p)] = {n, ++g_nblocks};
    if (g_level == 2) Line("hipMalloc").u("bytes", n).p("ptr", *p);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    if (p) {
        g_image.erase(p);
        if (g_level == 2) Line("hipFree").p("ptr", p);
        g_blocks.erase(static_cast<const char*>(p));
        free(p);
        --g_live;
    }
    return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) {
    if (g_level == 2) log_copy("hipMemcpy", d, s, n, k);
    if (g_level && k == hipMemcpyHostToDevice) log_upload(d, s, n);
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st) {
    if (g_level == 2) { Line l("hipMemcpyAsync"); l.kv("kind", kind_text(k)).u("bytes", n).p("dst", d).p("src", s).st(st); }
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) {
    if (g_level == 2) Line("hipMemset").i("value", v).u("bytes", n).p("dst", d);
    if (step_fails()) return hipErrorUnknown;
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
    if (g_level == 2) Line("hipMemsetAsync").i("value", v).u("bytes", n).p("dst", d).st(st);
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetLastError(void) { const hipError_t e = g_last_error; g_last_error = hipSuccess; return e; }
hipError_t hipDeviceSynchronize(void) {
    if (g_raw) Line("hipDeviceSynchronize");
    return step_fails() ? hipErrorUnknown : hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute attr, int value) {
    if (g_raw) Line("hipFuncSetAttribute").kv("kernel", kernel_text(f)).i("attr", (int)attr).i("value", value);
    return step_fails() ? hipErrorUnknown : hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    if (step_fails()) { if (g_raw) Line("hipStreamCreateWithFlags").u("flags", flags).kv("stream", "failed"); return hipErrorUnknown; }
    *s = reinterpret_cast<hipStream_t>(malloc(8)); ++g_live; g_streams[*s] = ++g_nstreams;
    if (g_raw) Line("hipStreamCreateWithFlags").u("flags", flags).st(*s);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { g_streams.erase(s); free(s); --g_live; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    if (g_level == 2) Line("hipStreamWaitEvent").kv("event", handle_text(g_events, e)).st(s);
    return step_fails() ? hipErrorUnknown : hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    if (step_fails()) { if (g_raw) Line("hipEventCreateWithFlags").u("flags", flags).kv("event", "failed"); return hipErrorUnknown; }
    *e = reinterpret_cast<hipEvent_t>(malloc(8)); ++g_live; g_events[*e] = ++g_nevents;
    if (g_raw) Line("hipEventCreateWithFlags").u("flags", flags).kv("event", handle_text(g_events, *e));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { g_events.erase(e); free(e); --g_live; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (g_level == 2) Line("hipEventRecord").kv("event", handle_text(g_events, e)).st(s);
    return step_fails() ? hipErrorUnknown : hipSuccess;
}
// ---- the raw launch level: what the compiler's host code of a kernel and of a <<< >>> calls
void** __hipRegisterFatBinary(const void*) { static void* module = nullptr; return &module; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, uint3*, uint3*, dim3*, dim3*, int*) { kernels()[host] = name; }
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) { g_config = {grid, block, lds, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* st) {
    *grid = g_config.grid; *block = g_config.block; *lds = g_config.lds; *st = g_config.stream;
    return hipSuccess;
}
// arguments by the driver's letters, one per parameter: p pointer, i int, l long, u uint32, U uint64, z size_t, f float, d double, S a struct by value (skipped)
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t st) {
    const std::string name = kernel_text(f);
    if (g_raw) {
        Line l("launch");
        char buf[96];
        snprintf(buf, sizeof(buf), "%u,%u,%u", grid.x, grid.y, grid.z);
        l.kv("kernel", name).kv("grid", buf);
        snprintf(buf, sizeof(buf), "%u,%u,%u", block.x, block.y, block.z);
        l.kv("block", buf).u("lds", lds).st(st);
        const char* sig = g_params ? g_params(name.c_str()) : nullptr;
        if (!sig) l.kv("args", "unknown");
        for (int i = 0; sig && sig[i]; ++i) {
            const std::string k = "a" + std::to_string(i);
            const void* a = args[i];
            switch (sig[i]) {
                case 'p': l.p(k.c_str(), *static_cast<void* const*>(a)); break;
                case 'i': l.i(k.c_str(), *static_cast<const int*>(a)); break;
                case 'l': l.i(k.c_str(), *static_cast<const long*>(a)); break;
                case 'u': l.u(k.c_str(), *static_cast<const uint32_t*>(a)); break;
                case 'U': l.u(k.c_str(), *static_cast<const uint64_t*>(a)); break;
                case 'z': l.u(k.c_str(), *static_cast<const size_t*>(a)); break;
                case 'f': l.f(k.c_str(), *static_cast<const float*>(a)); break;
                case 'd': { char b[48]; snprintf(b, sizeof(b), "%a", *static_cast<const double*>(a)); l.kv(k.c_str(), b); break; }
                default: l.kv(k.c_str(), "skipped(struct)"); break;
            }
        }
    }
    if (step_fails()) { g_last_error = hipErrorLaunchFailure; return hipErrorLaunchFailure; }
    return hipSuccess;
}
}

namespace amuse {
static hipError_t log_sample(const char* name, const SampleArgs& a, int prec, hipStream_t st) {
    if (g_log) printf("%s prec=%d image=%016llx wave_units=%u a=%u b=%u\n", name, prec, image_of(a.wstream), a.wave_units, a.wave_units_a, a.wave_units_b);
    if (g_level == 2)   // (drop_epoch: the launchers set it themselves)
        Line(name).i("prec", prec).st(st).w(a.wstream).U_(wave_units).U_(wave_units_a).U_(wave_units_b).P_(pvec).P_(time_tok).P_(time_tok_clip).P_(cond_tok).P_(pe0).P_(coef)
            .P_(x_init).P_(step_noise).P_(latents_out).P_(traj_out).P_(eps_out).P_(tap_out).U_(seed).U_(clip0).I_(B).I_(T).I_(S).I_(G).I_(no_update).P_(prof_out).I_(prof_step)
            .U_(drop_thr).f("drop_scale", a.drop_scale).U_(drop_seed);
    return hipSuccess;
}
static void log_drop(Line& l, const VaeDropArgs& a) { l.U_(drop_thr).f("drop_scale", a.drop_scale).U_(drop_seed).U_(drop_clip0); }
static hipError_t log_rows(const char* name, const VaeRowsArgs& a, int prec, int mode, hipStream_t st) {
    if (g_log)
        printf("%s prec=%d mode=%d stage=%d image=%016llx stage_base=%016llx stage_units=%016llx\n", name, prec, mode, a.stage, image_of(a.wstream),
               (unsigned long long)fnv1a(a.stage_base, sizeof(a.stage_base)), (unsigned long long)fnv1a(a.stage_units, sizeof(a.stage_units)));
    if (g_level == 2) {
        Line l(name);
        l.i("prec", prec).i("mode", mode).st(st).w(a.wstream).x("stage_base", fnv1a(a.stage_base, sizeof(a.stage_base))).x("stage_units", fnv1a(a.stage_units, sizeof(a.stage_units)))
            .P_(pvec).P_(final_bias).P_(pe).P_(ca).P_(lengths).P_(x).P_(q).P_(k).P_(v).P_(attn_o).P_(skip).P_(feats_out).P_(poses_out).P_(trans_out).I_(B).I_(stage).I_(quat_mode)
            .I_(tiles).P_(c1).P_(c1_out).P_(enc_feats).P_(tok).P_(emb_bias).P_(stats_out).I_(S).I_(npre).P_(pre_tok_t).U_(pre_tok_t_stride).P_(pre_tok_c)
            .p("mem.tkv", a.mem.tkv).u("mem.tkv_clip_stride", a.mem.tkv_clip_stride).p("mem.ckv", a.mem.ckv).i("mem.ncond", a.mem.ncond)
            .P_(coef).P_(x_out).P_(step_noise).U_(seed).U_(clip0).I_(step);
        if (mode == VAE_MODE_DEC_DROP) {   // the argument is a VaeRowsDropArgs handed over by its base
            const VaeRowsDropArgs& d = static_cast<const VaeRowsDropArgs&>(a);
            log_drop(l, d.drop);
            l.p("ca_bias", d.ca_bias);
        }
    }
    return hipSuccess;
}
static hipError_t log_stream(const char* name, const void* wstream) {
    if (g_log) printf("%s image=%016llx\n", name, image_of(wstream));
    return hipSuccess;
}
static hipError_t log_vae_fused(const char* name, const VaeFusedArgs& a, hipStream_t st) {
    if (g_level == 2)
        Line(name).st(st).w(a.wstream).P_(pvec).P_(final_bias).P_(pe).P_(ca).P_(lengths).P_(skip).P_(feats_out).P_(poses_out).P_(trans_out).P_(tap_out).P_(c1).I_(B).I_(quat_mode)
            .I_(ablate_attention);
    return log_stream(name, a.wstream);
}
static hipError_t log_den_fused(const char* name, const DenFusedArgs& a, hipStream_t st) {
    if (g_level == 2)
        Line(name).st(st).w(a.wstream).P_(pvec).P_(final_bias).P_(emb_bias).P_(pe).P_(ttok).U_(ttok_stride).P_(ctok).P_(skip).P_(x).P_(eps_out).P_(coef).P_(step_noise).P_(lengths)
            .U_(seed).U_(clip0).I_(step).I_(B).I_(npre).I_(ablate_attention);
    return log_stream(name, a.wstream);
}
hipError_t launch_sample(const SampleArgs& a, int prec, hipStream_t st) { return log_sample("launch_sample", a, prec, st); }
hipError_t launch_sample8(const SampleArgs& a, hipStream_t st) { return log_sample("launch_sample8", a, -1, st); }
hipError_t launch_sample8x(const SampleArgs& a, hipStream_t st) { return log_sample("launch_sample8x", a, -1, st); }
hipError_t launch_sample8h(const SampleArgs& a, hipStream_t st) { return log_sample("launch_sample8h", a, -1, st); }
hipError_t launch_time_tokens(const int* ts, int T, const float* freqs, const float* w1t, const float* b1, const float* w2t, const float* b2, const float* pe1, float* out, hipStream_t st) {
    if (g_level == 2) Line("launch_time_tokens").st(st).p("timesteps", ts).i("T", T).p("freqs", freqs).p("w1t", w1t).p("b1", b1).p("w2t", w2t).p("b2", b2).p("pe1", pe1).p("out", out);
    return hipSuccess;
}
hipError_t launch_cond_tokens(const CondArgs& a, hipStream_t st) {
    if (g_level == 2)
        Line("launch_cond_tokens").st(st).p("z0", a.z[0]).p("z1", a.z[1]).p("z2", a.z[2]).p("wt0", a.wt[0]).p("wt1", a.wt[1]).p("wt2", a.wt[2]).p("bias0", a.bias[0])
            .p("bias1", a.bias[1]).p("bias2", a.bias[2]).P_(pe).P_(out).I_(B).I_(ncond).I_(pe_base);
    return hipSuccess;
}
hipError_t launch_repack(const float* params, const int* map, void* dst, size_t n, int kind, hipStream_t st) {   // (the gather map is host memory here)
    if (g_log) printf("launch_repack n=%zu kind=%d image=%016llx map=%016llx\n", n, kind, image_of(dst), (unsigned long long)fnv1a(map, n * sizeof(int)));
    if (g_level == 2) Line("launch_repack").st(st).p("params", params).x("map", fnv1a(map, n * sizeof(int))).p("dst", dst).x("image", image_of(dst)).u("n", n).i("kind", kind);
    return hipSuccess;
}
hipError_t launch_add_noise(const float* z0, const float* noise, const float* sa, const float* sb, float* out, int B, hipStream_t st, int nfeat) {
    if (g_level == 2) Line("launch_add_noise").st(st).p("z0", z0).p("noise", noise).p("sa", sa).p("sb", sb).p("out", out).i("B", B).i("nfeat", nfeat);
    return hipSuccess;
}
hipError_t launch_counter_normal(uint64_t seed, uint64_t clip0, int B, int step, int rng_stream, float* out, hipStream_t st, int nfeat) {
    if (g_level == 2) Line("launch_counter_normal").st(st).u("seed", seed).u("clip0", clip0).i("B", B).i("step", step).i("rng_stream", rng_stream).p("out", out).i("nfeat", nfeat);
    return hipSuccess;
}
hipError_t launch_vae_rows(const VaeRowsArgs& a, int prec, int mode, hipStream_t st) { return log_rows("launch_vae_rows", a, prec, mode, st); }
hipError_t launch_vae_rows8x(const VaeRowsArgs& a, hipStream_t st, int mode) { return log_rows("launch_vae_rows8x", a, -1, mode, st); }
hipError_t launch_vae_attn(const VaeAttnArgs& a, int prec, int mode, hipStream_t st) {
    if (g_level == 2) {
        Line l("launch_vae_attn");
        l.i("prec", prec).i("mode", mode).st(st).P_(q).P_(k).P_(v).P_(lengths).P_(o).I_(B).I_(q_tiles).I_(S);
        if (mode == VAE_MODE_DEC_DROP) {   // the argument is a VaeAttnDropArgs handed over by its base
            const VaeAttnDropArgs& d = static_cast<const VaeAttnDropArgs&>(a);
            l.i("layer", d.layer);
            log_drop(l, d.drop);
        }
    }
    return hipSuccess;
}
hipError_t launch_vae_fused(const VaeFusedArgs& a, hipStream_t st) { return log_vae_fused("launch_vae_fused", a, st); }
hipError_t launch_vae_fusedh(const VaeFusedArgs& a, hipStream_t st) { return log_vae_fused("launch_vae_fusedh", a, st); }
hipError_t launch_den_fused(const DenFusedArgs& a, hipStream_t st) { return log_den_fused("launch_den_fused", a, st); }
hipError_t launch_den_fusedh(const DenFusedArgs& a, hipStream_t st) { return log_den_fused("launch_den_fusedh", a, st); }
hipError_t launch_vae_fusedx(const VaeFusedXArgs& a, hipStream_t st) {
    if (g_level == 2)
        Line("launch_vae_fusedx").st(st).w(a.wstream).P_(pvec).P_(final_bias).P_(pe).P_(ca).P_(lengths).P_(skip).P_(obuf).P_(feats_out).P_(poses_out).P_(trans_out).P_(tap_out)
            .P_(c1).P_(c1_out).I_(B).I_(quat_mode);
    return log_stream("launch_vae_fusedx", a.wstream);
}
hipError_t launch_den_fusedx(const DenFusedXArgs& a, hipStream_t st) {
    if (g_level == 2)
        Line("launch_den_fusedx").st(st).w(a.wstream).P_(pvec).P_(emb_bias).P_(final_bias).P_(pe).P_(ttok).U_(ttok_stride).P_(ctok).P_(x_in).P_(x_out).P_(eps_out).P_(coef)
            .P_(step_noise).P_(lengths).P_(obuf).P_(skip).U_(seed).U_(clip0).I_(step).I_(B).I_(S).I_(npre).I_(encode);
    return log_stream("launch_den_fusedx", a.wstream);
}
hipError_t launch_sample_dec(const SampleDecArgs& a, int prec, hipStream_t st) {
    if (g_log) printf("launch_sample_dec prec=%d image=%016llx wave_units=%u\n", prec, image_of(a.wstream), a.wave_units);
    if (g_level == 2)
        Line("launch_sample_dec").i("prec", prec).st(st).w(a.wstream).U_(wave_units).P_(pvec).P_(pe0).p("mem.tkv", a.mem.tkv).u("mem.tkv_clip_stride", a.mem.tkv_clip_stride)
            .p("mem.ckv", a.mem.ckv).i("mem.ncond", a.mem.ncond).U_(tkv_step_stride).P_(coef).P_(x_init).P_(step_noise).P_(latents_out).P_(traj_out).P_(eps_out).P_(tap_out)
            .U_(seed).U_(clip0).I_(B).I_(T).I_(no_update);
    return hipSuccess;
}
hipError_t launch_mem_kv(const float* tok, int N, const float* wkv_t, const float* bkv, float* kv, hipStream_t st) {
    if (g_level == 2) Line("launch_mem_kv").st(st).p("tok", tok).i("N", N).p("wkv_t", wkv_t).p("bkv", bkv).p("kv", kv);
    return hipSuccess;
}
hipError_t launch_feats_to_smplx(const float* feats, size_t nrows, int quat_mode, float* poses, float* trans, hipStream_t st) {
    if (g_level == 2) Line("launch_feats_to_smplx").st(st).p("feats", feats).u("nrows", nrows).i("quat_mode", quat_mode).p("poses", poses).p("trans", trans);
    return hipSuccess;
}
hipError_t launch_smplx_to_feats(const float* poses, const float* trans, size_t nrows, float* feats, hipStream_t st) {
    if (g_level == 2) Line("launch_smplx_to_feats").st(st).p("poses", poses).p("trans", trans).u("nrows", nrows).p("feats", feats);
    return hipSuccess;
}
hipError_t launch_vae_latent(const float* stats, const float* eps, float* mu, float* std, float* latent, int B, hipStream_t st) {
    if (g_level == 2) Line("launch_vae_latent").st(st).p("stats", stats).p("eps", eps).p("mu", mu).p("std", std).p("latent", latent).i("B", B);
    return hipSuccess;
}
hipError_t launch_vae_ca(const float* z, const float* wv_t, const float* bv, const float* wo_t, const float* bo, float* ca, int B, hipStream_t st) {
    if (g_level == 2) Line("launch_vae_ca").st(st).p("z", z).p("wv_t", wv_t).p("bv", bv).p("wo_t", wo_t).p("bo", bo).p("ca", ca).i("B", B);
    return hipSuccess;
}
// ---- the audio front-end's launchers (amuse_audio.hpp): launch log only.  Weight pointers (GemmArgs::W, the head's W) also print the digest of their image
hipError_t launch_gemm(const GemmArgs& a, int epi, hipStream_t st) {
    if (g_level == 2) Line("launch_gemm").i("epi", epi).st(st).P_(A).wp("W", a.W).P_(bias).I_(M).I_(N).I_(K).P_(out_bf16).P_(out_f32).P_(pos).P_(vt);
    return hipSuccess;
}
hipError_t launch_fbank(const float* wave, int n_samples, int B, const float* window, const float* melw_t, const int* mel_range, float mean, float std, float* out, hipStream_t st) {
    if (g_level == 2)
        Line("launch_fbank").st(st).p("wave", wave).i("n_samples", n_samples).i("B", B).p("window", window).p("melw_t", melw_t).p("mel_range", mel_range).f("mean", mean).f("std", std).p("out", out);
    return hipSuccess;
}
hipError_t launch_im2col(const float* fbank, unsigned short* patches, int B, hipStream_t st) {
    if (g_level == 2) Line("launch_im2col").st(st).p("fbank", fbank).p("patches", patches).i("B", B);
    return hipSuccess;
}
hipError_t launch_ast_tokens(const float* cls, const float* dist, const float* pos, float* X, int B, hipStream_t st) {
    if (g_level == 2) Line("launch_ast_tokens").st(st).p("cls", cls).p("dist", dist).p("pos", pos).p("X", X).i("B", B);
    return hipSuccess;
}
hipError_t launch_ln_bf16(const float* X, const float* gamma, const float* beta, float eps, unsigned short* out, int M, hipStream_t st) {
    if (g_level == 2) Line("launch_ln_bf16").st(st).p("X", X).p("gamma", gamma).p("beta", beta).f("eps", eps).p("out", out).i("M", M);
    return hipSuccess;
}
hipError_t launch_tile_bf16(const unsigned short* src, unsigned short* dst, int M, int F, hipStream_t st) {
    if (g_level == 2) Line("launch_tile_bf16").st(st).p("src", src).p("dst", dst).i("M", M).i("F", F);
    return hipSuccess;
}
hipError_t launch_untile_bf16(const unsigned short* src, unsigned short* dst, int M, int F, hipStream_t st) {
    if (g_level == 2) Line("launch_untile_bf16").st(st).p("src", src).p("dst", dst).i("M", M).i("F", F);
    return hipSuccess;
}
hipError_t launch_untile_f32(const float* src, float* dst, int M, int F, int rows_in, int rows_out, hipStream_t st) {
    if (g_level == 2) Line("launch_untile_f32").st(st).p("src", src).p("dst", dst).i("M", M).i("F", F).i("rows_in", rows_in).i("rows_out", rows_out);
    return hipSuccess;
}
hipError_t launch_ast_attn(const unsigned short* QK, const unsigned short* Vt, unsigned short* O, int B, hipStream_t st) {
    if (g_level == 2) Line("launch_ast_attn").st(st).p("QK", QK).p("Vt", Vt).p("O", O).i("B", B);
    return hipSuccess;
}
hipError_t launch_ast_pool(const float* X, const float* gamma, const float* beta, int frame_based, float* pooled, int B, hipStream_t st) {
    if (g_level == 2) Line("launch_ast_pool").st(st).p("X", X).p("gamma", gamma).p("beta", beta).i("frame_based", frame_based).p("pooled", pooled).i("B", B);
    return hipSuccess;
}
hipError_t launch_ast_head(const float* pooled, int frame_based, const float* gamma, const float* beta, const unsigned short* W, const float* bias, float* out, int B, hipStream_t st) {
    if (g_level == 2)
        Line("launch_ast_head").st(st).p("pooled", pooled).i("frame_based", frame_based).p("gamma", gamma).p("beta", beta).wp("W", W).p("bias", bias).p("out", out).i("B", B);
    return hipSuccess;
}
}  // namespace amuse
// a second stream for drivers that do not include the HIP headers (tests/host_asan/launch_args.cpp)
void* amuse_stub_stream_create() { hipStream_t s = nullptr; (void)hipStreamCreateWithFlags(&s, 0); return s; }
void amuse_stub_stream_destroy(void* s) { (void)hipStreamDestroy(static_cast<hipStream_t>(s)); }
