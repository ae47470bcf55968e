// Host-side pieces shared by the library's translation units: the error slot, the launch plan, the context struct and the upload helper that classifies
// every packed image.  (State-dict index and weight packers: amuse_pack.hpp, which only amuse_api.hip and amuse_variants.hip include.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_dev.hpp"
#include "amuse_kernels.hpp"

// error slot of the C ABI (thread-local text behind amuse_last_error; defined in amuse_api.hip)
__attribute__((visibility("hidden"), format(printf, 2, 3))) int amuse_failf(int code, const char* fmt, ...);
#define fail(...) amuse_failf(__VA_ARGS__)

namespace amuse {
// amuse_update_weights_device learns the packed images' gather maps by running the builders on probe parameters with upload()
// redirected into host memory, keyed by the context slot the image belongs to; kind and class are what the builder passed to upload()
struct Capture {
    struct Image { std::vector<unsigned char> bytes; int kind, cls; };
    std::map<void**, Image> bufs;
};
__attribute__((visibility("hidden"))) inline thread_local Capture* g_capture = nullptr;
__attribute__((visibility("hidden"))) inline bool g_probe_f16 = false;   // build_repack_maps: the lo units carry the probe value too (amuse_update_weights_device)
}  // namespace amuse

using namespace amuse;

namespace {
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(AMUSE_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

}  // namespace

struct amuse_variant;   // the Denoiser variants' streams and tables (amuse_variants.hip)
// ---- The launch plan: ONE statement of which kernels a job takes (exported as amuse_plan, include/amuse_hip.h; amuse_amd/shard.py and
// tests/c_client call that - nothing restates these rules).  Every choice is keyed by the clip count of the CALL / the JOB, never of a chunk or a shard.
constexpr int kFusedMinClips = 64;   // the per-clip 16-bit kernels occupy one CU per clip: they win once the clips fill a good part of the chip (profiles/r03_decode_perf.txt:
                                     // fused 0.61 ms for any B <= 128; staged 0.51 ms at 32 clips, 0.66 ms at 64, 1.07 ms at 128)
// Do the clips fill rounds of the chip's 256 CUs well enough for the fp32x per-clip kernels (k_vae_fusedx.hip)?  A clip takes ~1.5 ms on its CU whatever the batch: from 160
// clips in the first round, in round r >= 2 with at least 164 - 50 (r - 2) clips in it (profiles/r05_fusedx_decode.txt, ms at 160 / 256 / 384 / 512 / 768 / 1024 clips:
// 1.49 1.65 3.05 3.18 4.76 6.32 against 1.67 1.86 2.84 3.88 5.81 7.75 on the row / attention launches)
inline bool fills_rounds(int B) {
    if (B < 160) return false;
    const int r = (B + 255) / 256, in_last = B - 256 * (r - 1);
    return r == 1 || in_last >= 164 - 50 * (r - 2);
}
// clips per 16-row tile of the latent trans_enc sampler (k_sampler*.hip); the other Denoiser variants have no such choice (1).  One clip per tile up to 128 clips, then fatter
// tiles: a step costs the same for 1..16/tokens clips per tile, and 128 busy CUs run it 6-7 % faster than 256 - with every CU re-streaming the whole network each step the
// 256-workgroup launch sits at the L2's delivery limit (profiles/r01_batch_sweep.txt: 256 clips 36.0 ms with one clip per tile, 33.6 ms with two or three).
inline int plan_clips_per_group(int arch, int B, int tokens) {
    if (arch != AMUSE_ARCH_ENC) return 1;
    const int gmax = 16 / tokens;
    int g = (B + 127) / 128;
    if (g > gmax) g = gmax;
    return g < 1 ? 1 : g;
}
// MotionPrior.decode: fp32 has one kernel family (STAGED); bf16 / fp16: the fused per-clip kernel (k_vae_fused.hip) from kFusedMinClips; fp32x: the per-clip kernel
// (k_vae_fusedx.hip, CLIP) where the clips fill rounds, else the no-split-K row kernel (k_vae_rows8.hip, FUSED) from kFusedMinClips, else the split-K row kernel (STAGED)
inline int plan_decode_path(int precision, int B) {
    if (precision == AMUSE_PREC_F32) return AMUSE_DECODE_STAGED;
    if (precision == AMUSE_PREC_F32X && fills_rounds(B)) return AMUSE_DECODE_CLIP;
    return B >= kFusedMinClips ? AMUSE_DECODE_FUSED : AMUSE_DECODE_STAGED;
}
// MotionPrior.encode: only the fp32x mode has more than the staged kernels (the decode's rule)
inline int plan_encode_path(int precision, int B) { return precision == AMUSE_PREC_F32X ? plan_decode_path(precision, B) : AMUSE_DECODE_STAGED; }
// one Denoiser step of the pose-space trans_enc variant (S = 304 rows per clip): the decode's rule on k_den_fused / k_vae_rows8x<ENC> / k_den_fusedx; the other variants: STAGED
inline int plan_step_path(int arch, int precision, int B) { return arch == AMUSE_ARCH_ENC_POSE ? plan_decode_path(precision, B) : AMUSE_DECODE_STAGED; }
// a pin (amuse_set_decode_path) against what the precision has: FUSED = the fused kernel of the 16-bit modes / the row kernel without split-K of fp32x; CLIP = fp32x's
// per-clip kernel, FUSED in the modes that have no third kernel; fp32 has one family
inline int resolve_path(int pin, int planned, int precision) {
    if (pin == AMUSE_DECODE_AUTO) return planned;
    if (precision == AMUSE_PREC_F32 || pin == AMUSE_DECODE_STAGED) return AMUSE_DECODE_STAGED;
    return (pin == AMUSE_DECODE_CLIP && precision == AMUSE_PREC_F32X) ? AMUSE_DECODE_CLIP : AMUSE_DECODE_FUSED;
}

struct amuse_ctx {
    int device = 0;
    int arch = AMUSE_ARCH_ENC;         // Denoiser variant (amuse_create_arch); anything but AMUSE_ARCH_ENC runs through `var`
    amuse_variant* var = nullptr;
    bool has_prior = true;             // pose-space variants may be created without MotionPrior weights
    int clips_per_group = 0;
    int decode_path = AMUSE_DECODE_AUTO;
    int last_plan[4] = {0, 0, 0, 0};   // amuse_debug_last_plan: clips per tile / decode / encode / step path the last call of each kind actually took
    float* decode_tap = nullptr;       // amuse_debug_set_decode_tap
    int ablate = 0;                    // amuse_debug_set_ablation
    // train-mode sampling (amuse_set_sample_dropout): drop_thr = p 2^24, 0 = eval
    uint32_t drop_thr = 0;
    float drop_scale = 1.f;
    uint64_t drop_seed = 0;
    // train-mode decode (amuse_set_decode_dropout): dec_drop_thr = p 2^24, 0 = eval; dec_drop_clip0 = global index of clip 0 of an amuse_vae_decode call
    uint32_t dec_drop_thr = 0;
    float dec_drop_scale = 1.f;
    uint64_t dec_drop_seed = 0, dec_drop_clip0 = 0;
    // denoiser
    uint4* den_w = nullptr;            // fp32 streams of the 4-wave kernel (k_sampler.hip: the fp32 parity mode)
    uint32_t den_wave_units = 0;
    uint4* den_w8 = nullptr;           // bf16 streams of the 8-wave kernel (k_sampler8.hip)
    uint32_t den_w8_units[2] = {0, 0}; // per-step units of a group-A / group-B wave
    uint4* den_w8h = nullptr;          // fp16 streams of the same kernel built for fp16 operands (k_sampler8h.hip, AMUSE_PREC_F16)
    uint4* den_w8x = nullptr;          // split-fp16 streams of the 8-wave fp32x kernel (k_sampler8x.hip)
    uint32_t den_w8x_units[2] = {0, 0};
    float* den_pvec = nullptr;
    float* den_pe = nullptr;           // [500][128]
    float* den_freqs = nullptr;        // [128]
    float *te_w1t = nullptr, *te_b1 = nullptr, *te_w2t = nullptr, *te_b2 = nullptr;
    float* cond_wt[3] = {nullptr, nullptr, nullptr};
    float* cond_b[3] = {nullptr, nullptr, nullptr};
    // prior decoder
    uint4* vae_w[4] = {nullptr, nullptr, nullptr, nullptr};   // staged decode streams: fp32 | bf16 | split-fp16 (fp32x) | fp16
    uint32_t vae_stage_base[4][kVaeStages];
    uint32_t vae_stage_units[4][kVaeStages];
    uint4* vae_wf = nullptr;           // bf16 stream of the fused decode kernel (k_vae_fused.hip)
    uint4* vae_wfh = nullptr;          // its fp16 twin (k_vae_fusedh.hip, AMUSE_PREC_F16)
    float* vae_c1[4] = {nullptr, nullptr, nullptr, nullptr};   // block 0's self-attention half of the fused decoder, bf16 | fp16 build: [300][128] (+ the tap scratch behind it); [2]: of the fp32x row stages
    bool vae_c1_valid[4] = {false, false, false, false};   // (re)computed by the next fused decode after a weight change
    hipEvent_t vae_c1_ev[4] = {nullptr, nullptr, nullptr, nullptr};     // recorded behind the launches that produced vae_c1[i] ...
    hipStream_t vae_c1_stream[4] = {nullptr, nullptr, nullptr, nullptr}; // ... on this stream: a decode on ANOTHER stream waits on the event first
    uint4* vae_w8x = nullptr;          // fp32x row stages without split-K (k_vae_rows8.hip): one stream per stage, consumption order
    uint32_t vae_w8x_base[kVaeStages];
    uint4* vaee_wfx = nullptr;         // fp32x encoder as one per-clip kernel (k_vae_fusedx.hip k_den_fusedx<encode>): one stream for the whole network
    uint4* vae_wfx = nullptr;          // fp32x fused decoder (k_vae_fusedx.hip): one stream of unit pairs for the whole network, consumption order
    uint4* vaee_w8x = nullptr;         // the same for MotionPrior.encode's stages 1..9 (AMUSE_UPD_ENCODER | AMUSE_UPD_F32X)
    uint32_t vaee_w8x_base[kVaeStages];
    uint4* vae_skip = nullptr; size_t vae_skip_cap = 0;   // clips
    float* vae_ca_ws = nullptr; size_t vae_ca_cap = 0;    // clips
    float *vae_pvec = nullptr, *vae_final_bias = nullptr, *vae_pe = nullptr;
    float *vae_wv_t = nullptr, *vae_bv = nullptr, *vae_wo_t = nullptr, *vae_bo = nullptr;
    // prior encoder (MotionPrior.encode)
    uint4* vaee_w[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t vaee_stage_base[4][kVaeStages];
    uint32_t vaee_stage_units[4][kVaeStages];
    float *vaee_pvec = nullptr, *vaee_pe = nullptr, *vaee_tok = nullptr, *vaee_emb_bias = nullptr;
    // schedule
    int T = 0;
    int* d_timesteps = nullptr;
    float *d_coef = nullptr, *d_time_tok = nullptr;
    int* d_ts1 = nullptr;
    float *d_tt1 = nullptr, *d_coef1 = nullptr;
    // workspaces
    float* cond_tok = nullptr; size_t cond_cap = 0;
    float* lat_tmp = nullptr; size_t lat_cap = 0;
    float* fwd_ws = nullptr; size_t fwd_cap = 0;
    float* vae_ws = nullptr; size_t vae_cap = 0;  // clips
    int* d_lengths = nullptr; size_t len_cap = 0;
    std::vector<void*> owned;          // every allocation upload() made (all weight images, the variants' included) + the re-pack's gather maps: freed by amuse_destroy
    // amuse_update_weights_device: one entry per packed image (built on the first call)
    struct Repack { void** slot; int* map; size_t n; int prior, kind, cls; };
    std::vector<Repack> repack;
};

// AMUSE_UPD_* bit of a precision's streams, per PREC_* index
constexpr int kUpdBit[4] = {AMUSE_UPD_F32, AMUSE_UPD_BF16, AMUSE_UPD_F32X, AMUSE_UPD_F16};
constexpr int kImgConst = -1;   // upload()'s class of an image that is no function of the parameters: never re-packed on the device

namespace {
// Uploads a packed image into its context slot: the first call allocates (the context owns the memory from then on), later calls (amuse_update_weights:
// same architecture, same sizes) overwrite in place.  The image is classified HERE, by the builder that knows what it packed: `kind` = its element type as
// launch_repack takes it (the PREC_* index of the packer: 0 fp32, 1 bf16, 2 split-fp16, 3 fp16), `cls` = the AMUSE_UPD_* bits that must all be requested for
// it to be replaced (0: small parameters, always replaced).  amuse_update_weights_device reads both back through the capture.
template <typename T>
int upload(amuse_ctx* c, T** dst, const void* src, size_t bytes, int kind = PREC_F32, int cls = 0) {
    if (g_capture) {
        const unsigned char* b = static_cast<const unsigned char*>(src);
        if (cls != kImgConst) g_capture->bufs[reinterpret_cast<void**>(dst)] = {{b, b + bytes}, kind, cls};
        return 0;
    }
    if (!*dst) {
        HIP_TRY(hipMalloc((void**)dst, bytes));
        c->owned.push_back(*dst);
    }
    HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int ensure(float** p, size_t* cap, size_t need_floats) {
    if (*cap >= need_floats) return 0;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, need_floats * sizeof(float)));
    *cap = need_floats;
    return 0;
}
}  // namespace
