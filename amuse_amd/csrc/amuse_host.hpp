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
#include "amuse_seq_host.hpp"

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

// The weight images of one skip network - nine skip-connected blocks over [clips][rows][128]: MotionPrior's decoder and encoder, the pose-space trans_enc Denoiser - in
// every layout a kernel consumes (amuse_pack.hpp states the layouts), with the small parameters that belong to the network.  A slot a network has no kernel for stays null.
struct RowNet {
    uint4* staged[4] = {nullptr, nullptr, nullptr, nullptr};   // row-stage streams [stage][wave][units]: fp32 | bf16 | split-fp16 (fp32x) | fp16 (PREC_* index)
    uint32_t stage_base[4][kVaeStages];
    uint32_t stage_units[4][kVaeStages];
    uint4* rows8 = nullptr;            // fp32x row stages without split-K (k_vae_rows8.hip): one stream per stage, consumption order
    uint32_t rows8_base[kVaeStages];
    uint4* fusedx = nullptr;           // fp32x, the whole network as ONE stream of unit pairs for the per-clip kernels (k_vae_fusedx.hip)
    uint4* fused16[2] = {nullptr, nullptr};   // the per-clip 16-bit kernels' stream (k_vae_fused.hip / k_den_fused.hip): bf16 | fp16
    float* pvec = nullptr;             // PV_* layout (the trans_dec Denoisers: PVX_*)
    float* final_bias = nullptr;       // bias of the matrix behind stage 9, zero-padded to [384]
    float* emb_bias = nullptr;         // bias of the matrix in front of stage 0 [128]
    float* pe = nullptr;               // positional table [500][128] (the pose-space Denoiser borrows the context's query_pos table)
};
// Block 0's self-attention half of the decoder does not depend on the latent: one [300][128] constant per weight set and kernel family, produced on the stream of the
// decode that first needed it (amuse_api.hip produce_c1 / consume_c1)
struct HoistedC1 {
    float* buf = nullptr;
    bool valid = false;                // (re)computed by the next decode of its family after a weight change
    hipEvent_t event = nullptr;        // recorded behind the launches that produced buf ...
    hipStream_t stream = nullptr;      // ... on this stream: a decode on ANOTHER stream waits on the event first
};

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
    // MotionPrior: decoder and encoder networks; the decoder's cross-attention (one memory token: the latent) as plain matrices for launch_vae_ca
    RowNet dec, enc;
    float *vae_wv_t = nullptr, *vae_bv = nullptr, *vae_wo_t = nullptr, *vae_bo = nullptr;
    float* vaee_tok = nullptr;         // global_motion_token [2][128]
    HoistedC1 c1_bf16, c1_f16;         // of the fused decoder's bf16 | fp16 build: [300][128] + the tap scratch behind it
    HoistedC1 c1_rows8, c1_clip;       // of the fp32x row stages without split-K | of the fp32x per-clip decoder: [300][128]
    uint4* vae_skip = nullptr; size_t vae_skip_cap = 0;   // clips
    float* vae_ca_ws = nullptr; size_t vae_ca_cap = 0;    // clips
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
// grow-only buffer: `cap` and `need` in the caller's unit (elements, or clips with `elems` = the elements that many clips take)
template <typename T>
int ensure(T** p, size_t* cap, size_t need, size_t elems = 0) {
    if (*cap >= need) return 0;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, (elems ? elems : need) * sizeof(T)));
    *cap = need;
    return 0;
}
}  // namespace
