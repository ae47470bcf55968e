// Prints the launch log of hip_stub.cpp (amuse_stub_log(2): every runtime call and every launch with all its arguments, pointers as offsets into their allocation or into
// a named buffer of this driver) in named sections: tests/test_launch_args_cpu.py compares it, in order, with tests/golden/launch_args.json.  Per arch the calls of
// pack_images.cpp at 2 clips with the optional arguments set, then the clip counts that cross each chunk loop, path choice and hoist of the launch sequences.
// C ABI only; parameters from main.cpp's LCG.  The large buffers are never touched (launches are no-ops): they only give the pointers a name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();
void amuse_stub_log(int on);
void amuse_stub_name(const char* name, const void* p, size_t bytes);
void* amuse_stub_stream_create();
void amuse_stub_stream_destroy(void* s);

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, amuse_last_error()); return 1; } \
    } while (0)

static void fill(std::vector<float>& v, uint32_t seed, float scale) {
    uint32_t s = seed;
    for (float& x : v) { s = s * 1664525u + 1013904223u; x = (((s >> 8) & 0xffff) / 65536.0f - 0.5f) * scale; }
}
static float* named(const char* name, size_t floats) {
    float* p = static_cast<float*>(malloc(floats * sizeof(float)));
    amuse_stub_name(name, p, floats * sizeof(float));
    return p;
}

int main() {
    const int B = 2, T = 2, NB = 600;   // NB: clips the named buffers hold
    const size_t SD = AMUSE_POSE_STATE;
    const int kPrecBits[4] = {AMUSE_UPD_F32, AMUSE_UPD_BF16, AMUSE_UPD_F32X, AMUSE_UPD_F16};
    std::vector<float> pri(AMUSE_PRIOR_PARAMS), coef((size_t)T * 8, 0.5f), sa(NB, 0.9f), sb(NB, 0.1f);
    std::vector<int> ts{1, 0}, tsb(NB), lengths(NB);
    for (int i = 0; i < NB; ++i) { tsb[i] = i % 7; lengths[i] = 300 - (i * 37) % 250; }   // lengths[0] = 300
    fill(pri, 2, 0.2f);
    float *con = named("con", (size_t)NB * 256), *emo = named("emo", (size_t)NB * 256), *sty = named("sty", (size_t)NB * 256), *lat = named("lat", (size_t)NB * 128),
          *lat2 = named("lat2", (size_t)NB * 128), *mu = named("mu", (size_t)NB * 128), *sd = named("std", (size_t)NB * 128), *eps = named("eps", (size_t)NB * 128),
          *feats = named("feats", (size_t)NB * 300 * 333), *poses = named("poses", (size_t)NB * 300 * 165), *trans = named("trans", (size_t)NB * 900),
          *x = named("x", (size_t)NB * SD), *out = named("out", (size_t)NB * SD), *noise = named("noise", (size_t)T * B * SD), *traj = named("traj", (size_t)T * B * SD),
          *tap = named("tap", (size_t)11 * 300 * 128), *dtap = named("dtap", (size_t)11 * 300 * 128);
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(named("stamps", 2 * 4 * 192));
    amuse_stub_name("sa", sa.data(), sa.size() * 4);
    amuse_stub_name("sb", sb.data(), sb.size() * 4);
    amuse_stub_name("tsb", tsb.data(), tsb.size() * 4);
    amuse_stub_name("lengths", lengths.data(), lengths.size() * 4);
    void* s2 = amuse_stub_stream_create();
    amuse_stub_log(2);
    for (int arch : {AMUSE_ARCH_ENC, AMUSE_ARCH_DEC, AMUSE_ARCH_ENC_POSE, AMUSE_ARCH_DEC_POSE}) {
        const bool pose = (arch & 2) != 0, latent = !pose;
        std::vector<float> den(amuse_denoiser_param_count(arch));
        fill(den, 10 + arch, 0.2f);
        const float* pp = pose ? nullptr : pri.data();
        const size_t np = pose ? 0 : pri.size();
        printf("== arch %d create\n", arch);
        amuse_ctx* c = amuse_create_arch(0, arch, den.data(), den.size(), pp, np);
        REQUIRE(c != nullptr);
        printf("== arch %d schedule\n", arch);
        amuse_schedule s{T, ts.data(), coef.data(), nullptr};
        REQUIRE(amuse_set_schedule(c, &s, nullptr) == 0);
        float* state = pose ? out : lat;
        for (int prec = AMUSE_PREC_F32; prec <= AMUSE_PREC_F16; ++prec)
            for (int path : {AMUSE_DECODE_STAGED, AMUSE_DECODE_FUSED, AMUSE_DECODE_CLIP}) {
                printf("== arch %d calls prec=%d path=%d\n", arch, prec, path);
                REQUIRE(amuse_set_decode_path(c, path) == 0);
                REQUIRE(amuse_sample(c, con, emo, nullptr, B, prec, 7, 0, nullptr, nullptr, state, nullptr, nullptr) == 0);
                REQUIRE(amuse_sample(c, con, emo, sty, B, prec, 9, 40, x, noise, state, traj, s2) == 0);
                REQUIRE(amuse_denoise_step(c, x, 5, con, nullptr, nullptr, B, prec, out, latent ? tap : nullptr, nullptr) == 0);
                REQUIRE(amuse_diffusion_forward(c, x, x + B * SD, tsb.data(), sa.data(), sb.data(), con, nullptr, sty, B, prec, out + B * SD, out, nullptr) == 0);
                REQUIRE(amuse_diffusion_backward(c, con, nullptr, nullptr, B, prec, AMUSE_QUAT_P3D, 1, 0, nullptr, nullptr, nullptr, poses, trans, nullptr) == 0);
                REQUIRE(amuse_diffusion_backward(c, con, emo, sty, B, prec, AMUSE_QUAT_LEGACY, 1, 6, x, nullptr, state, poses, trans, s2) == 0);
                if (arch == AMUSE_ARCH_ENC) REQUIRE(amuse_profile_sample(c, con, nullptr, nullptr, B, prec, 1, stamps, nullptr) == 0);
                if (pose) {
                    REQUIRE(amuse_denoise_step_pose(c, x, 5, con, nullptr, nullptr, nullptr, B, prec, out, nullptr) == 0);
                    REQUIRE(amuse_denoise_step_pose(c, x, 5, con, emo, nullptr, lengths.data(), B, prec, out, s2) == 0);
                    continue;
                }
                REQUIRE(amuse_vae_decode(c, lat, nullptr, B, prec, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
                REQUIRE(amuse_vae_decode(c, lat, lengths.data(), B, prec, AMUSE_QUAT_LEGACY, nullptr, poses, nullptr, nullptr) == 0);
                REQUIRE(amuse_debug_set_decode_tap(c, dtap) == 0);
                REQUIRE(amuse_vae_decode(c, lat, nullptr, B, prec, AMUSE_QUAT_P3D, feats, nullptr, nullptr, nullptr) == 0);
                REQUIRE(amuse_debug_set_decode_tap(c, nullptr) == 0);
                REQUIRE(amuse_vae_encode(c, feats, nullptr, B, prec, nullptr, lat2, nullptr, nullptr, nullptr) == 0);
                REQUIRE(amuse_vae_encode(c, feats, lengths.data(), B, prec, eps, mu, sd, lat2, nullptr) == 0);
                if (prec != AMUSE_PREC_F32X && path == AMUSE_DECODE_STAGED) {   // train-mode decode
                    REQUIRE(amuse_set_decode_dropout(c, 0.1f, 3, 0) == 0);
                    REQUIRE(amuse_vae_decode(c, lat, nullptr, B, prec, AMUSE_QUAT_P3D, feats, nullptr, nullptr, nullptr) == 0);
                    REQUIRE(amuse_set_decode_dropout(c, 0.f, 0, 0) == 0);
                }
            }
        REQUIRE(amuse_set_decode_path(c, AMUSE_DECODE_AUTO) == 0);
        if (latent) {
            // the chunk loops of the staged kernels (512 clips per chunk), lengths given
            printf("== arch %d staged decode encode 513\n", arch);
            REQUIRE(amuse_set_decode_path(c, AMUSE_DECODE_STAGED) == 0);
            REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 513, AMUSE_PREC_F32, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_encode(c, feats, lengths.data(), 513, AMUSE_PREC_F32, eps, mu, sd, lat2, nullptr) == 0);
            REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 513, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, nullptr, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_encode(c, feats, lengths.data(), 513, AMUSE_PREC_F32X, nullptr, mu, nullptr, nullptr, nullptr) == 0);
            REQUIRE(amuse_set_decode_path(c, AMUSE_DECODE_AUTO) == 0);
            printf("== arch %d fp32x 513 unpinned\n", arch);   // rows8 in two chunks, the hoist; encode's stages 1..9 on rows8
            REQUIRE(amuse_vae_decode(c, lat, nullptr, 513, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_encode(c, feats, nullptr, 513, AMUSE_PREC_F32X, nullptr, mu, nullptr, nullptr, nullptr) == 0);
            printf("== arch %d fp32x decode 160 twice\n", arch);   // the per-clip kernel with its hoist
            for (int i = 0; i < 2; ++i) REQUIRE(amuse_vae_decode(c, lat, nullptr, 160, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 160, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_encode(c, feats, lengths.data(), 160, AMUSE_PREC_F32X, eps, mu, sd, lat2, nullptr) == 0);
            REQUIRE(amuse_vae_encode(c, feats, nullptr, 600, AMUSE_PREC_F32X, nullptr, nullptr, nullptr, lat2, nullptr) == 0);   // per-clip encode in two chunks
            for (int prec : {AMUSE_PREC_BF16, AMUSE_PREC_F16}) {
                printf("== arch %d decode 64 prec=%d hoist\n", arch, prec);
                for (int i = 0; i < 2; ++i) REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, prec, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
                REQUIRE(amuse_update_weights(c, nullptr, 0, pp, np, kPrecBits[prec], nullptr) == 0);   // the constant belongs to the old weights
                REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 64, prec, AMUSE_QUAT_P3D, nullptr, poses, trans, nullptr) == 0);
                REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, prec, AMUSE_QUAT_P3D, feats, poses, trans, s2) == 0);   // another stream: waits on the producer's event
                REQUIRE(amuse_debug_set_decode_tap(c, dtap) == 0);
                REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, prec, AMUSE_QUAT_P3D, feats, nullptr, nullptr, nullptr) == 0);
                REQUIRE(amuse_debug_set_decode_tap(c, nullptr) == 0);
                REQUIRE(amuse_debug_set_ablation(c, 1) == 0);
                REQUIRE(amuse_update_weights(c, nullptr, 0, pp, np, kPrecBits[prec], nullptr) == 0);
                REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, prec, AMUSE_QUAT_P3D, feats, nullptr, nullptr, nullptr) == 0);   // (ablation: no hoist)
                REQUIRE(amuse_debug_set_ablation(c, 0) == 0);
            }
            printf("== arch %d fp32x decode 64\n", arch);   // the rows8 hoist, and no hoist with lengths
            REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 64, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, feats, poses, trans, s2) == 0);
            REQUIRE(amuse_vae_encode(c, feats, lengths.data(), 64, AMUSE_PREC_F32X, nullptr, mu, sd, nullptr, nullptr) == 0);
            printf("== arch %d train-mode decode\n", arch);   // clip_index0 != 0: the setter's through amuse_vae_decode, the call's through amuse_diffusion_backward
            REQUIRE(amuse_set_decode_dropout(c, 0.25f, 11, 1000) == 0);
            REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 513, AMUSE_PREC_F32, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
            REQUIRE(amuse_vae_decode(c, lat, nullptr, 64, AMUSE_PREC_BF16, AMUSE_QUAT_P3D, feats, nullptr, nullptr, nullptr) == 0);
            REQUIRE(amuse_diffusion_backward(c, con, nullptr, nullptr, B, AMUSE_PREC_F16, AMUSE_QUAT_P3D, 1, 77, nullptr, nullptr, nullptr, poses, trans, nullptr) == 0);
            REQUIRE(amuse_diffusion_backward(c, con, nullptr, nullptr, B, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, 1, 77, nullptr, nullptr, nullptr, poses, trans, nullptr) != 0);
            printf("refused: %s\n", amuse_last_error());
            REQUIRE(amuse_set_decode_dropout(c, 0.f, 0, 0) == 0);
            printf("== arch %d forward per-clip timesteps\n", arch);
            REQUIRE(amuse_diffusion_forward(c, lat, lat2, tsb.data(), sa.data(), sb.data(), con, emo, nullptr, 300, AMUSE_PREC_BF16, mu, eps, nullptr) == 0);
            REQUIRE(amuse_sample(c, con, nullptr, nullptr, 300, AMUSE_PREC_F32, 3, 5, nullptr, nullptr, lat, nullptr, nullptr) == 0);
        }
        if (arch == AMUSE_ARCH_ENC) {
            printf("== arch %d train-mode sampling\n", arch);
            REQUIRE(amuse_set_sample_dropout(c, 0.1f, 5) == 0);
            REQUIRE(amuse_sample(c, con, emo, nullptr, B, AMUSE_PREC_BF16, 7, 3, nullptr, nullptr, lat, nullptr, nullptr) == 0);
            REQUIRE(amuse_denoise_step(c, lat, 5, con, nullptr, nullptr, B, AMUSE_PREC_F32, lat2, nullptr, nullptr) == 0);
            REQUIRE(amuse_sample(c, con, emo, nullptr, B, AMUSE_PREC_F32X, 7, 3, nullptr, nullptr, lat, nullptr, nullptr) != 0);
            printf("refused: %s\n", amuse_last_error());
            REQUIRE(amuse_set_sample_dropout(c, 0.f, 0) == 0);
        }
        if (arch == AMUSE_ARCH_ENC) {
            // the device re-pack invalidates the hoisted constants too.  Its gather maps are allocated and its launches go in the order of the slots' addresses,
            // which is no part of the contract: a context of its own, re-packed and destroyed with the log off
            printf("== arch %d decode after device re-pack\n", arch);
            amuse_stub_log(0);
            amuse_ctx* c2 = amuse_create_arch(0, arch, den.data(), den.size(), pp, np);
            REQUIRE(c2 != nullptr);
            amuse_stub_log(2);
            for (int i = 0; i < 2; ++i) {
                REQUIRE(amuse_vae_decode(c2, lat, nullptr, 64, AMUSE_PREC_BF16, AMUSE_QUAT_P3D, nullptr, poses, trans, nullptr) == 0);
                REQUIRE(amuse_vae_decode(c2, lat, nullptr, 64, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, nullptr, poses, trans, nullptr) == 0);
                REQUIRE(amuse_vae_decode(c2, lat, nullptr, 160, AMUSE_PREC_F32X, AMUSE_QUAT_P3D, nullptr, poses, trans, nullptr) == 0);
                if (i) break;
                amuse_stub_log(0);
                REQUIRE(amuse_update_weights_device(c2, nullptr, pri.data(), AMUSE_UPD_ALL, nullptr) == 0);
                amuse_stub_log(2);
            }
            const long live = amuse_stub_live_allocations();
            amuse_stub_log(0);
            amuse_destroy(c2);
            amuse_stub_log(2);
            printf("second context: %s\n", amuse_stub_live_allocations() < live ? "destroyed" : "still there");
        }
        if (pose) {
            printf("== arch %d staged 257\n", arch);   // 256 clips per chunk
            REQUIRE(amuse_set_decode_path(c, AMUSE_DECODE_STAGED) == 0);
            for (int prec : {AMUSE_PREC_F32, AMUSE_PREC_F32X}) {
                REQUIRE(amuse_sample(c, con, emo, nullptr, 257, prec, 7, 10, nullptr, nullptr, out, nullptr, nullptr) == 0);
                REQUIRE(amuse_denoise_step_pose(c, x, 5, con, nullptr, sty, lengths.data(), 257, prec, out, nullptr) == 0);
                REQUIRE(amuse_diffusion_forward(c, x, out, tsb.data(), sa.data(), sb.data(), con, nullptr, nullptr, 257, prec, nullptr, out, nullptr) == 0);
            }
            REQUIRE(amuse_set_decode_path(c, AMUSE_DECODE_AUTO) == 0);
            for (int n : {64, 160, 300}) {
                printf("== arch %d unpinned %d\n", arch, n);
                for (int prec : {AMUSE_PREC_BF16, AMUSE_PREC_F32X, AMUSE_PREC_F16}) {
                    REQUIRE(amuse_sample(c, con, emo, nullptr, n, prec, 7, 10, nullptr, nullptr, out, nullptr, nullptr) == 0);
                    REQUIRE(amuse_denoise_step_pose(c, x, 5, con, nullptr, nullptr, lengths.data(), n, prec, out, nullptr) == 0);
                    REQUIRE(amuse_diffusion_forward(c, x, out, tsb.data(), sa.data(), sb.data(), con, nullptr, nullptr, n, prec, nullptr, out, nullptr) == 0);
                }
            }
        }
        printf("== arch %d update and rerun\n", arch);   // a smaller call after larger ones: the grow-only buffers stay
        REQUIRE(amuse_update_weights(c, den.data(), den.size(), pp, np, AMUSE_UPD_BF16 | AMUSE_UPD_ENCODER, nullptr) == 0);
        REQUIRE(amuse_sample(c, con, nullptr, nullptr, B, AMUSE_PREC_BF16, 7, 0, nullptr, nullptr, state, nullptr, nullptr) != 0);   // the schedule must be set again
        printf("refused: %s\n", amuse_last_error());
        REQUIRE(amuse_set_schedule(c, &s, s2) == 0);
        REQUIRE(amuse_sample(c, con, nullptr, nullptr, B, AMUSE_PREC_BF16, 7, 0, nullptr, nullptr, state, nullptr, nullptr) == 0);
        if (latent) REQUIRE(amuse_vae_decode(c, lat, lengths.data(), 3, AMUSE_PREC_BF16, AMUSE_QUAT_P3D, feats, poses, trans, nullptr) == 0);
        printf("== arch %d destroy\n", arch);
        amuse_destroy(c);
        REQUIRE(amuse_stub_live_allocations() == 1);   // (the second stream)
        printf("live allocations after destroy: %ld\n", amuse_stub_live_allocations() - 1);
    }
    amuse_stub_log(0);
    amuse_stub_stream_destroy(s2);
    REQUIRE(amuse_stub_live_allocations() == 0);
    for (const void* p : {(const void*)con, (const void*)emo, (const void*)sty, (const void*)lat, (const void*)lat2, (const void*)mu, (const void*)sd, (const void*)eps,
                          (const void*)feats, (const void*)poses, (const void*)trans, (const void*)x, (const void*)out, (const void*)noise, (const void*)traj, (const void*)tap,
                          (const void*)dtap, (const void*)stamps})
        free(const_cast<void*>(p));
    printf("== end\nLAUNCH ARGS OK\n");
    return 0;
}
