// Prints the image log of hip_stub.cpp (every uploaded image, every stage / unit table a launcher is handed, every device re-pack) for all four Denoiser archs,
// in named sections: tests/test_pack_images_cpu.py compares it with tests/golden/pack_images.json.  C ABI only; parameters from main.cpp's LCG.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();
void amuse_stub_log(int on);

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, amuse_last_error()); return 1; } \
    } while (0)

static void fill(std::vector<float>& v, uint32_t seed, float scale) {
    uint32_t s = seed;
    for (float& x : v) { s = s * 1664525u + 1013904223u; x = (((s >> 8) & 0xffff) / 65536.0f - 0.5f) * scale; }
}

int main() {
    const int B = 2, T = 2;
    const int kPrecBits[4] = {AMUSE_UPD_F32, AMUSE_UPD_BF16, AMUSE_UPD_F32X, AMUSE_UPD_F16};
    std::vector<float> pri(AMUSE_PRIOR_PARAMS), cond((size_t)B * 256, 0.25f), lat((size_t)B * 128), feats((size_t)B * 300 * 333), poses((size_t)B * 300 * 55 * 3),
        trans((size_t)B * 300 * 3), x((size_t)B * AMUSE_POSE_STATE), out((size_t)B * AMUSE_POSE_STATE), coef((size_t)T * 8, 0.5f), sa(B, 0.9f), sb(B, 0.1f);
    std::vector<unsigned long long> stamps(4 * 192);
    std::vector<int> ts{1, 0}, tsb(B, 1);
    fill(pri, 2, 0.2f);
    amuse_stub_log(1);
    for (int arch : {AMUSE_ARCH_ENC, AMUSE_ARCH_DEC, AMUSE_ARCH_ENC_POSE, AMUSE_ARCH_DEC_POSE}) {
        const bool pose = (arch & 2) != 0;
        std::vector<float> den(amuse_denoiser_param_count(arch));
        fill(den, 10 + arch, 0.2f);
        const float* pp = pose ? nullptr : pri.data();
        const size_t np = pose ? 0 : pri.size();
        printf("== arch %d create\n", arch);
        amuse_ctx* c = amuse_create_arch(0, arch, den.data(), den.size(), pp, np);
        REQUIRE(c != nullptr);
        fill(den, 20 + arch, 0.1f);
        for (int p = 0; p < 4; ++p)
            for (int enc : {0, (int)AMUSE_UPD_ENCODER}) {
                printf("== arch %d update what=%d\n", arch, kPrecBits[p] | enc);
                REQUIRE(amuse_update_weights(c, den.data(), den.size(), pp, np, kPrecBits[p] | enc, nullptr) == 0);
            }
        printf("== arch %d schedule\n", arch);
        amuse_schedule s{T, ts.data(), coef.data(), nullptr};
        REQUIRE(amuse_set_schedule(c, &s, nullptr) == 0);
        float* state = pose ? out.data() : lat.data();
        for (int prec = AMUSE_PREC_F32; prec <= AMUSE_PREC_F16; ++prec)
            for (int path : {AMUSE_DECODE_STAGED, AMUSE_DECODE_FUSED, AMUSE_DECODE_CLIP}) {
                printf("== arch %d calls prec=%d path=%d\n", arch, prec, path);
                REQUIRE(amuse_set_decode_path(c, path) == 0);
                REQUIRE(amuse_sample(c, cond.data(), cond.data(), nullptr, B, prec, 7, 0, nullptr, nullptr, state, nullptr, nullptr) == 0);
                REQUIRE(amuse_denoise_step(c, x.data(), 5, cond.data(), nullptr, nullptr, B, prec, out.data(), nullptr, nullptr) == 0);
                REQUIRE(amuse_diffusion_forward(c, x.data(), x.data(), tsb.data(), sa.data(), sb.data(), cond.data(), nullptr, nullptr, B, prec, nullptr, out.data(), nullptr) == 0);
                REQUIRE(amuse_diffusion_backward(c, cond.data(), nullptr, nullptr, B, prec, AMUSE_QUAT_P3D, 1, 0, nullptr, nullptr, nullptr, poses.data(), trans.data(), nullptr) == 0);
                if (arch == AMUSE_ARCH_ENC) REQUIRE(amuse_profile_sample(c, cond.data(), nullptr, nullptr, B, prec, 0, stamps.data(), nullptr) == 0);
                if (pose) {
                    REQUIRE(amuse_denoise_step_pose(c, x.data(), 5, cond.data(), nullptr, nullptr, nullptr, B, prec, out.data(), nullptr) == 0);
                    continue;
                }
                REQUIRE(amuse_vae_decode(c, lat.data(), nullptr, B, prec, AMUSE_QUAT_P3D, feats.data(), poses.data(), trans.data(), nullptr) == 0);
                REQUIRE(amuse_vae_encode(c, feats.data(), nullptr, B, prec, nullptr, lat.data(), nullptr, nullptr, nullptr) == 0);
                if (prec != AMUSE_PREC_F32X && path == AMUSE_DECODE_STAGED) {   // train-mode decode: the dropout instantiations take the same tables
                    REQUIRE(amuse_set_decode_dropout(c, 0.1f, 3, 0) == 0);
                    REQUIRE(amuse_vae_decode(c, lat.data(), nullptr, B, prec, AMUSE_QUAT_P3D, feats.data(), nullptr, nullptr, nullptr) == 0);
                    REQUIRE(amuse_set_decode_dropout(c, 0.f, 0, 0) == 0);
                }
            }
        if (arch == AMUSE_ARCH_ENC) {   // the device re-pack (shipped configuration only): the gather maps are built and uploaded by the first call
            printf("== arch %d device what=%d\n", arch, AMUSE_UPD_ALL);
            REQUIRE(amuse_update_weights_device(c, den.data(), pri.data(), AMUSE_UPD_ALL, nullptr) == 0);
            for (int p = 0; p < 4; ++p)
                for (int enc : {0, (int)AMUSE_UPD_ENCODER}) {
                    printf("== arch %d device what=%d\n", arch, kPrecBits[p] | enc);
                    REQUIRE(amuse_update_weights_device(c, den.data(), pri.data(), kPrecBits[p] | enc, nullptr) == 0);
                }
        }
        printf("== arch %d destroy\n", arch);
        amuse_destroy(c);
        REQUIRE(amuse_stub_live_allocations() == 0);
    }
    printf("== end\nPACK IMAGES OK\n");
    return 0;
}
