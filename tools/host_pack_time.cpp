// Host time of one amuse_update_weights(..., AMUSE_UPD_ALL) on the shipped arch (what a training iteration without the device re-pack pays), on the stubbed HIP
// runtime of tests/host_asan/hip_stub.cpp - no GPU.  Build two trees and alternate them (tools/host_pack_time.sh OLD_TREE NEW_TREE; profiles/pack_refactor_host_time.txt).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "amuse_hip.h"

int main() {
    std::vector<float> den(AMUSE_DENOISER_PARAMS), pri(AMUSE_PRIOR_PARAMS);
    uint32_t s = 1;
    for (auto* v : {&den, &pri})
        for (float& x : *v) { s = s * 1664525u + 1013904223u; x = (((s >> 8) & 0xffff) / 65536.0f - 0.5f) * 0.2f; }
    amuse_ctx* c = amuse_create(0, den.data(), den.size(), pri.data(), pri.size());
    if (!c) { printf("create failed: %s\n", amuse_last_error()); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    if (amuse_update_weights(c, den.data(), den.size(), pri.data(), pri.size(), AMUSE_UPD_ALL, nullptr)) { printf("update failed: %s\n", amuse_last_error()); return 1; }
    printf("%.1f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    amuse_destroy(c);
    return 0;
}
