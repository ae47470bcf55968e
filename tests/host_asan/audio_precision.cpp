// amuse_audio_set_precision on the host-only build (hip_stub.cpp + the library's host objects, WITHOUT amuse_audio_x.o): the parity mode's translation
// unit is not linked there, so AMUSE_PREC_F32X must be refused with AMUSE_ESTATE and change nothing; the bf16 mode and the argument checks work as in
// the full library.  Built and run by tests/test_audio_precision_abi_cpu.py on the objects of tests/host_asan/build.sh.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();

#define REQUIRE(x)                                                    \
    do {                                                              \
        if (!(x)) {                                                   \
            printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #x, amuse_last_error()); \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    REQUIRE(amuse_audio_set_precision(nullptr, AMUSE_PREC_BF16) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_precision(nullptr) == AMUSE_EINVAL);
    std::vector<float> ast(AMUSE_AST_PARAMS), mel((size_t)128 * 257), win(400, 0.5f);
    for (size_t i = 0; i < ast.size(); ++i) ast[i] = 0.05f * (float)((int)(i * 2654435761u >> 20 & 255) - 128) / 128.f;
    for (size_t i = 0; i < mel.size(); ++i) mel[i] = (i % 257) / 2 == i / 257 ? 1.0f : 0.0f;
    amuse_audio_ctx* a = amuse_audio_create(0, ast.data(), ast.data(), ast.data(), AMUSE_AST_PARAMS, mel.data(), win.data(), -4.f, 4.5f, 1);
    REQUIRE(a != nullptr);
    const long live = amuse_stub_live_allocations();
    REQUIRE(amuse_audio_precision(a) == AMUSE_PREC_BF16);
    REQUIRE(amuse_audio_set_precision(a, AMUSE_PREC_F32X) == AMUSE_ESTATE);
    REQUIRE(strstr(amuse_last_error(), "not linked") != nullptr);
    REQUIRE(amuse_audio_precision(a) == AMUSE_PREC_BF16 && amuse_stub_live_allocations() == live);
    REQUIRE(amuse_audio_set_precision(a, AMUSE_PREC_BF16) == AMUSE_OK);
    const int bads[] = {AMUSE_PREC_F32, AMUSE_PREC_F16, -1, 4, 1000};
    for (int bad : bads) {
        REQUIRE(amuse_audio_set_precision(a, bad) == AMUSE_EINVAL);
        REQUIRE(amuse_audio_precision(a) == AMUSE_PREC_BF16);
    }
    std::vector<float> fb((size_t)1024 * 128), f256(256);
    REQUIRE(amuse_audio_encode(a, 0, fb.data(), 1, f256.data(), nullptr, 0, nullptr) == 0);
    amuse_audio_destroy(a);
    REQUIRE(amuse_stub_live_allocations() == 0);
    printf("AUDIO PRECISION STUB OK\n");
    return 0;
}
