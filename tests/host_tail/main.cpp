// The C ABI of AST_EVP's tail on the stubbed runtime (tests/host_asan/hip_stub.cpp + tail_stub.cpp), under ASan / UBSan: argument checks, set_tail,
// reconstruct, encode_labels, destroy.  Linked twice by build.sh: WITH amuse_audio_tail.o (host_tail) and WITHOUT it (host_notail, the objects of
// tests/host_asan/build.sh alone) - there every call that needs the tail must return AMUSE_ESTATE and launch / allocate nothing.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();
long amuse_tail_stub_launches() __attribute__((weak));
extern "C" const void* amuse_audio_tail_ops(void) __attribute__((weak));

#define REQUIRE(x)                                                                                  \
    do {                                                                                            \
        if (!(x)) {                                                                                 \
            printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #x, amuse_last_error());     \
            return 1;                                                                               \
        }                                                                                           \
    } while (0)

int main() {
    const bool linked = amuse_audio_tail_ops != nullptr;
    std::vector<float> ast(AMUSE_AST_PARAMS), mel((size_t)128 * 257), win(400, 0.5f);
    for (size_t i = 0; i < ast.size(); ++i) ast[i] = 0.05f * (float)((int)(i * 2654435761u >> 20 & 255) - 128) / 128.f;
    for (size_t i = 0; i < mel.size(); ++i) mel[i] = (i % 257) / 2 == i / 257 ? 1.0f : 0.0f;
    amuse_audio_ctx* a = amuse_audio_create(0, ast.data(), ast.data(), ast.data(), AMUSE_AST_PARAMS, mel.data(), win.data(), -4.f, 4.5f, 1);
    REQUIRE(a != nullptr);
    std::vector<float>().swap(ast);
    const int B = 34;   // two passes of the encoders (32 + 2 clips), two of the tail
    std::vector<float> fb((size_t)B * 1024 * 128, 0.25f), feat((size_t)B * 256, 0.5f), logits((size_t)B * 30), out((size_t)B * 1024 * 128), hid((size_t)B * 1024);
    const long live = amuse_stub_live_allocations();

    // ---- argument checks: nothing allocated, nothing launched
    REQUIRE(amuse_audio_set_tail(nullptr, feat.data(), AMUSE_AST_TAIL_PARAMS) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_set_tail(a, nullptr, AMUSE_AST_TAIL_PARAMS) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_set_tail(a, feat.data(), 17) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_CON, -1, fb.data(), 1, feat.data(), logits.data(), nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_encode_labels(a, 3, -1, fb.data(), 1, feat.data(), nullptr, nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_EMO, -1, fb.data(), 0, feat.data(), nullptr, nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_encode_labels(nullptr, AMUSE_AUDIO_EMO, -1, fb.data(), 1, feat.data(), nullptr, nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_EMO, -1, fb.data(), 1, feat.data(), logits.data(), nullptr) == AMUSE_ESTATE);   // no tail set / not linked
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 4, 3, out.data(), nullptr) == AMUSE_EINVAL);          // 4 % 3
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 17, 17, out.data(), nullptr) == AMUSE_EINVAL);        // group > 16
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 2, 0, out.data(), nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), nullptr, feat.data(), 2, 1, out.data(), nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 2, 1, nullptr, nullptr) == AMUSE_EINVAL);
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 2, 1, out.data(), nullptr) == AMUSE_ESTATE);          // no tail set / not linked
    REQUIRE(strstr(amuse_last_error(), linked ? "no tail set" : "not linked") != nullptr);
    REQUIRE(amuse_debug_tail_hidden(a, feat.data(), feat.data(), feat.data(), 2, 1, hid.data(), nullptr) == AMUSE_ESTATE);
    REQUIRE(amuse_stub_live_allocations() == live);
    if (amuse_tail_stub_launches) REQUIRE(amuse_tail_stub_launches() == 0);

    if (!linked) {
        std::vector<float> some(16);
        REQUIRE(amuse_audio_set_tail(a, some.data(), AMUSE_AST_TAIL_PARAMS) == AMUSE_ESTATE);   // refused before the array is read
        REQUIRE(strstr(amuse_last_error(), "not linked") != nullptr);
        REQUIRE(amuse_stub_live_allocations() == live);
        REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_STY, 0, fb.data(), 2, feat.data(), nullptr, nullptr) == AMUSE_OK);   // features alone need no tail
        amuse_audio_destroy(a);
        REQUIRE(amuse_stub_live_allocations() == 0);
        printf("AUDIO TAIL STUB OK (tail not linked)\n");
        return 0;
    }

    // ---- the tail: upload, replace, run
    {
        std::vector<float> tail(AMUSE_AST_TAIL_PARAMS);
        for (size_t i = 0; i < tail.size(); ++i) tail[i] = 0.03f * (float)((int)(i * 2654435761u >> 19 & 511) - 256) / 256.f;
        REQUIRE(amuse_audio_set_tail(a, tail.data(), AMUSE_AST_TAIL_PARAMS) == AMUSE_OK);
        const long with_tail = amuse_stub_live_allocations();
        REQUIRE(with_tail > live);
        REQUIRE(amuse_audio_set_tail(a, tail.data(), AMUSE_AST_TAIL_PARAMS) == AMUSE_OK);   // again: the old images are freed
        REQUIRE(amuse_stub_live_allocations() == with_tail);
    }
    long n0 = amuse_tail_stub_launches();
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 1, 1, out.data(), nullptr) == AMUSE_OK);
    const long per_pass = amuse_tail_stub_launches() - n0;
    REQUIRE(per_pass == 1 + 6 * 7 + 2 + 2 + 1);       // cat, six layers of seven launches, fusion norm + fc, decoder norm + projection.0, the last Linear
    n0 = amuse_tail_stub_launches();
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), B, 2, out.data(), nullptr) == AMUSE_OK);   // 32 + 2 rows
    REQUIRE(amuse_tail_stub_launches() - n0 == 2 * per_pass);
    n0 = amuse_tail_stub_launches();
    REQUIRE(amuse_audio_reconstruct(a, feat.data(), feat.data(), feat.data(), 33, 11, out.data(), nullptr) == AMUSE_OK);  // whole groups per pass: 22 + 11 rows
    REQUIRE(amuse_tail_stub_launches() - n0 == 2 * per_pass);
    n0 = amuse_tail_stub_launches();
    REQUIRE(amuse_debug_tail_hidden(a, feat.data(), feat.data(), feat.data(), 5, 5, hid.data(), nullptr) == AMUSE_OK);
    REQUIRE(amuse_tail_stub_launches() - n0 == per_pass - 1);
    for (int fbflag = -1; fbflag <= 1; ++fbflag) {
        n0 = amuse_tail_stub_launches();
        REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_EMO, fbflag, fb.data(), B, feat.data(), logits.data(), nullptr) == AMUSE_OK);
        REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_STY, fbflag, fb.data(), B, feat.data(), logits.data(), nullptr) == AMUSE_OK);
        REQUIRE(amuse_tail_stub_launches() - n0 == 4);   // one head launch per encoder pass (32 + 2 clips)
    }
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_CON, 0, fb.data(), 3, feat.data(), nullptr, nullptr) == AMUSE_OK);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_CON, 1, fb.data(), 1, feat.data(), logits.data(), nullptr) == AMUSE_EINVAL);
    amuse_audio_destroy(a);
    REQUIRE(amuse_stub_live_allocations() == 0);
    printf("AUDIO TAIL STUB OK\n");
    return 0;
}
