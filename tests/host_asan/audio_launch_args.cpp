// Prints the launch log of hip_stub.cpp + audio_x_stub.cpp (amuse_stub_log(2)) for the audio front-end in named sections: tests/test_audio_launch_args_cpu.py
// compares it, in order, with tests/golden/audio_launch_args.json.  Both precisions of the AST encoders are linked (amuse_audio_x.o, amuse_audio_tail.o and the
// stubs of their launchers beside what build.sh links).  Without an argument: create, every entry point of the encoders in bf16, the switch to fp32x (the split
// images are built, the host copy goes), the same calls in fp32x, the switches back and forth (nothing is built or allocated again), the refusals, destroy.  With
// the argument `tail`: amuse_audio_set_tail, then the labels with logits - whose frame-based form takes the mode's SECOND pooling - in both precisions; a process
// of its own because three encoders in two modes beside the tail's 131072 x 1024 Linear are several GB.
// C ABI only; parameters from main.cpp's LCG, one array shared by the three encoders as there.  The large buffers are never touched by the encoders' launchers
// (no-ops): they only give the pointers a name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static const int NB = 33;   // clips the named buffers hold: the smallest count that crosses the 32-clip chunk loop
static float *wav, *fb, *con, *emo, *sty, *hid, *logits;
static void* s2;

// every entry point of the encoders, in the context's current precision
static int encoder_calls(amuse_audio_ctx* a, const char* tag) {
    printf("== %s fbank\n", tag);
    REQUIRE(amuse_audio_fbank(a, wav, 16000, 2, fb, nullptr) == 0);
    for (int which = 0; which < 3; ++which) {
        printf("== %s encode which=%d B=1\n", tag, which);
        REQUIRE(amuse_audio_encode(a, which, fb, 1, con, hid, 0, nullptr) == 0);
        REQUIRE(amuse_audio_encode(a, which, fb, 1, emo, hid, 11, nullptr) == 0);
        REQUIRE(amuse_audio_encode(a, which, fb, 1, sty, nullptr, 0, nullptr) == 0);
    }
    printf("== %s features B=2 second stream\n", tag);
    REQUIRE(amuse_audio_features(a, wav, 16000, 2, con, emo, sty, s2) == 0);
    printf("== %s features B=3 no emo\n", tag);
    REQUIRE(amuse_audio_features(a, wav, 16000, 3, con, nullptr, sty, nullptr) == 0);
    printf("== %s encode B=33\n", tag);   // two chunks (32 + 1); workspace 0 grows: freed and allocated again
    REQUIRE(amuse_audio_encode(a, AMUSE_AUDIO_EMO, fb, NB, emo, hid, 5, nullptr) == 0);
    printf("== %s encode B=1 again\n", tag);   // the grow-only workspace stays
    REQUIRE(amuse_audio_encode(a, AMUSE_AUDIO_CON, fb, 1, con, nullptr, 0, s2) == 0);
    printf("== %s encode_labels without logits\n", tag);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_CON, -1, fb, 1, con, nullptr, nullptr) == 0);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_EMO, 0, fb, 2, emo, nullptr, nullptr) == 0);
    REQUIRE(amuse_audio_encode_labels(a, AMUSE_AUDIO_STY, 1, fb, 1, sty, nullptr, s2) == 0);
    return 0;
}

// the labels with logits: frame-based 1 takes the second pooling (the mode table's `pool`, AudioModeOps of amuse_audio_enc.hpp), 0 the features themselves
static int label_calls(amuse_audio_ctx* a, const char* tag) {
    printf("== %s labels with logits\n", tag);
    for (int which : {AMUSE_AUDIO_EMO, AMUSE_AUDIO_STY})
        for (int frame_based : {1, 0}) REQUIRE(amuse_audio_encode_labels(a, which, frame_based, fb, 1, which == AMUSE_AUDIO_EMO ? emo : sty, logits, nullptr) == 0);
    return 0;
}

int main(int argc, char** argv) {
    const bool tail = argc > 1 && !strcmp(argv[1], "tail");
    const char* pre = tail ? "tail " : "";
    std::vector<float> ast(AMUSE_AST_PARAMS), mel((size_t)128 * 257), win(400, 0.5f);
    fill(ast, 5, 0.05f);
    for (size_t i = 0; i < mel.size(); ++i) mel[i] = (i % 257) / 2 == i / 257 ? 1.0f : 0.0f;   // a sparse bank with supports
    wav = named("wav", (size_t)NB * 16000); fb = named("fb", (size_t)NB * 1024 * 128); con = named("con", (size_t)NB * 256); emo = named("emo", (size_t)NB * 256);
    sty = named("sty", (size_t)NB * 256); hid = named("hid", (size_t)NB * 1214 * 768); logits = named("logits", (size_t)NB * 30);
    memset(con, 0, (size_t)NB * 256 * 4); memset(emo, 0, (size_t)NB * 256 * 4); memset(sty, 0, (size_t)NB * 256 * 4);   // (the tail's stub reads the features it is handed)
    s2 = amuse_stub_stream_create();
    amuse_stub_log(2);
    printf("== %screate\n", pre);
    amuse_audio_ctx* a = amuse_audio_create(0, ast.data(), ast.data(), ast.data(), AMUSE_AST_PARAMS, mel.data(), win.data(), -4.f, 4.5f, 1);
    REQUIRE(a != nullptr);
    if (tail) {
        printf("== tail set_tail\n");
        {
            std::vector<float> tp(AMUSE_AST_TAIL_PARAMS);
            fill(tp, 7, 0.05f);
            REQUIRE(amuse_audio_set_tail(a, tp.data(), tp.size()) == 0);
        }
        if (label_calls(a, "tail bf16")) return 1;
        printf("== tail set_precision fp32x\n");
        REQUIRE(amuse_audio_set_precision(a, AMUSE_PREC_F32X) == 0);
        if (label_calls(a, "tail fp32x")) return 1;
    } else {
        if (encoder_calls(a, "bf16")) return 1;
        printf("== set_precision fp32x\n");   // the split images of the three encoders; the host copy of the parameters is released
        REQUIRE(amuse_audio_set_precision(a, AMUSE_PREC_F32X) == 0 && amuse_audio_precision(a) == AMUSE_PREC_F32X);
        if (encoder_calls(a, "fp32x")) return 1;
        printf("== back to bf16\n");   // no allocation may appear
        REQUIRE(amuse_audio_set_precision(a, AMUSE_PREC_BF16) == 0 && amuse_audio_precision(a) == AMUSE_PREC_BF16);
        REQUIRE(amuse_audio_encode(a, AMUSE_AUDIO_STY, fb, 1, sty, hid, 3, nullptr) == 0);
        printf("== to fp32x again\n");   // no rebuild, no allocation
        REQUIRE(amuse_audio_set_precision(a, AMUSE_PREC_F32X) == 0);
        REQUIRE(amuse_audio_encode(a, AMUSE_AUDIO_STY, fb, 1, sty, hid, 3, nullptr) == 0);
        printf("== refusals\n");
        REQUIRE(amuse_audio_encode(a, 3, fb, 1, con, nullptr, 0, nullptr) != 0);
        printf("refused: %s\n", amuse_last_error());
        REQUIRE(amuse_audio_encode(a, 0, fb, 1, con, hid, 12, nullptr) != 0);
        printf("refused: %s\n", amuse_last_error());
        REQUIRE(amuse_audio_features(a, wav, 0, 1, con, nullptr, nullptr, nullptr) != 0);
        printf("refused: %s\n", amuse_last_error());
    }
    printf("== %sdestroy\n", pre);
    amuse_audio_destroy(a);
    REQUIRE(amuse_stub_live_allocations() == 1);   // (the second stream)
    printf("live allocations after destroy: %ld\n", amuse_stub_live_allocations() - 1);
    amuse_stub_log(0);
    amuse_stub_stream_destroy(s2);
    REQUIRE(amuse_stub_live_allocations() == 0);
    for (float* p : {wav, fb, con, emo, sty, hid, logits}) free(p);
    printf("== %send\nAUDIO LAUNCH ARGS OK\n", pre);
    return 0;
}
