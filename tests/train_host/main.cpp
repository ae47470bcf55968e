// The training step's host code (csrc/amuse_train.hip, and the launchers of k_train.hip, k_train_attn.hip, k_train_gemm.hip) in a stand-alone program under
// AddressSanitizer / UBSan: the translation units are linked as they are against the stubbed HIP runtime of tests/host_asan at its raw launch level
// (amuse_stub_log(3)), so every <<< >>> prints kernel name, grid, block, dynamic LDS, stream and - through the table of parameter letters below - its pointer and
// scalar arguments, and every runtime call its line.  tests/test_train_launch_args_cpu.py compares the sections with tests/golden/train_launch_args.json.
// Behind the golden's sections (`-- ` lines, not in the golden): the error paths, which this program asserts itself - refused calls launch nothing, every failure
// between a layer's fork and join still joins, a missing epoch word is an error.
// No buffer is ever touched: kernels do not run.  Every pointer field of amuse_train_layer gets an address of its own in a range that is never mapped.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();
void amuse_stub_log(int on);
void amuse_stub_name(const char* name, const void* p, size_t bytes);
void* amuse_stub_stream_create();
void amuse_stub_stream_destroy(void* s);
void amuse_stub_kernel_params(const char* (*lookup)(const char* mangled));
void amuse_stub_fail_at(long n);
long amuse_stub_steps();
void amuse_stub_capture(std::vector<std::string>* lines);

// the library's error slot (amuse_api.hip is not linked)
static char g_error[512];
__attribute__((format(printf, 2, 3))) int amuse_failf(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

#define REQUIRE(cond)                                                                      \
    do {                                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_error); return 1; } \
    } while (0)

// one letter per kernel parameter (hip_stub.cpp hipLaunchKernel), keyed by <length><name> of the mangled kernel name
static const char* kernel_params(const char* mangled) {
    static const struct { const char* key; const char* letters; } table[] = {
        {"14k_train_ln_fwd", "pppppufUUplppp"}, {"14k_train_ln_bwd", "pppppufUUplppp"}, {"16k_train_finalize", "pipppii"}, {"18k_train_layer_sums", "S"},
        {"13k_train_adamw", "ppppzfffffff"}, {"21k_train_adamw_scalars", "pdddp"}, {"17k_train_adamw_dev", "ppppzpfffff"}, {"15k_train_bgd_fwd", "ppufUUpzip"},
        {"15k_train_bgd_bwd", "pppufUUplipp"}, {"14k_train_colsum", "plip"}, {"17k_train_bias_rows", "pzip"}, {"10k_train_vk", "pufUUpliip"},
        {"10k_train_dc", "pufUUpiip"}, {"17k_train_epoch_set", "puui"}, {"13k_train_wgrad", "pppiii"}, {"17k_train_wgrad_sum", "pizp"},
        {"18k_train_colsum_any", "pliip"}, {"22k_train_colsum_any_fin", "piip"}, {"17k_train_gemm_tall", "ppppiiii"}, {"16k_train_gemm_any", "ppppiiiiip"},
        {"14k_gemm_any_sum", "pizipip"}, {"10k_attn_fwd", "S"}, {"10k_attn_bwd", "S"},
    };
    for (const auto& t : table)
        if (strstr(mangled, t.key)) return t.letters;
    return nullptr;
}

// addresses that name themselves: 256 MB apart in a range nothing maps, 16-byte aligned
static float* named(const std::string& name, size_t floats = (size_t)8 << 20) {
    static uintptr_t next = (uintptr_t)0x500000000000ull;
    float* p = reinterpret_cast<float*>(next);
    next += (uintptr_t)256 << 20;
    amuse_stub_name(name.c_str(), p, floats * sizeof(float));
    return p;
}

struct Layer {
    amuse_train_layer L;
    // decoder: mem given; self: Win given
    Layer(const char* tag, int B, int S, int ff, bool decoder, bool self) {
        memset(&L, 0, sizeof(L));
        const std::string t = std::string(tag) + ".";
        auto N = [&](const char* f) { return named(t + f); };
        L.rows = (long)B * S; L.B = B; L.S = S; L.H = 4; L.ff = ff;
        L.p = 0.1f; L.p_attn = 0.2f; L.seed = 0x1234567887654321ull;
        for (int i = 0; i < 5; ++i) L.off[i] = 1000 + 17 * i;
        L.off_self = 7777;
#define F_(f) L.f = N(#f)
        F_(Wo); F_(bo); F_(g1); F_(be1); F_(W1); F_(b1); F_(W2); F_(b2); F_(g3); F_(be3); F_(x); F_(o2); F_(x1); F_(zh1); F_(r1); F_(h); F_(a); F_(out); F_(zh3); F_(r3); F_(tmp);
        F_(dout); F_(dx); F_(do2); F_(dWo); F_(dbo); F_(dg1); F_(dbe1); F_(dW1); F_(db1); F_(dW2); F_(db2); F_(dg3); F_(dbe3); F_(s128a); F_(s128b); F_(s512a); F_(s512b);
        L.ws = named(t + "ws", amuse_train_ws_floats());
        if (decoder) { F_(Wv); F_(bv); F_(Wc); F_(bc); F_(g2); F_(be2); F_(mem); F_(c); F_(vk); F_(xm); F_(zh2); F_(r2); F_(dmem); F_(dWv); F_(dbv); F_(dWc); F_(dbc); F_(dg2); F_(dbe2); F_(sdc); }
        if (self) { F_(Win); F_(bin); F_(qkv); F_(lse); F_(dqkv); F_(dWin); F_(dbin); }
#undef F_
    }
};

static int layer_both(const char* name, const amuse_train_layer& L, void* stream) {
    printf("== %s fwd\n", name);
    REQUIRE(amuse_train_layer_fwd(&L, stream) == 0);
    printf("== %s bwd\n", name);
    REQUIRE(amuse_train_layer_bwd(&L, stream) == 0);
    return 0;
}

// ---- the error paths.  The stub counts every runtime call and launch it can fail (amuse_stub_steps) and fails the n-th on request (amuse_stub_fail_at; it
// prints `-- injected failure` there); amuse_stub_capture hands this program the lines of a call
static long steps_of(int (*call)(const amuse_train_layer*, void*), const amuse_train_layer& L, void* st, int* ret) {
    amuse_stub_fail_at(-1);   // (never reached: counts only)
    *ret = call(&L, st);
    const long n = amuse_stub_steps();
    amuse_stub_fail_at(0);
    return n;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    setvbuf(stdout, nullptr, _IOLBF, 0);
    amuse_stub_kernel_params(kernel_params);
    amuse_stub_log(3);
    void* s1 = amuse_stub_stream_create();
    float *A = named("A"), *Bm = named("B"), *C = named("C"), *D = named("D"), *E = named("E"), *F = named("F"), *G = named("G"), *H = named("H"), *I = named("I");
    float* ws = named("ws", amuse_train_ws_floats());
    const uint64_t seed = 0xabcdef0123456789ull;

    if (mode == "noepoch") {   // a process of its own: no epoch word yet, and its allocation fails - every mask-drawing entry point is an error and launches nothing
        Layer dec("dec1200", 4, 300, 512, true, true);
        int n = 0;
#define NO_EPOCH(call)                                                                 \
        amuse_stub_fail_at(1);                                                         \
        REQUIRE((call) == AMUSE_EHIP && amuse_stub_steps() == 1);                      \
        ++n;
        NO_EPOCH(amuse_train_ln_fwd(A, Bm, C, D, E, 0.1f, seed, 11, 1207, F, G, H, s1));
        NO_EPOCH(amuse_train_ln_bwd(A, Bm, C, D, E, 0.1f, seed, 13, 1207, F, G, H, I, nullptr, ws, s1));
        NO_EPOCH(amuse_train_bias_gelu_drop_fwd(A, Bm, 0.1f, seed, 15, 1207, 512, C, s1));
        NO_EPOCH(amuse_train_bias_gelu_drop_bwd(A, Bm, C, 0.1f, seed, 16, 1207, 512, D, E, ws, s1));
        NO_EPOCH(amuse_train_attn_fwd(A, 4, 300, 0.1f, seed, 22, Bm, C, nullptr, s1));
        NO_EPOCH(amuse_train_attn_bwd(A, Bm, C, D, 4, 300, 0.1f, seed, 22, E, s1));
        NO_EPOCH(amuse_train_epoch_advance(1, s1));
        NO_EPOCH(amuse_train_epoch_set(5, s1));
        NO_EPOCH(amuse_train_layer_fwd(&dec.L, s1));
        NO_EPOCH(amuse_train_layer_bwd(&dec.L, s1));
#undef NO_EPOCH
        amuse_stub_fail_at(0);
        amuse_stub_stream_destroy(s1);
        printf("-- %d entry points refuse without the epoch word\nlive allocations at exit: %ld\ntrain_host ok\n", n, amuse_stub_live_allocations());
        return 0;
    }

    // ---- every raw entry point, once each (the first mask-drawing call creates the device's epoch word)
    printf("== raw ln_fwd\n");
    REQUIRE(amuse_train_ln_fwd(A, Bm, C, D, E, 0.1f, seed, 11, 1207, F, G, H, s1) == 0);
    printf("== raw ln_fwd rows=40000 no x no state\n");
    REQUIRE(amuse_train_ln_fwd(nullptr, Bm, nullptr, D, E, 0.f, seed, 12, 40000, F, nullptr, nullptr, nullptr) == 0);
    printf("== raw ln_bwd\n");
    REQUIRE(amuse_train_ln_bwd(A, Bm, C, D, E, 0.1f, seed, 13, 1207, F, G, H, I, nullptr, ws, s1) == 0);
    printf("== raw ln_bwd rows=100000\n");
    REQUIRE(amuse_train_ln_bwd(A, nullptr, C, D, E, 0.25f, seed, 14, 100000, nullptr, G, H, I, F, ws, nullptr) == 0);
    printf("== raw bias_gelu_drop_fwd\n");
    REQUIRE(amuse_train_bias_gelu_drop_fwd(A, Bm, 0.1f, seed, 15, 1207, 512, C, s1) == 0);
    REQUIRE(amuse_train_bias_gelu_drop_fwd(A, Bm, 0.1f, seed, 15, 20000, 1024, C, s1) == 0);
    printf("== raw bias_gelu_drop_bwd\n");
    REQUIRE(amuse_train_bias_gelu_drop_bwd(A, Bm, C, 0.1f, seed, 16, 1207, 512, D, E, ws, s1) == 0);
    REQUIRE(amuse_train_bias_gelu_drop_bwd(A, Bm, C, 0.1f, seed, 16, 33, 36, D, E, ws, s1) == 0);
    printf("== raw colsum\n");
    REQUIRE(amuse_train_colsum(A, 1207, 384, Bm, ws, s1) == 0);
    REQUIRE(amuse_train_colsum(A, 3, 4, Bm, ws, nullptr) == 0);
    printf("== raw refusals\n");
    REQUIRE(amuse_train_ln_fwd(A, nullptr, C, D, E, 0.1f, seed, 11, 1207, F, G, H, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_ln_fwd(A, Bm, C, D, E, 1.0f, seed, 11, 1207, F, G, H, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_ln_bwd(A, Bm, C, D, E, 0.1f, seed, 13, 0, F, G, H, I, nullptr, ws, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_bias_gelu_drop_fwd(A, Bm, 0.1f, seed, 15, 1207, 510, C, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_bias_gelu_drop_bwd(A, Bm, C, 0.1f, seed, 16, 1207, 512, D, E, nullptr, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_colsum(A, 1207, 1028, Bm, ws, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_set_lane(2) == AMUSE_EINVAL);

    // ---- linear forward / backward: one shape per branch of the GEMM dispatch
    struct Lin { const char* name; long rows; int K, N; int off; } lins[] = {
        {"tall projection rows=1200 K=128 N=384", 1200, 128, 384, 0},   {"N=333 rows=1200 K=128", 1200, 128, 333, 0},
        {"32 rows K=128 N=128", 32, 128, 128, 0},                       {"long reduction rows=9600 K=128 N=512", 9600, 128, 512, 0},
        {"long reduction rows=9600 K=128 N=128", 9600, 128, 128, 0},    {"long reduction beyond 64 chunks rows=12480 K=128 N=128", 12480, 128, 128, 0},
        {"ragged rows=1204 K=512 N=128", 1204, 512, 128, 0},            {"operands on a 4-byte boundary rows=1200 K=128 N=384", 1200, 128, 384, 1},
    };
    for (const Lin& l : lins) {
        printf("== linear_fwd %s\n", l.name);
        REQUIRE(amuse_train_linear_fwd(A + l.off, Bm + l.off, C, l.rows, l.K, l.N, D, s1) == 0);
        REQUIRE(amuse_train_linear_fwd(A + l.off, Bm + l.off, nullptr, l.rows, l.K, l.N, D, nullptr) == 0);
        printf("== linear_bwd %s\n", l.name);
        REQUIRE(amuse_train_linear_bwd(A + l.off, Bm + l.off, C + l.off, l.rows, l.K, l.N, D, E, F, 0, ws, s1) == 0);
        REQUIRE(amuse_train_linear_bwd(A + l.off, Bm + l.off, C + l.off, l.rows, l.K, l.N, D, nullptr, F, 1, nullptr, s1) == 0);
        REQUIRE(amuse_train_linear_bwd(A + l.off, Bm + l.off, C + l.off, l.rows, l.K, l.N, nullptr, E, nullptr, 0, ws, nullptr) == 0);
    }
    printf("== linear refusals\n");
    REQUIRE(amuse_train_linear_fwd(A, nullptr, C, 32, 128, 128, D, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_linear_bwd(A, Bm, C, 32, 128, 1028, D, E, F, 0, ws, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_linear_bwd(A, Bm, C, 32, 128, 128, D, E, F, 0, nullptr, s1) == AMUSE_EINVAL);

    // ---- attention
    printf("== attn_fwd one part B=2 S=8\n");
    REQUIRE(amuse_train_attn_fwd(A, 2, 8, 0.1f, seed, 21, Bm, C, nullptr, s1) == 0);
    printf("== attn_fwd two parts B=4 S=300\n");
    REQUIRE(amuse_train_attn_fwd(A, 4, 300, 0.1f, seed, 22, Bm, C, nullptr, s1) == 0);
    printf("== attn_fwd one part B=128 S=300\n");
    REQUIRE(amuse_train_attn_fwd(A, 128, 300, 0.f, seed, 22, Bm, C, nullptr, nullptr) == 0);
    printf("== attn_fwd mask_debug\n");
    REQUIRE(amuse_train_attn_fwd(A, 2, 8, 0.1f, seed, 23, Bm, C, D, s1) == 0);
    printf("== attn_bwd\n");
    REQUIRE(amuse_train_attn_bwd(A, Bm, C, D, 4, 300, 0.1f, seed, 22, E, s1) == 0);
    REQUIRE(amuse_train_attn_bwd(A, Bm, C, D, 2, 8, 0.1f, seed, 21, E, nullptr) == 0);
    printf("== attn refusals\n");
    REQUIRE(amuse_train_attn_fwd(A, 2, 305, 0.1f, seed, 21, Bm, C, nullptr, s1) == AMUSE_EINVAL);
    REQUIRE(amuse_train_attn_bwd(A, Bm, C, D, 2, 8, 0.1f, seed, 21, nullptr, s1) == AMUSE_EINVAL);

    // ---- optimizer and epoch
    printf("== adamw\n");
    REQUIRE(amuse_train_adamw(A, Bm, C, D, 1000003, 1e-4, 0.9, 0.999, 1e-8, 0.01, 7, s1) == 0);
    REQUIRE(amuse_train_adamw(A, Bm, C, D, 100000000, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1, nullptr) == 0);
    printf("== adamw_dev advance=0\n");
    REQUIRE(amuse_train_adamw_dev(A, Bm, C, D, 1000003, 1e-4, 0.9, 0.999, 1e-8, 0.01, (long*)E, F, 0, s1) == 0);
    printf("== adamw_dev advance=1\n");
    REQUIRE(amuse_train_adamw_dev(A, Bm, C, D, 1000003, 1e-4, 0.9, 0.999, 1e-8, 0.01, (long*)E, F, 1, s1) == 0);
    printf("== epoch advance and set\n");
    REQUIRE(amuse_train_epoch_advance(1, s1) == 0);
    REQUIRE(amuse_train_epoch_set(5, nullptr) == 0);
    REQUIRE(amuse_train_adamw(A, Bm, C, D, 1000, 1e-4, 0.9, 0.999, 1e-8, 0.01, 0, s1) == AMUSE_EINVAL);

    // ---- the layer sequences
    Layer enc_small("enc906", 3, 302, 512, false, false), enc_self("enc1200", 4, 300, 512, false, true), dec_small("dec900", 3, 300, 512, true, false);
    Layer dec_self("dec1200", 4, 300, 512, true, true), enc_tiny("enc160", 32, 5, 1024, false, true);
    if (layer_both("encoder layer rows=906", enc_small.L, s1)) return 1;
    if (layer_both("encoder layer rows=1200 Win", enc_self.L, s1)) return 1;
    if (layer_both("encoder layer rows=160 Win ff=1024", enc_tiny.L, nullptr)) return 1;
    if (layer_both("decoder layer rows=900", dec_small.L, s1)) return 1;
    if (layer_both("decoder layer rows=1200 Win first", dec_self.L, s1)) return 1;
    if (layer_both("decoder layer rows=1200 Win again", dec_self.L, s1)) return 1;
    REQUIRE(amuse_train_set_lane(1) == 0);
    if (layer_both("decoder layer rows=1200 Win lane 1", dec_self.L, s1)) return 1;
    REQUIRE(amuse_train_set_lane(0) == 0);
    if (layer_both("decoder layer rows=1200 Win lane 0 again", dec_self.L, nullptr)) return 1;
    printf("== layer refusals\n");
    {
        amuse_train_layer L = dec_small.L;
        L.H = 3;
        REQUIRE(amuse_train_layer_fwd(&L, s1) == AMUSE_EINVAL);
        L = dec_small.L;
        L.dWc = nullptr;
        REQUIRE(amuse_train_layer_bwd(&L, s1) == AMUSE_EINVAL);
        L = dec_small.L;
        L.p = -0.5f;
        REQUIRE(amuse_train_layer_bwd(&L, s1) == AMUSE_EINVAL);
        REQUIRE(amuse_train_layer_fwd(nullptr, s1) == AMUSE_EINVAL);
    }
    printf("-- end of the golden's sections\n");
    if (mode == "sections" || mode == "overflow") amuse_stub_stream_destroy(s1);
    if (mode == "sections") return 0;
    if (mode == "overflow") {   // where the sources at hand refuse the layer that overflows the weight-gradient workspace: runtime calls and launches issued, return code
        Layer big("dec12288", 48, 256, 960, true, false);
        int ret = 0;
        const long n = steps_of(amuse_train_layer_bwd, big.L, s1, &ret);
        printf("-- overflow: %ld runtime calls and launches issued, returned %d\n", n, ret);
        return 0;
    }

    // ---- refused calls launch nothing and make no runtime call
    int ret = 0;
    {
        amuse_train_layer L = dec_self.L;
        L.dqkv = nullptr;
        REQUIRE(steps_of(amuse_train_layer_bwd, L, s1, &ret) == 0 && ret == AMUSE_EINVAL);
        L = dec_self.L;
        L.lse = nullptr;
        REQUIRE(steps_of(amuse_train_layer_fwd, L, s1, &ret) == 0 && ret == AMUSE_EINVAL);
        REQUIRE(steps_of(amuse_train_layer_bwd, L, s1, &ret) == 0 && ret == AMUSE_EINVAL);
        // the weight-gradient partials of a decoder layer with ff = 960 are 2 x 960 x 128 + 2 x 128 x 128 = 278,528 floats per 192-row chunk: 60 chunks
        // (11,520 rows) fit the workspace's 16,777,216 floats, 61 do not, and neither do the 64 of 12,288 rows
        Layer big("dec12288", 48, 256, 960, true, false), over("dec11712", 48, 244, 960, true, false), fits("dec11520", 48, 240, 960, true, false);
        REQUIRE(steps_of(amuse_train_layer_bwd, big.L, s1, &ret) == 0 && ret == AMUSE_EINVAL);
        REQUIRE(steps_of(amuse_train_layer_bwd, over.L, s1, &ret) == 0 && ret == AMUSE_EINVAL);
        REQUIRE(steps_of(amuse_train_layer_bwd, fits.L, s1, &ret) > 0 && ret == 0);
    }
    // ---- every failure between fork and join of the decoder layer with >= 1,024 rows: the call returns an error, launches nothing more, and has joined
    {
        std::vector<std::string> clean;
        amuse_stub_capture(&clean);
        REQUIRE(amuse_train_layer_bwd(&dec_self.L, s1) == 0);
        amuse_stub_capture(nullptr);
        auto starts = [](const std::string& l, const char* w) { return l.rfind(w, 0) == 0; };
        size_t fork = 0, join = 0;   // 1-based: the fork's wait, the join's record
        for (size_t i = 0; i < clean.size(); ++i) {
            if (starts(clean[i], "hipStreamWaitEvent") && !fork) fork = i + 1;
            if (starts(clean[i], "hipEventRecord")) join = i + 1;
        }
        REQUIRE(fork > 0 && join > fork + 10 && join + 2 == clean.size() && starts(clean[join], "hipStreamWaitEvent") && starts(clean[join + 1], "launch"));
        for (size_t n = fork + 1; n < join; ++n) {
            std::vector<std::string> got;
            amuse_stub_capture(&got);
            amuse_stub_fail_at((long)n);
            ret = amuse_train_layer_bwd(&dec_self.L, s1);
            amuse_stub_fail_at(0);
            amuse_stub_capture(nullptr);
            REQUIRE(ret != 0);
            size_t at = 0;
            while (at < got.size() && got[at] != "-- injected failure") ++at;
            REQUIRE(at < got.size());
            // behind the failure: the join's two lines as the clean run has them, and no launch
            REQUIRE(got.size() == at + 3 && got[at + 1] == clean[join - 1] && got[at + 2] == clean[join]);
        }
        printf("-- %zu failures between fork and join: all joined\n", join - fork - 1);
    }
    amuse_stub_stream_destroy(s1);
    // what is live now is the per-device training state, which the library keeps for the life of the process: the epoch word, per lane the weight-gradient
    // workspace and the side stream with its two events, and lane 0's split-k workspace (lane 1 made no split-k call)
    printf("live allocations at exit: %ld\ntrain_host ok\n", amuse_stub_live_allocations());
    return 0;
}
