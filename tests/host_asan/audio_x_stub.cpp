// Stand-ins for the five launchers of the audio front-end's parity mode (csrc/amuse_audio_x.hpp), beside hip_stub.cpp: with amuse_audio_x.o linked, the
// host code of AMUSE_PREC_F32X runs under ASan / UBSan without a GPU and prints its launches into the launch log (amuse_stub_log(2), struct Line of
// stub_log.hpp; GemmXArgs::W and the head's Wt also by image digest).  Linked into tests/host_asan/audio_launch_args.cpp ONLY: the programs of build.sh
// link without it and without amuse_audio_x.o, which is what makes them refuse the mode (tests/test_audio_precision_abi_cpu.py).
#include <hip/hip_runtime.h>

#include "../../amuse_amd/csrc/amuse_audio_x.hpp"
#include "stub_log.hpp"

namespace amuse {
hipError_t launch_gemm_x(const GemmXArgs& a, int epi, hipStream_t st) {
    if (amuse_stub_log_level() == 2)
        Line("launch_gemm_x").i("epi", epi).st(st).P_(A_hi).P_(A_lo).wp("W", a.W).P_(bias).I_(M).I_(N).I_(K).P_(out_hi).P_(out_lo).P_(out_f32).P_(pos).P_(vt_hi).P_(vt_lo);
    return hipSuccess;
}
hipError_t launch_im2col_x(const float* fbank, unsigned short* p_hi, unsigned short* p_lo, int B, hipStream_t st) {
    if (amuse_stub_log_level() == 2) Line("launch_im2col_x").st(st).p("fbank", fbank).p("p_hi", p_hi).p("p_lo", p_lo).i("B", B);
    return hipSuccess;
}
hipError_t launch_ln_x(const float* X, const float* gamma, const float* beta, float eps, unsigned short* out_hi, unsigned short* out_lo, int M, hipStream_t st) {
    if (amuse_stub_log_level() == 2) Line("launch_ln_x").st(st).p("X", X).p("gamma", gamma).p("beta", beta).f("eps", eps).p("out_hi", out_hi).p("out_lo", out_lo).i("M", M);
    return hipSuccess;
}
hipError_t launch_ast_attn_x(const unsigned short* qk_hi, const unsigned short* qk_lo, const unsigned short* vt_hi, const unsigned short* vt_lo, unsigned short* o_hi,
                             unsigned short* o_lo, int B, hipStream_t st) {
    if (amuse_stub_log_level() == 2)
        Line("launch_ast_attn_x").st(st).p("qk_hi", qk_hi).p("qk_lo", qk_lo).p("vt_hi", vt_hi).p("vt_lo", vt_lo).p("o_hi", o_hi).p("o_lo", o_lo).i("B", B);
    return hipSuccess;
}
hipError_t launch_ast_head_x(const float* pooled, int frame_based, const float* gamma, const float* beta, const float* Wt, const float* bias, float* out, int B, hipStream_t st) {
    if (amuse_stub_log_level() == 2)
        Line("launch_ast_head_x").st(st).p("pooled", pooled).i("frame_based", frame_based).p("gamma", gamma).p("beta", beta).wp("Wt", Wt).p("bias", bias).p("out", out).i("B", B);
    return hipSuccess;
}
}  // namespace amuse
