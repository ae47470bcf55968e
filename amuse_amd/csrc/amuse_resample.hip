// Sample-rate conversion: the C entry points (include/amuse_hip.h).  The plan and the bank touch no HIP at all; create uploads the bank; the call touches HIP
// only after its checks, in the one launch amuse_resample_host.hpp makes.
#include "amuse_resample_host.hpp"

extern "C" {

int amuse_resample_plan(int rate_in, int rate_out, long long n_in, int* up, int* down, int* taps, long long* n_out) {
    return amuse::resample_plan(rate_in, rate_out, n_in, up, down, taps, n_out);
}

amuse_resampler* amuse_resampler_create(int device, int rate_in, int rate_out) {
    return reinterpret_cast<amuse_resampler*>(amuse::resampler_create(device, rate_in, rate_out));   // (the opaque handle IS the host struct)
}

void amuse_resampler_destroy(amuse_resampler* r) { amuse::resampler_destroy(reinterpret_cast<amuse::Resampler*>(r)); }

int amuse_resample(amuse_resampler* r, const void* pcm, int format, int channels, long long n_in, float* out, long long out_capacity, void* stream) {
    return amuse::resample_run(reinterpret_cast<const amuse::Resampler*>(r), pcm, format, channels, n_in, out, out_capacity, static_cast<hipStream_t>(stream));
}

int amuse_debug_resample_bank(int rate_in, int rate_out, float* bank_out_host) {
    amuse::ResamplePlan p{};
    if (int rc = amuse::resample_plan_rates(rate_in, rate_out, &p)) return rc;
    if (!bank_out_host) return amuse_failf(AMUSE_EINVAL, "amuse_debug_resample_bank: bank_out_host is NULL");
    amuse::resample_bank(p, bank_out_host);
    return AMUSE_OK;
}

}  // extern "C"
