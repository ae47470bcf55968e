// Beat alignment: the C entry points (include/amuse_hip.h).  Every call touches HIP only after its checks, through amuse_beat_host.hpp; the only call that
// allocates after amuse_beat_create is amuse_beat_reserve.
#include "amuse_beat_host.hpp"

extern "C" {

int amuse_beat_default_params(amuse_beat_params* params) { return amuse::beat_default_params(params); }

amuse_beat* amuse_beat_create(int device, const float* mel_banks, const float* window) {
    return reinterpret_cast<amuse_beat*>(amuse::beat_create(device, mel_banks, window));   // (the opaque handle IS the host struct)
}

void amuse_beat_destroy(amuse_beat* ctx) { amuse::beat_destroy(reinterpret_cast<amuse::Beat*>(ctx)); }

int amuse_beat_plan(long long n_samples, int* frames) { return amuse::beat_plan(n_samples, frames); }

int amuse_beat_reserve(amuse_beat* ctx, int B, int n_samples) { return amuse::beat_reserve(reinterpret_cast<amuse::Beat*>(ctx), B, n_samples); }

int amuse_beat_onsets(amuse_beat* ctx, const float* waves_dev, const int* n_valid_dev, int n_samples, int B, const amuse_beat_params* params,
                      float* envelope_out, unsigned char* onset_mask_out, void* stream) {
    return amuse::beat_onsets(reinterpret_cast<amuse::Beat*>(ctx), waves_dev, n_valid_dev, n_samples, B, params, envelope_out, onset_mask_out, static_cast<hipStream_t>(stream));
}

int amuse_beat_pick(const float* envelope_dev, const int* frames_dev, int B, int T, const amuse_beat_params* params, unsigned char* onset_mask_out, void* stream) {
    return amuse::beat_pick(envelope_dev, frames_dev, B, T, params, onset_mask_out, static_cast<hipStream_t>(stream));
}

int amuse_beat_align_row(void) { return amuse::kBeatRow; }

int amuse_beat_align(const unsigned char* onset_mask_dev, const int* audio_frames_dev, int T, const float* joints, const int* lengths_dev, int N, int F,
                     const amuse_beat_params* params, double* rows_out, unsigned char* beat_mask_out, void* stream) {
    return amuse::beat_align(onset_mask_dev, audio_frames_dev, T, joints, lengths_dev, N, F, params, rows_out, beat_mask_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
