// Long-form inference: the two C entry points (include/amuse_hip.h).  Both are context-free; the window plan touches no HIP at all, the join touches it only
// after its checks, in the launches amuse_stitch_host.hpp packs.
#include "amuse_stitch_host.hpp"

extern "C" {

int amuse_longform_plan(long long n_samples, int hop_frames, int* windows, int* frames, int* hop_samples) {
    return amuse::longform_plan(n_samples, hop_frames, windows, frames, hop_samples);
}

int amuse_stitch_windows(const float* poses, const float* trans, int S, const int* windows, const int* frames, int F, int hop, const float* blend, float* poses_out,
                         float* trans_out, void* stream) {
    return amuse::stitch_windows(poses, trans, S, windows, frames, F, hop, blend, poses_out, trans_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
