// Motion smoothing: the two C entry points (include/amuse_hip.h).  Both are context-free; the bank touches no HIP at all, the filter touches it only after its
// checks, in the launches amuse_smooth_host.hpp packs.
#include "amuse_smooth_host.hpp"

extern "C" {

int amuse_smooth_banks(int order, float* banks_out_host) { return amuse::smooth_banks(order, banks_out_host); }

int amuse_smooth_motion(const float* poses, const float* trans, int S, const int* frames, const unsigned char* half_window, const float* banks_dev, float* poses_out,
                        float* trans_out, void* stream) {
    return amuse::smooth_motion(poses, trans, S, frames, half_window, banks_dev, poses_out, trans_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
