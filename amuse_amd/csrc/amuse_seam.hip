// Long-form candidates: the four C entry points (include/amuse_hip.h).  All are context-free; the plan touches no HIP at all, the others touch it only after
// their checks, in the launches amuse_seam_host.hpp packs.
#include "amuse_seam_host.hpp"

extern "C" {

int amuse_seam_plan(int S, const int* windows, int K, int F, int hop, long long* seams, size_t* workspace_bytes) {
    return amuse::seam_plan(S, windows, K, F, hop, seams, workspace_bytes);
}

int amuse_seam_cost(const float* poses, const float* trans, int S, const int* windows, const int* frames, int K, int F, int hop, const float* row_weight,
                    const float* joint_weight, float trans_weight, void* workspace, double* cost_out, void* stream) {
    return amuse::seam_cost(poses, trans, S, windows, frames, K, F, hop, row_weight, joint_weight, trans_weight, workspace, cost_out, static_cast<hipStream_t>(stream));
}

int amuse_seam_path(const double* cost, int S, const int* windows, int K, int* choice_out, double* total_out, void* stream) {
    return amuse::seam_path(cost, S, windows, K, choice_out, total_out, static_cast<hipStream_t>(stream));
}

int amuse_seam_select(const float* poses, const float* trans, const int* choice, int n, int n_in, int F, float* poses_out, float* trans_out, void* stream) {
    return amuse::seam_select(poses, trans, choice, n, n_in, F, poses_out, trans_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
