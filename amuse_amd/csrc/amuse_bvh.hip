// BVH export: the four C entry points (include/amuse_hip.h).  All are context-free; the layout touches no HIP at all, the others touch it only after their checks,
// in the launches amuse_bvh_host.hpp packs.
#include "amuse_bvh_host.hpp"

extern "C" {

int amuse_bvh_layout(const int* parents, int n, int* dfs_out) { return amuse::bvh_layout(parents, n, dfs_out); }

int amuse_bvh_format(const float* values, long long n, int per_row, void* text_out, int* status, void* stream) {
    return amuse::bvh_format(values, n, per_row, static_cast<unsigned char*>(text_out), status, static_cast<hipStream_t>(stream));
}

int amuse_bvh_motion(const float* poses, const float* trans, const float* root_rest, int S, const int* frames, const int* dfs, int order, float scale, int unwrap,
                     float* euler_out, void* text_out, int* status, void* stream) {
    return amuse::bvh_motion(poses, trans, root_rest, S, frames, dfs, order, scale, unwrap, euler_out, static_cast<unsigned char*>(text_out), status,
                             static_cast<hipStream_t>(stream));
}

int amuse_bvh_decode(const float* channels, int S, const int* frames, const int* dfs, int order, float scale, const float* root_rest, float* poses_out,
                     float* trans_out, void* stream) {
    return amuse::bvh_decode(channels, S, frames, dfs, order, scale, root_rest, poses_out, trans_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
