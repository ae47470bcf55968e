// Launch interface of the body-model kernels (k_body.hip), called by amuse_body.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amuse {

constexpr int kBodyMaxSets = 3;
constexpr int kBodyAFloats = 55 * 12;   // skinning transforms of a frame: [55][3 rows][R | t]

// per-frame kernel: rotations -> pose-feature planes, the kinematic chain, skinning transforms, posed joints
struct BodyPoseArgs {
    const float* rot; const float* trans;         // rows of rot_stride / trans_stride floats per frame; trans nullable (zero)
    int rot_stride, trans_stride, rot_kind;       // rot_kind 0: 55 x 3 axis-angle, 1: 55 x 6D
    const int* subject; int n_subjects;           // device [N]; outside 0..n_subjects-1: the clip is skipped
    const float* J;                               // [subjects][55][4]
    signed char parents[56];
    int nframes, F;                               // frames of the call (the grid covers them rounded up to 16: pad frames get zero features)
    float* A;                                     // [frames16][55][12]
    float* tr;                                    // [frames16][4]
    uint16_t *pf_hi, *pf_lo;                      // [frames16 / 16][16 k-steps][64 lanes][8]: the B operand of the pose-blend product, fragment order
    float* joints_out;                            // [nframes][55][3] or null
};
hipError_t launch_body_pose(const BodyPoseArgs& a, hipStream_t st);

// the hot kernel: (vertex group x 16-frame tile) pose-blend MFMA, skinning in-lane, then either the vertices or the SmoothL1 partial sums
struct BodySkinArgs {
    const uint16_t *pd_hi, *pd_lo;                // packed posedirs planes (amuse_body_pack.hpp)
    float scale_inv;                              // 2^-shift
    const void* skin; int nnz;                    // [groups * 4][nnz] (int32 joint, float weight)
    const float* v_shaped;                        // [subjects][groups * 4][4]
    const int* subject; int n_subjects;
    int V, groups, nframes, F, nsets, chunks;
    const float* A[kBodyMaxSets]; const float* tr[kBodyMaxSets];
    const uint16_t* pf_hi[kBodyMaxSets]; const uint16_t* pf_lo[kBodyMaxSets];
    float* vertices_out;                          // forward: [nframes][V][3]
    float* partials;                              // loss: [tiles * chunks][2]
};
hipError_t launch_body_skin(const BodySkinArgs& a, int split, int loss, hipStream_t st);
// sums_out[0..1] = the partials' columns added up in index order in double (column 1 = 0 when nsets == 2)
hipError_t launch_body_loss_reduce(const float* partials, int n, int nsets, double* sums_out, hipStream_t st);

}  // namespace amuse
