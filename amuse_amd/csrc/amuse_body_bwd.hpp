// Launch interface of the body model's backward kernels (k_body_bwd.hip), called by amuse_body_grad.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amuse {

constexpr int kBodyDAStride = 664;      // per frame of a partial: 55 x 12 dA values | 3 translation sums | pad
constexpr int kBodyDpfFloats = 8192;    // per workgroup: [32 feature tiles][64 lanes][4] = the accumulator image, feature 16 ft + 4 (lane >> 4) + r at frame lane & 15
constexpr int kBodyDpShift = 10;        // dp is scaled by 2^10 before it is cut into fp16 pieces (|dp| <= sqrt 3: the hi piece stays below 2^11, the lo piece normal)
constexpr int kBodyFixShift = 38;       // dA and the translation sums accumulate as value x 2^38 in int64 (capacity 2^25 per sum)

// the hot kernel: the forward pass of the reference and ONE candidate recomputed per (vertex-group pair x 16-frame tile), then g, dp, dA, the transposed product
struct BodySkinBwdArgs {
    const uint16_t *pd_hi, *pd_lo;                // packed posedirs planes (forward image)
    const uint16_t *pt_hi, *pt_lo;                // the transposed image (amuse_body_pack.hpp pack_posedirs_t)
    float scale_inv;                              // 2^-shift
    const void* skin; int nnz;
    const float* v_shaped;
    const int* subject; int n_subjects;
    int V, groups, pairs, nframes, F, chunks;
    const float* A[2]; const float* tr[2];        // 0: the reference, 1: the candidate
    const uint16_t* pf_hi[2]; const uint16_t* pf_lo[2];
    float* dA_part;                               // [tiles * chunks][16][kBodyDAStride]
    float* dpf_part;                              // [tiles * chunks][kBodyDpfFloats], still scaled by 2^(shift + kBodyDpShift)
};
hipError_t launch_body_skin_bwd(const BodySkinBwdArgs& a, int split, hipStream_t st);

// per-frame kernel: chunk partials summed in index order, dA -> dG, the chain in reverse, + dpf, Gram-Schmidt backward, grad row written
struct BodyPoseBwdArgs {
    const float* rows;                            // the candidate's feature rows [nframes][333]
    const int* subject; int n_subjects;
    const float* J;                               // [subjects][55][4]
    signed char parents[56];
    int nframes, F, chunks;
    const float* A;                               // the candidate's skinning transforms [frames16][55][12] (their rotation part is G_j.R)
    const float* dA_part; const float* dpf_part;
    float dpf_scale;                              // 2^-(shift + kBodyDpShift)
    float scale;                                  // the caller's factor on the whole row
    float* grad;                                  // [nframes][333]
};
hipError_t launch_body_pose_bwd(const BodyPoseBwdArgs& a, hipStream_t st);

}  // namespace amuse
