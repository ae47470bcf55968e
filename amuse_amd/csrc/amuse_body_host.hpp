// Shared by the two host translation units of the body model (amuse_body.hip: context, packing, workspace, forward calls; amuse_body_grad.hip: the gradient
// calls): the context, the error slot and the HIP call wrapper.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_seq_host.hpp"
#define fail(...) amuse_failf(__VA_ARGS__)
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(AMUSE_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct amuse_body_ctx {
    int device = 0;
    int V = 0, groups = 0, n_betas = 0, nnz = 0, shift = 0, S = 0;
    std::vector<float> v_template, shapedirs, Jreg;   // host copies for amuse_body_set_subjects
    signed char parents[56];
    uint16_t *pd_hi = nullptr, *pd_lo = nullptr;
    void* skin = nullptr;
    float *v_shaped = nullptr, *J = nullptr;
    // workspace for `cap` frames (a multiple of 16) x kBodyMaxSets motion sets
    size_t cap = 0;
    float *A = nullptr, *tr = nullptr, *partials = nullptr;
    uint16_t* pf = nullptr;   // [sets][hi | lo][cap * 512]
    std::vector<void*> retired;   // workspaces outgrown by a later call: kept until destroy, a graph captured earlier still replays into them
    // gradients (amuse_body_enable_grad): the transposed posedirs image and the partials of the backward kernels, sized with the workspace
    int grad = 0;
    uint16_t *pt_hi = nullptr, *pt_lo = nullptr;
    float *dA_part = nullptr, *dpf_part = nullptr;
    size_t gcap = 0;              // frames the partials are sized for (0 until gradients are enabled)
};

// amuse_body.hip: sizes the workspace (and, once gradients are enabled, the backward partials) for `frames` frames; never frees what a graph may replay into
int amuse_body_reserve_ws(amuse_body_ctx* c, size_t frames);
// amuse_body.hip: the argument checks every compute call shares; the forward pose kernel on 6D feature rows into workspace slice s
int amuse_body_check_call(const amuse_body_ctx* c, const int* subject_dev, int N, int F, int precision, int rot_kind);
int amuse_body_pose_rows6d(const amuse_body_ctx* c, int s, const float* rows, const int* subject_dev, int nframes, int F, void* stream);


