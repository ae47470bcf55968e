// Host side of the body model's gradient calls (include/amuse_hip.h amuse_body_enable_grad / amuse_body_vertex_loss_grad): the transposed posedirs image, the
// argument checks and the launch order of k_body_bwd.hip.  A translation unit of its own beside amuse_body.hip, which keeps the context and the workspace.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_body.hpp"
#include "amuse_body_bwd.hpp"
#include "amuse_body_host.hpp"
#include "amuse_body_pack.hpp"

using namespace amuse;
namespace ab = amuse_body;

extern "C" {

int amuse_body_enable_grad(amuse_body_ctx* c) {
    if (!c) return fail(AMUSE_EINVAL, "amuse_body_enable_grad: NULL context");
    if (c->grad) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // the forward planes come back from the device and are re-ordered: the same halfs, and no dense host copy of posedirs is kept for a call most contexts never make
    const size_t nf = ab::posedirs_plane_halfs(c->V), nt = ab::posedirs_t_plane_halfs(c->V);
    std::vector<uint16_t> fwd(nf), img;
    uint16_t* dst[2] = {nullptr, nullptr};
    const uint16_t* src[2] = {c->pd_hi, c->pd_lo};
    for (int p = 0; p < 2; ++p) {
        hipError_t e = hipMemcpy(fwd.data(), src[p], nf * sizeof(uint16_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
            ab::transpose_posedirs_plane(fwd.data(), c->V, img);
            e = hipMalloc((void**)&dst[p], nt * sizeof(uint16_t));
        }
        if (e == hipSuccess) e = hipMemcpy(dst[p], img.data(), nt * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            for (uint16_t* d : dst)
                if (d) (void)hipFree(d);
            return fail(AMUSE_EHIP, "amuse_body_enable_grad: %s", hipGetErrorString(e));
        }
    }
    c->pt_hi = dst[0];
    c->pt_lo = dst[1];
    c->grad = 1;
    return c->cap ? amuse_body_reserve_ws(c, c->cap) : 0;   // a workspace that exists already gets its backward partials now
}

int amuse_body_vertex_loss_grad(amuse_body_ctx* c, const float* ref, const float* x, const float* y, int rot_kind, const int* subject_dev, int N, int F, int precision,
                                float scale_a, float scale_b, float* grad_a, float* grad_b, void* stream) {
    if (int e = amuse_body_check_call(c, subject_dev, N, F, precision, rot_kind)) return e;
    if (rot_kind != AMUSE_BODY_ROT_6D)
        return fail(AMUSE_EINVAL, "amuse_body_vertex_loss_grad: 6D feature rows only (the published Rodrigues form, angle = |r + 1e-8|, has no usable derivative at the zero vector)");
    if (!c->grad) return fail(AMUSE_ESTATE, "amuse_body_vertex_loss_grad: gradients are not enabled (amuse_body_enable_grad)");
    if (!ref || !x || !grad_a) return fail(AMUSE_EINVAL, "amuse_body_vertex_loss_grad: ref, a or grad_a is NULL");
    if ((y == nullptr) != (grad_b == nullptr)) return fail(AMUSE_EINVAL, "amuse_body_vertex_loss_grad: b and grad_b go together");
    const int nframes = N * F, ncand = y ? 2 : 1;
    if (int e = amuse_body_reserve_ws(c, (size_t)nframes)) return e;
    const float* sets[3] = {ref, x, y};
    for (int s = 0; s <= ncand; ++s)
        if (int e = amuse_body_pose_rows6d(c, s, sets[s], subject_dev, nframes, F, stream)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tiles = (nframes + 15) / 16;
    auto slice = [&](int s, const float** A, const float** tr, const uint16_t** hi, const uint16_t** lo) {
        *A = c->A + (size_t)s * c->cap * kBodyAFloats;
        *tr = c->tr + (size_t)s * c->cap * 4;
        *hi = c->pf + (size_t)(2 * s) * c->cap * ab::kPoseK;
        *lo = c->pf + (size_t)(2 * s + 1) * c->cap * ab::kPoseK;
    };
    for (int k = 1; k <= ncand; ++k) {   // one candidate per pass; the partials are re-used, in stream order
        BodySkinBwdArgs a;
        a.pd_hi = c->pd_hi; a.pd_lo = c->pd_lo; a.pt_hi = c->pt_hi; a.pt_lo = c->pt_lo; a.scale_inv = ldexpf(1.f, -c->shift);
        a.skin = c->skin; a.nnz = c->nnz; a.v_shaped = c->v_shaped; a.subject = subject_dev; a.n_subjects = c->S;
        a.V = c->V; a.groups = c->groups; a.pairs = ab::vertex_pairs(c->V); a.nframes = nframes; a.F = F;
        a.chunks = ab::bwd_chunks(tiles, a.pairs);
        slice(0, &a.A[0], &a.tr[0], &a.pf_hi[0], &a.pf_lo[0]);
        slice(k, &a.A[1], &a.tr[1], &a.pf_hi[1], &a.pf_lo[1]);
        a.dA_part = c->dA_part; a.dpf_part = c->dpf_part;
        HIP_TRY(launch_body_skin_bwd(a, precision == AMUSE_PREC_F32X, st));
        BodyPoseBwdArgs p;
        p.rows = sets[k]; p.subject = subject_dev; p.n_subjects = c->S; p.J = c->J;
        memcpy(p.parents, c->parents, sizeof(p.parents));
        p.nframes = nframes; p.F = F; p.chunks = a.chunks; p.A = a.A[1]; p.dA_part = c->dA_part; p.dpf_part = c->dpf_part;
        p.dpf_scale = ldexpf(1.f, -(c->shift + kBodyDpShift)); p.scale = k == 1 ? scale_a : scale_b; p.grad = k == 1 ? grad_a : grad_b;
        HIP_TRY(launch_body_pose_bwd(p, st));
    }
    return 0;
}

}  // extern "C"
