// Host side of the SMPL-X body model (include/amuse_hip.h amuse_body_*): context, packing (amuse_body_pack.hpp), workspace, argument checks, launch order.
// A translation unit of its own: nothing here is referenced from amuse_api.hip / amuse_audio_api.hip, and it needs only the error slot of the C ABI.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/amuse_hip.h"
#include "amuse_body.hpp"
#include "amuse_body_pack.hpp"
#include "amuse_body_bwd.hpp"
#include "amuse_body_host.hpp"

using namespace amuse;
namespace ab = amuse_body;

namespace {
void retire_ws(amuse_body_ctx* c) {
    for (void* p : {(void*)c->A, (void*)c->tr, (void*)c->partials, (void*)c->pf})
        if (p) c->retired.push_back(p);
    c->A = c->tr = c->partials = nullptr;
    c->pf = nullptr;
    c->cap = 0;
}
int reserve_grad(amuse_body_ctx* c, size_t need) {   // the backward partials: tiles * bwd_chunks(tiles) <= tiles + 512 workgroups
    if (!c->grad || need <= c->gcap) return 0;
    for (void* p : {(void*)c->dA_part, (void*)c->dpf_part})
        if (p) c->retired.push_back(p);
    c->dA_part = c->dpf_part = nullptr;
    c->gcap = 0;
    const size_t wgs = ab::bwd_partial_workgroups(need);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc((void**)&c->dA_part, wgs * 16 * kBodyDAStride * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->dpf_part, wgs * kBodyDpfFloats * sizeof(float)));
    c->gcap = need;
    return 0;
}
int reserve(amuse_body_ctx* c, size_t frames) {
    const size_t need = (frames + 15) / 16 * 16;
    if (need > c->cap) {
        retire_ws(c);
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMalloc((void**)&c->A, kBodyMaxSets * need * kBodyAFloats * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&c->tr, kBodyMaxSets * need * 4 * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&c->pf, kBodyMaxSets * 2 * need * ab::kPoseK * sizeof(uint16_t)));
        HIP_TRY(hipMalloc((void**)&c->partials, (need / 16 + 1025) * 2 * sizeof(float)));   // tiles * skin_chunks(tiles) <= tiles + 1024
        c->cap = need;
    }
    return reserve_grad(c, c->cap);
}
struct SetPtrs { float *A, *tr; uint16_t *pf_hi, *pf_lo; };
SetPtrs set_ptrs(const amuse_body_ctx* c, int s) {
    return {c->A + (size_t)s * c->cap * kBodyAFloats, c->tr + (size_t)s * c->cap * 4, c->pf + (size_t)(2 * s) * c->cap * ab::kPoseK,
            c->pf + (size_t)(2 * s + 1) * c->cap * ab::kPoseK};
}
int check_call(const amuse_body_ctx* c, const int* subject_dev, int N, int F, int precision, int rot_kind) {
    if (!c) return fail(AMUSE_EINVAL, "amuse_body: NULL context");
    if (!subject_dev || N < 1 || F < 1) return fail(AMUSE_EINVAL, "amuse_body: subject_dev NULL or N / F < 1 (N %d, F %d)", N, F);
    if ((size_t)N * (size_t)F > (size_t)0x7fffff00u) return fail(AMUSE_EINVAL, "amuse_body: N * F = %zu frames exceed 2^31", (size_t)N * (size_t)F);
    if (precision != AMUSE_PREC_F32X && precision != AMUSE_PREC_F16) return fail(AMUSE_EINVAL, "amuse_body: precision %d (AMUSE_PREC_F32X or AMUSE_PREC_F16)", precision);
    if (rot_kind != AMUSE_BODY_ROT_AA && rot_kind != AMUSE_BODY_ROT_6D) return fail(AMUSE_EINVAL, "amuse_body: rot_kind %d", rot_kind);
    if (c->S < 1) return fail(AMUSE_ESTATE, "amuse_body: no subjects set (amuse_body_set_subjects)");
    return 0;
}
int pose_set(const amuse_body_ctx* c, int s, const float* rot, int rot_stride, const float* trans, int trans_stride, int rot_kind, const int* subject_dev, int nframes,
             int F, float* joints_out, hipStream_t st) {
    const SetPtrs p = set_ptrs(c, s);
    BodyPoseArgs a;
    a.rot = rot; a.trans = trans; a.rot_stride = rot_stride; a.trans_stride = trans_stride; a.rot_kind = rot_kind;
    a.subject = subject_dev; a.n_subjects = c->S; a.J = c->J;
    memcpy(a.parents, c->parents, sizeof(a.parents));
    a.nframes = nframes; a.F = F; a.A = p.A; a.tr = p.tr; a.pf_hi = p.pf_hi; a.pf_lo = p.pf_lo; a.joints_out = joints_out;
    HIP_TRY(launch_body_pose(a, st));
    return 0;
}
void skin_args(const amuse_body_ctx* c, BodySkinArgs& a, const int* subject_dev, int nframes, int F, int nsets) {
    a.pd_hi = c->pd_hi; a.pd_lo = c->pd_lo; a.scale_inv = ldexpf(1.f, -c->shift);
    a.skin = c->skin; a.nnz = c->nnz; a.v_shaped = c->v_shaped; a.subject = subject_dev; a.n_subjects = c->S;
    a.V = c->V; a.groups = c->groups; a.nframes = nframes; a.F = F; a.nsets = nsets;
    a.chunks = ab::skin_chunks((nframes + 15) / 16, c->groups);
    for (int s = 0; s < kBodyMaxSets; ++s) {
        const SetPtrs p = set_ptrs(c, s < nsets ? s : 0);
        a.A[s] = p.A; a.tr[s] = p.tr; a.pf_hi[s] = p.pf_hi; a.pf_lo[s] = p.pf_lo;
    }
    a.vertices_out = nullptr; a.partials = c->partials;
}
}  // namespace

int amuse_body_reserve_ws(amuse_body_ctx* c, size_t frames) { return reserve(c, frames); }
int amuse_body_check_call(const amuse_body_ctx* c, const int* subject_dev, int N, int F, int precision, int rot_kind) { return check_call(c, subject_dev, N, F, precision, rot_kind); }
int amuse_body_pose_rows6d(const amuse_body_ctx* c, int s, const float* rows, const int* subject_dev, int nframes, int F, void* stream) {
    return pose_set(c, s, rows, 333, rows + 330, 333, AMUSE_BODY_ROT_6D, subject_dev, nframes, F, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" {

amuse_body_ctx* amuse_body_create(int device, const amuse_body_model* m) {
    if (!m || m->V < 1 || m->n_betas < 0 || !m->v_template || (m->n_betas && !m->shapedirs) || !m->posedirs || !m->J_regressor || !m->weights || !m->parents) {
        fail(AMUSE_EINVAL, "amuse_body_create: NULL model array or V < 1");
        return nullptr;
    }
    if (m->V > (1 << 26)) { fail(AMUSE_EINVAL, "amuse_body_create: V %d too large", m->V); return nullptr; }
    if (!ab::parents_valid(m->parents)) {
        fail(AMUSE_EINVAL, "amuse_body_create: parents must have parents[0] = -1 and 0 <= parents[j] < j");
        return nullptr;
    }
    amuse_body_ctx* c = new amuse_body_ctx();
    c->device = device; c->V = m->V; c->n_betas = m->n_betas; c->groups = ab::vertex_groups(m->V);
    const size_t nv3 = (size_t)m->V * 3;
    c->v_template.assign(m->v_template, m->v_template + nv3);
    if (m->n_betas) c->shapedirs.assign(m->shapedirs, m->shapedirs + nv3 * m->n_betas);
    c->Jreg.assign(m->J_regressor, m->J_regressor + (size_t)ab::kJoints * m->V);
    memset(c->parents, 0, sizeof(c->parents));
    for (int j = 0; j < ab::kJoints; ++j) c->parents[j] = (signed char)m->parents[j];
    std::vector<uint16_t> hi, lo;
    c->shift = ab::posedirs_shift(m->posedirs, (size_t)ab::kPoseFeat * nv3);
    ab::pack_posedirs(m->posedirs, m->V, c->shift, hi, lo);
    std::vector<ab::SkinEntry> skin;
    c->nnz = ab::pack_skin(m->weights, m->V, skin);
    auto up = [&](void** dst, const void* src, size_t bytes) -> int {
        HIP_TRY(hipMalloc(dst, bytes));
        HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    auto build = [&]() -> int {   // (every failure site leaves its own message)
        HIP_TRY(hipSetDevice(device));
        if (int e = up((void**)&c->pd_hi, hi.data(), hi.size() * 2)) return e;
        if (int e = up((void**)&c->pd_lo, lo.data(), lo.size() * 2)) return e;
        return up(&c->skin, skin.data(), skin.size() * sizeof(ab::SkinEntry));
    };
    if (build()) {
        amuse_body_destroy(c);
        return nullptr;
    }
    return c;
}

void amuse_body_destroy(amuse_body_ctx* c) {
    if (!c) return;
    retire_ws(c);
    for (void* p : c->retired) (void)hipFree(p);
    for (void* p : {(void*)c->pd_hi, (void*)c->pd_lo, c->skin, (void*)c->v_shaped, (void*)c->J, (void*)c->pt_hi, (void*)c->pt_lo, (void*)c->dA_part, (void*)c->dpf_part})
        if (p) (void)hipFree(p);
    delete c;
}

int amuse_body_set_subjects(amuse_body_ctx* c, const float* betas, int S) {
    if (!c || S < 1 || (c->n_betas && !betas)) return fail(AMUSE_EINVAL, "amuse_body_set_subjects: NULL argument or S < 1");
    const size_t vs_n = (size_t)c->groups * 16, j_n = (size_t)ab::kJoints * 4;
    std::vector<float> vs(vs_n * S), J(j_n * S);
    for (int s = 0; s < S; ++s)
        ab::shape_subject(c->V, c->n_betas, c->v_template.data(), c->shapedirs.data(), c->Jreg.data(), betas + (size_t)s * c->n_betas, vs.data() + vs_n * s, J.data() + j_n * s);
    HIP_TRY(hipSetDevice(c->device));
    if (S != c->S) {
        if (c->v_shaped) HIP_TRY(hipFree(c->v_shaped));
        if (c->J) HIP_TRY(hipFree(c->J));
        c->v_shaped = c->J = nullptr;
        c->S = 0;
        HIP_TRY(hipMalloc((void**)&c->v_shaped, vs.size() * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&c->J, J.size() * sizeof(float)));
    }
    HIP_TRY(hipMemcpy(c->v_shaped, vs.data(), vs.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->J, J.data(), J.size() * sizeof(float), hipMemcpyHostToDevice));
    c->S = S;
    return 0;
}

int amuse_body_reserve(amuse_body_ctx* c, size_t frames) {
    if (!c || frames < 1 || frames > (size_t)0x7fffff00u) return fail(AMUSE_EINVAL, "amuse_body_reserve: NULL context or bad frame count");
    return reserve(c, frames);
}

int amuse_body_forward(amuse_body_ctx* c, const float* rot, int rot_kind, const float* trans, const int* subject_dev, int N, int F, int precision, float* joints_out,
                       float* vertices_out, void* stream) {
    if (int e = check_call(c, subject_dev, N, F, precision, rot_kind)) return e;
    if (!rot) return fail(AMUSE_EINVAL, "amuse_body_forward: rot is NULL");
    if (!joints_out && !vertices_out) return fail(AMUSE_EINVAL, "amuse_body_forward: both outputs are NULL");
    const int nframes = N * F;
    if (int e = reserve(c, (size_t)nframes)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool d6 = rot_kind == AMUSE_BODY_ROT_6D;
    if (int e = pose_set(c, 0, rot, d6 ? 333 : 165, d6 ? rot + 330 : trans, d6 ? 333 : 3, rot_kind, subject_dev, nframes, F, joints_out, st)) return e;
    if (vertices_out) {
        BodySkinArgs a;
        skin_args(c, a, subject_dev, nframes, F, 1);
        a.vertices_out = vertices_out;
        HIP_TRY(launch_body_skin(a, precision == AMUSE_PREC_F32X, 0, st));
    }
    return 0;
}

int amuse_body_vertex_loss(amuse_body_ctx* c, const float* ref, const float* x, const float* y, int rot_kind, const int* subject_dev, int N, int F, int precision,
                           double* sums_out, void* stream) {
    if (int e = check_call(c, subject_dev, N, F, precision, rot_kind)) return e;
    if (!ref || !x || !sums_out) return fail(AMUSE_EINVAL, "amuse_body_vertex_loss: ref, a or sums_out is NULL");
    const int nframes = N * F, nsets = y ? 3 : 2;
    if (int e = reserve(c, (size_t)nframes)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int stride = rot_kind == AMUSE_BODY_ROT_6D ? 333 : 168;
    const float* sets[3] = {ref, x, y};
    for (int s = 0; s < nsets; ++s)
        if (int e = pose_set(c, s, sets[s], stride, sets[s] + stride - 3, stride, rot_kind, subject_dev, nframes, F, nullptr, st)) return e;
    BodySkinArgs a;
    skin_args(c, a, subject_dev, nframes, F, nsets);
    HIP_TRY(launch_body_skin(a, precision == AMUSE_PREC_F32X, 1, st));
    HIP_TRY(launch_body_loss_reduce(c->partials, (nframes + 15) / 16 * a.chunks, nsets, sums_out, st));
    return 0;
}

int amuse_body_info(const amuse_body_ctx* c, int what) {
    if (!c) return fail(AMUSE_EINVAL, "amuse_body_info: NULL context");
    switch (what) {
        case 0: return c->V;
        case 1: return c->nnz;
        case 2: return c->shift;
        case 3: return c->S;
        case 4: return c->grad;
        default: return fail(AMUSE_EINVAL, "amuse_body_info: what %d", what);
    }
}

}  // extern "C"
