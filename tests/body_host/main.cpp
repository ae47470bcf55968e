// Stand-alone program (its own main): the host half of the SMPL-X body model - csrc/amuse_body_pack.hpp and csrc/amuse_body.hip - under AddressSanitizer /
// UBSan on a machine without a GPU.  The HIP runtime is tests/host_asan/hip_stub.cpp, unchanged ("device" memory is host memory); the three kernel launchers of
// k_body.hip are stand-ins here that keep the argument structs, so the images the library uploaded can be checked element by element against the dense matrices:
//   - the packed posedirs planes (hi + lo reconstruct the pre-scaled entry to 2^-21 relative, hi is rn16 of it, every pad slot is zero)
//   - the per-vertex (joint, weight) lists against the dense rows (order, padding, largest non-zero count)
//   - v_shaped / J of every subject against a double evaluation
//   - parents validation, V not a multiple of 4, argument checks, workspace growth, create / set_subjects / destroy with no allocation left
// tests/test_body_host_asan_cpu.py builds and runs it (tests/build_host_program.sh).  Prints "body_host ok" and returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../amuse_amd/csrc/amuse_body.hpp"
#include "../../amuse_amd/csrc/amuse_body_pack.hpp"
#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();

#include "../host_check.hpp"

static amuse::BodyPoseArgs g_pose[3];
static amuse::BodySkinArgs g_skin;
static int g_npose = 0, g_nskin = 0, g_nreduce = 0, g_split = -1, g_loss = -1, g_reduce_n = 0;
namespace amuse {
hipError_t launch_body_pose(const BodyPoseArgs& a, hipStream_t) { g_pose[g_npose++ % 3] = a; return hipSuccess; }
hipError_t launch_body_skin(const BodySkinArgs& a, int split, int loss, hipStream_t) { g_skin = a; ++g_nskin; g_split = split; g_loss = loss; return hipSuccess; }
hipError_t launch_body_loss_reduce(const float*, int n, int, double*, hipStream_t) { ++g_nreduce; g_reduce_n = n; return hipSuccess; }
}  // namespace amuse

namespace ab = amuse_body;

struct Model {
    int V, nb;
    std::vector<float> vt, sd, pd, jr, w;
    std::vector<int> parents;
    amuse_body_model c() const { return {V, nb, vt.data(), sd.data(), pd.data(), jr.data(), w.data(), parents.data()}; }
};
static Model make(int V, int nb, unsigned seed) {
    std::mt19937 g(seed);
    std::uniform_real_distribution<float> u(-1.f, 1.f), e(-7.f, -2.f);
    Model m;
    m.V = V; m.nb = nb;
    m.vt.resize((size_t)V * 3); m.sd.resize((size_t)V * 3 * nb); m.pd.resize((size_t)486 * V * 3); m.jr.assign((size_t)55 * V, 0.f); m.w.assign((size_t)V * 55, 0.f);
    for (auto& x : m.vt) x = u(g);
    for (auto& x : m.sd) x = 2e-3f * u(g);
    for (auto& x : m.pd) x = (u(g) < 0 ? -1.f : 1.f) * powf(10.f, e(g));
    for (int j = 0; j < 55; ++j)
        for (int k = 0; k < 4; ++k) m.jr[(size_t)j * V + g() % V] += 0.25f;
    for (int v = 0; v < V; ++v) {
        const int k = v < 2 ? 55 : 1 + v % 4;   // two dense rows, then 1..4 non-zeros
        for (int i = 0; i < k; ++i) m.w[(size_t)v * 55 + (k == 55 ? i : (v * 7 + i * 13) % 55)] = 1.f / k;
    }
    m.parents.resize(55);
    m.parents[0] = -1;
    for (int j = 1; j < 55; ++j) m.parents[j] = j <= 11 ? j - 1 : (int)(g() % j);
    return m;
}

static int run(int V) {
    const int nb = 5, S = 3;
    Model m = make(V, nb, 100 + V);
    // ---- the packer by itself
    const int shift = ab::posedirs_shift(m.pd.data(), m.pd.size());
    CHECK(shift >= 19 && shift <= 21);   // max entry just under 1e-2 -> 2^13..2^14
    std::vector<uint16_t> hi, lo;
    ab::pack_posedirs(m.pd.data(), V, shift, hi, lo);
    const int groups = ab::vertex_groups(V);
    CHECK(hi.size() == (size_t)groups * 16 * 64 * 8 && lo.size() == hi.size());
    std::vector<char> seen(hi.size(), 0);
    const float s = ldexpf(1.f, shift);
    for (int k = 0; k < 486; ++k)
        for (int v = 0; v < V; ++v)
            for (int c = 0; c < 3; ++c) {
                const size_t i = ab::posedirs_index(v, c, k);
                CHECK(i < hi.size() && !seen[i]);
                seen[i] = 1;
                const float x = m.pd[(size_t)k * V * 3 + v * 3 + c] * s;
                CHECK(hi[i] == ab::f2h(x));
                const float back = ab::h2f(hi[i]) + ab::h2f(lo[i]);
                CHECK(fabsf(back - x) <= ldexpf(fabsf(x), -21));
                // the unit's geometry: k-step, lane = (k octet) * 16 + output row, element
                CHECK(i == ((((size_t)(v >> 2) * 16 + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + (v & 3) * 4 + c) * 8 + (k & 7)));
            }
    for (size_t i = 0; i < hi.size(); ++i)
        if (!seen[i]) CHECK(hi[i] == 0 && lo[i] == 0);   // k >= 486, the pad output slot, the pad vertices of the last group
    std::vector<ab::SkinEntry> skin;
    const int nnz = ab::pack_skin(m.w.data(), V, skin);
    CHECK(nnz == 55 && skin.size() == (size_t)groups * 4 * nnz);
    for (int v = 0; v < groups * 4; ++v) {
        std::vector<float> dense(55, 0.f);
        int last = -1, n = 0;
        for (int i = 0; i < nnz; ++i) {
            const ab::SkinEntry e = skin[(size_t)v * nnz + i];
            CHECK(e.joint >= 0 && e.joint < 55);
            if (e.weight != 0.f) { CHECK(e.joint > last && i == n); last = e.joint; ++n; dense[e.joint] = e.weight; }   // ascending joints, no gap before the padding
        }
        for (int j = 0; j < 55; ++j) CHECK(dense[j] == (v < V ? m.w[(size_t)v * 55 + j] : 0.f));
    }
    CHECK(ab::skin_chunks(1, groups) >= 1 && ab::skin_chunks(1, groups) * 8 <= (groups < 8 ? 8 : groups) && ab::skin_chunks(100000, groups) == 1);
    // ---- the context
    const long live0 = amuse_stub_live_allocations();
    amuse_body_model c = m.c();
    {   // parents validation
        Model bad = m;
        bad.parents[9] = 9;
        amuse_body_model bc = bad.c();
        CHECK(amuse_body_create(0, &bc) == nullptr);
        bad.parents[9] = 3; bad.parents[0] = 0;
        bc = bad.c();
        CHECK(amuse_body_create(0, &bc) == nullptr);
        CHECK(amuse_body_create(0, nullptr) == nullptr);
        CHECK(amuse_stub_live_allocations() == live0);
    }
    amuse_body_ctx* ctx = amuse_body_create(0, &c);
    CHECK(ctx != nullptr);
    CHECK(amuse_body_info(ctx, 0) == V && amuse_body_info(ctx, 1) == nnz && amuse_body_info(ctx, 2) == shift && amuse_body_info(ctx, 3) == 0);
    std::vector<int> subj(4, 0);
    std::vector<float> rot((size_t)4 * 17 * 333, 0.1f), out((size_t)4 * 17 * (V > 55 ? V : 55) * 3);
    std::vector<double> sums(2);
    CHECK(amuse_body_forward(ctx, rot.data(), AMUSE_BODY_ROT_AA, nullptr, subj.data(), 4, 17, AMUSE_PREC_F32X, out.data(), nullptr, nullptr) == AMUSE_ESTATE);   // no subjects yet
    std::vector<float> betas((size_t)S * nb);
    for (size_t i = 0; i < betas.size(); ++i) betas[i] = 0.3f * (float)((int)(i % 7) - 3);
    CHECK(amuse_body_set_subjects(ctx, betas.data(), S) == 0 && amuse_body_info(ctx, 3) == S);
    CHECK(amuse_body_set_subjects(ctx, betas.data(), S) == 0);          // again: in place
    CHECK(amuse_body_set_subjects(ctx, betas.data(), 2) == 0 && amuse_body_set_subjects(ctx, betas.data(), S) == 0);   // another count: re-allocated
    CHECK(amuse_body_set_subjects(ctx, nullptr, S) == AMUSE_EINVAL && amuse_body_set_subjects(ctx, betas.data(), 0) == AMUSE_EINVAL);
    // argument checks
    CHECK(amuse_body_forward(ctx, rot.data(), 0, nullptr, subj.data(), 4, 17, AMUSE_PREC_F32, out.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_forward(ctx, rot.data(), 0, nullptr, subj.data(), 4, 17, AMUSE_PREC_BF16, out.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_forward(ctx, rot.data(), 2, nullptr, subj.data(), 4, 17, AMUSE_PREC_F32X, out.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_forward(ctx, rot.data(), 0, nullptr, subj.data(), 4, 17, AMUSE_PREC_F32X, nullptr, nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_forward(ctx, rot.data(), 0, nullptr, nullptr, 4, 17, AMUSE_PREC_F32X, out.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_forward(ctx, rot.data(), 0, nullptr, subj.data(), 0, 17, AMUSE_PREC_F32X, out.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_forward(ctx, rot.data(), 0, nullptr, subj.data(), 1 << 20, 1 << 12, AMUSE_PREC_F32X, out.data(), nullptr, nullptr) == AMUSE_EINVAL);   // N * F beyond 2^31
    CHECK(amuse_body_vertex_loss(ctx, rot.data(), nullptr, nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, sums.data(), nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_reserve(ctx, 0) == AMUSE_EINVAL && amuse_body_reserve(nullptr, 16) == AMUSE_EINVAL);
    CHECK(g_npose == 0 && g_nskin == 0);
    // joints only: the per-frame kernel alone
    CHECK(amuse_body_forward(ctx, rot.data(), AMUSE_BODY_ROT_AA, nullptr, subj.data(), 4, 17, AMUSE_PREC_F16, out.data(), nullptr, nullptr) == 0);
    CHECK(g_npose == 1 && g_nskin == 0 && g_pose[0].rot_stride == 165 && g_pose[0].trans == nullptr && g_pose[0].nframes == 68 && g_pose[0].F == 17 && g_pose[0].n_subjects == S);
    for (int j = 0; j < 55; ++j) CHECK(g_pose[0].parents[j] == m.parents[j]);
    // the uploaded subject images against a double evaluation
    for (int sidx = 0; sidx < S; ++sidx) {
        std::vector<double> vs((size_t)V * 3);
        for (size_t i = 0; i < vs.size(); ++i) {
            double a = m.vt[i];
            for (int b = 0; b < nb; ++b) a += (double)m.sd[i * nb + b] * (double)betas[(size_t)sidx * nb + b];
            vs[i] = a;
        }
        for (int j = 0; j < 55; ++j)
            for (int cc = 0; cc < 3; ++cc) {
                double a = 0;
                for (int v = 0; v < V; ++v) a += (double)m.jr[(size_t)j * V + v] * vs[(size_t)v * 3 + cc];
                CHECK(g_pose[0].J[((size_t)sidx * 55 + j) * 4 + cc] == (float)a);
            }
    }
    // vertices, 6D rows: translation = the row's last three
    CHECK(amuse_body_forward(ctx, rot.data(), AMUSE_BODY_ROT_6D, nullptr, subj.data(), 4, 17, AMUSE_PREC_F32X, nullptr, out.data(), nullptr) == 0);
    CHECK(g_npose == 2 && g_nskin == 1 && g_split == 1 && g_loss == 0 && g_pose[1].rot_stride == 333 && g_pose[1].trans == rot.data() + 330 && g_pose[1].trans_stride == 333);
    CHECK(g_skin.nsets == 1 && g_skin.V == V && g_skin.groups == groups && g_skin.nnz == nnz && g_skin.nframes == 68 && g_skin.vertices_out == out.data());
    CHECK(g_skin.scale_inv == ldexpf(1.f, -shift) && g_skin.chunks == ab::skin_chunks(5, groups));
    CHECK(g_skin.A[0] == g_pose[1].A && g_skin.pf_hi[0] == g_pose[1].pf_hi && g_skin.pf_lo[0] == g_pose[1].pf_lo && g_skin.tr[0] == g_pose[1].tr);
    for (size_t i = 0; i < hi.size(); ++i) CHECK(g_skin.pd_hi[i] == hi[i] && g_skin.pd_lo[i] == lo[i]);
    const ab::SkinEntry* up = static_cast<const ab::SkinEntry*>(g_skin.skin);
    for (size_t i = 0; i < skin.size(); ++i) CHECK(up[i].joint == skin[i].joint && up[i].weight == skin[i].weight);
    for (int sidx = 0; sidx < S; ++sidx)
        for (int v = 0; v < groups * 4; ++v)
            for (int cc = 0; cc < 4; ++cc) {
                double a = 0;
                if (v < V && cc < 3) {
                    a = m.vt[(size_t)v * 3 + cc];
                    for (int b = 0; b < nb; ++b) a += (double)m.sd[((size_t)v * 3 + cc) * nb + b] * (double)betas[(size_t)sidx * nb + b];
                }
                CHECK(g_skin.v_shaped[((size_t)sidx * groups * 4 + v) * 4 + cc] == (float)a);
            }
    // loss: three sets in three workspace slices, then the skinning kernel and the reduction over its partials; a larger call grows the workspace
    CHECK(amuse_body_vertex_loss(ctx, rot.data(), rot.data(), rot.data(), AMUSE_BODY_ROT_6D, subj.data(), 4, 17, AMUSE_PREC_F32X, sums.data(), nullptr) == 0);
    CHECK(g_npose == 5 && g_nskin == 2 && g_nreduce == 1 && g_loss == 1 && g_skin.nsets == 3 && g_reduce_n == 5 * g_skin.chunks);
    CHECK(g_skin.A[1] - g_skin.A[0] == (ptrdiff_t)80 * amuse::kBodyAFloats && g_skin.A[2] - g_skin.A[1] == (ptrdiff_t)80 * amuse::kBodyAFloats);   // 68 frames -> 80
    CHECK(g_skin.pf_lo[0] - g_skin.pf_hi[0] == (ptrdiff_t)80 * 512 && g_skin.pf_hi[1] - g_skin.pf_hi[0] == (ptrdiff_t)2 * 80 * 512);
    std::vector<float> rows((size_t)2 * 100 * 168, 0.05f);
    CHECK(amuse_body_vertex_loss(ctx, rows.data(), rows.data(), nullptr, AMUSE_BODY_ROT_AA, subj.data(), 2, 100, AMUSE_PREC_F16, sums.data(), nullptr) == 0);
    CHECK(g_skin.nsets == 2 && g_split == 0 && g_pose[(g_npose - 1) % 3].rot_stride == 168 && g_pose[(g_npose - 1) % 3].trans == rows.data() + 165);
    CHECK(g_skin.A[1] - g_skin.A[0] == (ptrdiff_t)208 * amuse::kBodyAFloats);
    const float* before = g_skin.A[0];
    CHECK(amuse_body_reserve(ctx, 100) == 0);
    CHECK(amuse_body_vertex_loss(ctx, rot.data(), rot.data(), nullptr, AMUSE_BODY_ROT_6D, subj.data(), 4, 17, AMUSE_PREC_F32X, sums.data(), nullptr) == 0);
    CHECK(g_skin.A[0] == before);   // a smaller call after the sizing: nothing re-allocated
    amuse_body_destroy(ctx);
    amuse_body_destroy(nullptr);
    CHECK(amuse_stub_live_allocations() == live0);
    g_npose = g_nskin = g_nreduce = 0;
    return 0;
}

int main() {
    // the fp16 conversion at its edges
    CHECK(ab::f2h(0.f) == 0 && ab::f2h(65504.f) == 0x7bff && ab::f2h(65520.f) == 0x7c00 && ab::f2h(5.9604645e-8f) == 1 && ab::f2h(2.9802322e-8f) == 0);
    CHECK(ab::h2f(1) == 5.9604644775390625e-8f && ab::h2f(0x3c00) == 1.f && ab::h2f(0xbc00) == -1.f);
    for (int V : {203, 37, 8, 1}) {   // not multiples of 4 (and one that is)
        if (int e = run(V)) return e;
    }
    puts("body_host ok");
    return 0;
}
