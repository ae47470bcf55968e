// Stand-alone program (its own main): the host half of the body model's gradient calls - the transposed-image packer of csrc/amuse_body_pack.hpp and
// csrc/amuse_body_grad.hip on top of amuse_body.hip - under AddressSanitizer / UBSan on a machine without a GPU.  The HIP runtime is tests/host_asan/hip_stub.cpp,
// unchanged ("device" memory is host memory); the kernel launchers of k_body.hip and k_body_bwd.hip are stand-ins that keep their argument structs.  Checked:
//   - pack_posedirs_t against the dense matrix with exact integer-valued entries (round trip, every slot written once, every pad slot zero), against the image
//     re-ordered from the forward planes (what amuse_body_enable_grad uploads), and its geometry: lane = (vertex & 3) * 16 + (feature & 15), element = 4 parity + c
//   - amuse_body_enable_grad: AMUSE_ESTATE before it, idempotent, amuse_body_info, the uploaded image, no allocation left after destroy
//   - reserve / grow: the backward partials appear with enable_grad, grow with the workspace, are not re-allocated by a smaller call
//   - argument checks (axis-angle rows, NULL pointers, b without grad_b) and the launch order: poses of ref, a, b; then (skin bwd, pose bwd) per candidate
// Prints the FNV-1a digest of the integer-valued image (tests/golden/body_grad_pack.json holds it) and "body_grad_host ok"; returns 0, or the first failed check and 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../amuse_amd/csrc/amuse_body.hpp"
#include "../../amuse_amd/csrc/amuse_body_bwd.hpp"
#include "../../amuse_amd/csrc/amuse_body_pack.hpp"
#include "../../include/amuse_hip.h"

long amuse_stub_live_allocations();

#include "../host_check.hpp"

static std::string g_order;
static amuse::BodyPoseArgs g_pose[3];
static amuse::BodySkinBwdArgs g_sb[2];
static amuse::BodyPoseBwdArgs g_pb[2];
static int g_npose = 0, g_nsb = 0, g_npb = 0, g_split = -1;
namespace amuse {
hipError_t launch_body_pose(const BodyPoseArgs& a, hipStream_t) { g_pose[g_npose++ % 3] = a; g_order += 'p'; return hipSuccess; }
hipError_t launch_body_skin(const BodySkinArgs&, int, int, hipStream_t) { g_order += 's'; return hipSuccess; }
hipError_t launch_body_loss_reduce(const float*, int, int, double*, hipStream_t) { g_order += 'r'; return hipSuccess; }
hipError_t launch_body_skin_bwd(const BodySkinBwdArgs& a, int split, hipStream_t) { g_sb[g_nsb++ % 2] = a; g_split = split; g_order += 'S'; return hipSuccess; }
hipError_t launch_body_pose_bwd(const BodyPoseBwdArgs& a, hipStream_t) { g_pb[g_npb++ % 2] = a; g_order += 'P'; return hipSuccess; }
}  // namespace amuse

namespace ab = amuse_body;

// integer-valued posedirs: every entry in -30..30, so that hi is exact, lo is zero and the round trip is an identity (shift 0 .. the packer's pre-scale is exact)
static float entry(int k, int v, int c) { return (float)((k * 31 + v * 7 + c * 3) % 61 - 30); }

static unsigned long long fnv(const std::vector<uint16_t>& a, unsigned long long h) {
    for (uint16_t x : a) {
        h = (h ^ (x & 0xff)) * 1099511628211ull;
        h = (h ^ (x >> 8)) * 1099511628211ull;
    }
    return h;
}

static int run(int V, bool digest) {
    std::vector<float> pd((size_t)486 * V * 3);
    for (int k = 0; k < 486; ++k)
        for (int v = 0; v < V; ++v)
            for (int c = 0; c < 3; ++c) pd[(size_t)k * V * 3 + v * 3 + c] = entry(k, v, c);
    const int shift = ab::posedirs_shift(pd.data(), pd.size());
    CHECK(shift == 9);   // 30 = 0.94 x 2^5 -> 2^14
    std::vector<uint16_t> hi, lo, fh, fl, th, tl;
    ab::pack_posedirs_t(pd.data(), V, shift, hi, lo);
    const int groups = ab::vertex_groups(V), pairs = ab::vertex_pairs(V);
    CHECK(pairs == (groups + 1) / 2 && hi.size() == (size_t)pairs * 32 * 64 * 8 && lo.size() == hi.size() && hi.size() == ab::posedirs_t_plane_halfs(V));
    std::vector<char> seen(hi.size(), 0);
    const float s = ldexpf(1.f, shift);
    for (int k = 0; k < 486; ++k)
        for (int v = 0; v < V; ++v)
            for (int c = 0; c < 3; ++c) {
                const size_t i = ab::posedirs_t_index(v, c, k);
                CHECK(i < hi.size() && !seen[i]);
                seen[i] = 1;
                CHECK(ab::h2f(hi[i]) == entry(k, v, c) * s && lo[i] == 0);   // exact: the round trip against the dense matrix
                // the unit's geometry: (pair, feature tile), lane = (vertex-in-group) * 16 + feature row, element = 4 x group parity + coordinate
                CHECK(i == ((((size_t)(v >> 3) * 32 + (k >> 4)) * 64 + (size_t)((v & 3) * 16 + (k & 15))) * 8 + (size_t)(((v >> 2) & 1) * 4 + c)));
            }
    for (size_t i = 0; i < hi.size(); ++i)
        if (!seen[i]) CHECK(hi[i] == 0 && lo[i] == 0);   // feature rows 486..511, the pad coordinate, the pad vertices, the missing group of an odd count
    ab::pack_posedirs(pd.data(), V, shift, fh, fl);
    ab::transpose_posedirs_plane(fh.data(), V, th);
    ab::transpose_posedirs_plane(fl.data(), V, tl);
    CHECK(th == hi && tl == lo);
    if (digest) printf("digest V %d %016llx\n", V, fnv(lo, fnv(hi, 1469598103934665603ull)));
    // a matrix with lo pieces: the re-ordered forward planes are the dense packer's image there too
    for (size_t i = 0; i < pd.size(); ++i) pd[i] = pd[i] * 1e-3f + 1e-6f * (float)(i % 13);
    const int shift2 = ab::posedirs_shift(pd.data(), pd.size());
    ab::pack_posedirs_t(pd.data(), V, shift2, hi, lo);
    ab::pack_posedirs(pd.data(), V, shift2, fh, fl);
    ab::transpose_posedirs_plane(fh.data(), V, th);
    ab::transpose_posedirs_plane(fl.data(), V, tl);
    CHECK(th == hi && tl == lo);
    bool any_lo = false;
    for (uint16_t x : lo) any_lo |= x != 0;
    CHECK(any_lo);
    CHECK(ab::bwd_chunks(1, pairs) >= 1 && ab::bwd_chunks(1, pairs) * 8 <= (pairs < 8 ? 8 : pairs) && ab::bwd_chunks(100000, pairs) == 1);
    for (int tiles : {1, 2, 3, 5, 7, 100, 511, 512, 513, 600, 4000})
        CHECK((size_t)tiles * ab::bwd_chunks(tiles, 1 << 20) <= ab::bwd_partial_workgroups((size_t)tiles * 16));
    // ---- the context
    std::vector<float> vt((size_t)V * 3, 0.25f), jr((size_t)55 * V, 0.f), w((size_t)V * 55, 0.f);
    std::vector<int> parents(55);
    parents[0] = -1;
    for (int j = 1; j < 55; ++j) parents[j] = (j - 1) / 2;
    for (int j = 0; j < 55; ++j) jr[(size_t)j * V + j % V] = 1.f;
    for (int v = 0; v < V; ++v) w[(size_t)v * 55 + v % 55] = 1.f;
    const long live0 = amuse_stub_live_allocations();
    amuse_body_model m = {V, 0, vt.data(), nullptr, pd.data(), jr.data(), w.data(), parents.data()};
    amuse_body_ctx* ctx = amuse_body_create(0, &m);
    CHECK(ctx != nullptr);
    float beta = 0.f;
    CHECK(amuse_body_set_subjects(ctx, &beta, 1) == 0);
    std::vector<int> subj(4, 0);
    std::vector<float> rows((size_t)4 * 17 * 333, 0.1f), ga(rows.size()), gb(rows.size());
    std::vector<double> sums(2);
    CHECK(amuse_body_info(ctx, 4) == 0);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, AMUSE_BODY_ROT_6D, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_ESTATE);
    CHECK(amuse_body_enable_grad(nullptr) == AMUSE_EINVAL);
    // a workspace that exists before enable_grad gets its partials from enable_grad
    CHECK(amuse_body_vertex_loss(ctx, rows.data(), rows.data(), nullptr, AMUSE_BODY_ROT_6D, subj.data(), 4, 17, AMUSE_PREC_F32X, sums.data(), nullptr) == 0);
    const long live1 = amuse_stub_live_allocations();
    CHECK(amuse_body_enable_grad(ctx) == 0 && amuse_body_info(ctx, 4) == 1);
    CHECK(amuse_stub_live_allocations() == live1 + 4);   // the two planes of the image, the two partial arrays
    CHECK(amuse_body_enable_grad(ctx) == 0 && amuse_stub_live_allocations() == live1 + 4);   // idempotent
    // argument checks: nothing is launched
    g_order.clear();
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, AMUSE_BODY_ROT_AA, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), nullptr, nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, nullptr, nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), rows.data(), 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), gb.data(), nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, 1, nullptr, 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(amuse_body_vertex_loss_grad(nullptr, rows.data(), rows.data(), nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == AMUSE_EINVAL);
    CHECK(g_order.empty());
    // one candidate, then two: the launch order and the arguments
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data() + 333, nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F16, 0.5f, 9.f, ga.data(), nullptr, nullptr) == 0);
    CHECK(g_order == "ppSP" && g_split == 0);
    const amuse::BodySkinBwdArgs& sb = g_sb[(g_nsb - 1) % 2];
    const amuse::BodyPoseBwdArgs& pb = g_pb[(g_npb - 1) % 2];
    CHECK(sb.V == V && sb.groups == groups && sb.pairs == pairs && sb.nframes == 68 && sb.F == 17 && sb.chunks == ab::bwd_chunks(5, pairs) && sb.n_subjects == 1);
    CHECK(sb.scale_inv == ldexpf(1.f, -shift2));
    CHECK(sb.A[1] - sb.A[0] == (ptrdiff_t)80 * amuse::kBodyAFloats && sb.pf_lo[0] - sb.pf_hi[0] == (ptrdiff_t)80 * 512 && sb.pf_hi[1] - sb.pf_hi[0] == (ptrdiff_t)2 * 80 * 512);
    CHECK(sb.tr[1] - sb.tr[0] == (ptrdiff_t)80 * 4);
    for (size_t i = 0; i < hi.size(); ++i) CHECK(sb.pt_hi[i] == hi[i] && sb.pt_lo[i] == lo[i]);   // the uploaded image
    for (size_t i = 0; i < fh.size(); ++i) CHECK(sb.pd_hi[i] == fh[i] && sb.pd_lo[i] == fl[i]);
    CHECK(pb.rows == rows.data() + 333 && pb.grad == ga.data() && pb.scale == 0.5f && pb.chunks == sb.chunks && pb.A == sb.A[1] && pb.nframes == 68 && pb.F == 17);
    CHECK(pb.dA_part == sb.dA_part && pb.dpf_part == sb.dpf_part && pb.dpf_scale == ldexpf(1.f, -(shift2 + amuse::kBodyDpShift)));
    for (int j = 0; j < 55; ++j) CHECK(pb.parents[j] == parents[j]);
    // the partial arrays hold every workgroup's slice: write the last one ("device" memory is host memory here, ASan watches)
    const size_t last = (size_t)5 * sb.chunks - 1;
    sb.dA_part[(last + 1) * 16 * amuse::kBodyDAStride - 1] = 1.f;
    sb.dpf_part[(last + 1) * amuse::kBodyDpfFloats - 1] = 1.f;
    g_order.clear();
    const float* parts = sb.dA_part;
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), rows.data() + 666, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 2.f, ga.data(), gb.data(), nullptr) == 0);
    CHECK(g_order == "pppSPSP" && g_split == 1);
    CHECK(g_pb[(g_npb - 2) % 2].grad == ga.data() && g_pb[(g_npb - 1) % 2].grad == gb.data() && g_pb[(g_npb - 1) % 2].scale == 2.f && g_pb[(g_npb - 1) % 2].rows == rows.data() + 666);
    CHECK(g_sb[(g_nsb - 1) % 2].A[1] - g_sb[(g_nsb - 1) % 2].A[0] == (ptrdiff_t)2 * 80 * amuse::kBodyAFloats && g_pb[(g_npb - 1) % 2].A == g_sb[(g_nsb - 1) % 2].A[1]);
    CHECK(g_sb[(g_nsb - 1) % 2].dA_part == parts);       // covered: nothing re-allocated
    // growing: a larger call (or reserve) re-allocates workspace AND partials, and keeps the old ones until destroy
    const long live2 = amuse_stub_live_allocations();
    CHECK(amuse_body_reserve(ctx, 4000) == 0);
    CHECK(amuse_stub_live_allocations() == live2 + 6);
    std::vector<float> big((size_t)2 * 100 * 333, 0.1f), gbig(big.size());
    CHECK(amuse_body_vertex_loss_grad(ctx, big.data(), big.data(), nullptr, 1, subj.data(), 2, 100, AMUSE_PREC_F32X, 1.f, 1.f, gbig.data(), nullptr, nullptr) == 0);
    CHECK(amuse_stub_live_allocations() == live2 + 6 && g_sb[(g_nsb - 1) % 2].dA_part != parts);
    const amuse::BodySkinBwdArgs& sg = g_sb[(g_nsb - 1) % 2];
    sg.dA_part[ab::bwd_partial_workgroups(4000) * 16 * amuse::kBodyDAStride - 1] = 1.f;
    sg.dpf_part[ab::bwd_partial_workgroups(4000) * amuse::kBodyDpfFloats - 1] = 1.f;
    const_cast<float*>(parts)[0] = 2.f;                  // the outgrown partials are still alive (a graph captured earlier replays into them)
    amuse_body_destroy(ctx);
    CHECK(amuse_stub_live_allocations() == live0);
    // enable_grad first, then the first call sizes both
    ctx = amuse_body_create(0, &m);
    CHECK(ctx && amuse_body_set_subjects(ctx, &beta, 1) == 0 && amuse_body_enable_grad(ctx) == 0);
    CHECK(amuse_body_vertex_loss_grad(ctx, rows.data(), rows.data(), nullptr, 1, subj.data(), 4, 17, AMUSE_PREC_F32X, 1.f, 1.f, ga.data(), nullptr, nullptr) == 0);
    CHECK(g_sb[(g_nsb - 1) % 2].dA_part != nullptr && g_sb[(g_nsb - 1) % 2].dpf_part != nullptr);
    amuse_body_destroy(ctx);
    CHECK(amuse_stub_live_allocations() == live0);
    g_order.clear();
    return 0;
}

int main() {
    for (int V : {203, 37, 8, 1, 12}) {   // odd and even group counts, a single vertex
        if (int e = run(V, V == 203 || V == 37)) return e;
    }
    puts("body_grad_host ok");
    return 0;
}
