// Long-form candidates (include/amuse_hip.h amuse_seam_cost / amuse_seam_path / amuse_seam_select): K candidates of every window, the cost of every (candidate of
// window k, candidate of window k + 1) pair over the frames the two windows share, the path of least total cost, and the gather of its windows.
//   k_seam_quats   a thread per (seam, side, candidate, overlap row, joint): axis-angle -> unit quaternion ONCE, into the caller's workspace - the K x K pairs of
//                  a seam read 2 K candidates' rows, so no conversion is repeated per pair.
//   k_seam_cost    a wave per pair, a lane per joint (lane 55: the translation), a loop over the overlap rows: the geodesic angle in fp32, its weighted square
//                  and every sum in double.  Per lane the rows are added in row order, then the 64 lanes by the xor butterfly 32, 16, .., 1: ONE order, whatever K,
//                  the pair's place in the grid or the sequence's place in the call.  No atomics, no LDS.
//   k_seam_path    a wave per sequence, a lane per candidate: the dynamic programme in double, back-pointers in LDS (a byte each), then the backtrack.
//   k_seam_select  a thread per float of an output row: the chosen batch row's bits.
// A translation unit of its own; the quaternion arithmetic is amuse_rot.hpp's.
#include "amuse_rot.hpp"
#include "amuse_seam_host.hpp"

namespace amuse {

namespace {

// overlap rows of seam k that reach the output: min(F - hop, L - (k + 1) hop), >= 1 by the entry point's check on L
__device__ __forceinline__ int seam_rows(int F, int hop, int L, int k) {
    const int O = F - hop, left = L - (k + 1) * hop;
    return left < O ? left : O;
}

__global__ void __launch_bounds__(kSeamBlock) k_seam_quats(const SeamArgs a) {
    const SeamSeq sq = a.seq[blockIdx.z];
    const int k = blockIdx.y >> 1, side = blockIdx.y & 1;            // side 0: window k's rows i + hop; side 1: window k + 1's rows i
    if (k >= sq.W - 1) return;
    const int O = a.F - a.hop, Ok = seam_rows(a.F, a.hop, sq.L, k);
    const int idx = blockIdx.x * kSeamBlock + threadIdx.x;          // (candidate, row, joint)
    const int per = O * kSmplxJoints;
    const int c = idx / per, r = idx - c * per, i = r / kSmplxJoints, j = r - i * kSmplxJoints;
    if (c >= a.K || i >= Ok) return;
    const size_t row = ((size_t)(sq.win0 + k + side) * a.K + c) * a.F + (side ? i : i + a.hop);
    const float* p = a.poses + (row * kSmplxJoints + j) * 3;
    const Quat q = aa_to_quat(p[0], p[1], p[2]);
    a.quats[(((size_t)(sq.seam0 + k) * 2 + side) * a.K + c) * per + r] = make_float4(q.w, q.x, q.y, q.z);
}

__global__ void __launch_bounds__(kSeamBlock) k_seam_cost(const SeamArgs a) {
    const SeamSeq sq = a.seq[blockIdx.z];
    const int k = blockIdx.y;
    if (k >= sq.W - 1) return;
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * (kSeamBlock / 64) + (threadIdx.x >> 6);
    if (pair >= a.K * a.K) return;                                   // (a whole wave: the shuffles below stay among lanes that all arrive)
    const int ca = pair / a.K, cb = pair - ca * a.K;
    const int O = a.F - a.hop, Ok = seam_rows(a.F, a.hop, sq.L, k);
    const size_t per = (size_t)O * kSmplxJoints, seam = (size_t)(sq.seam0 + k);
    double acc = 0.0;
    if (lane < kSmplxJoints) {
        const float4* qa = a.quats + ((seam * 2 + 0) * a.K + ca) * per + lane;
        const float4* qb = a.quats + ((seam * 2 + 1) * a.K + cb) * per + lane;
        const double wj = (double)a.joint_weight[lane];
        for (int i = 0; i < Ok; ++i) {
            const float4 A = qa[(size_t)i * kSmplxJoints], B = qb[(size_t)i * kSmplxJoints];
            const Quat r = quat_conj_mul(Quat{A.x, A.y, A.z, A.w}, Quat{B.x, B.y, B.z, B.w});
            const float th = 2.0f * atan2f(sqrtf(r.x * r.x + r.y * r.y + r.z * r.z), fabsf(r.w));
            acc += (double)a.row_weight[i] * (wj * ((double)th * (double)th));
        }
    } else if (lane == kSmplxJoints && a.trans != nullptr) {
        const float* ta = a.trans + (((size_t)(sq.win0 + k) * a.K + ca) * a.F + a.hop) * 3;
        const float* tb = a.trans + (((size_t)(sq.win0 + k + 1) * a.K + cb) * a.F) * 3;
        const double tw = (double)a.trans_weight;
        for (int i = 0; i < Ok; ++i) {
            const float dx = ta[i * 3] - tb[i * 3], dy = ta[i * 3 + 1] - tb[i * 3 + 1], dz = ta[i * 3 + 2] - tb[i * 3 + 2];
            const double d2 = (double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz;
            acc += (double)a.row_weight[i] * (tw * d2);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) a.cost[(seam * a.K + ca) * a.K + cb] = acc;
}

// a sum that is not finite counts as +infinity: it never wins a `<`
__device__ __forceinline__ double finite_or_inf(double v) { return fabs(v) < __builtin_huge_val() ? v : __builtin_huge_val(); }

__global__ void __launch_bounds__(64) k_seam_path(const PathArgs a) {
    __shared__ unsigned char back[kSeamPathWindows * 64];            // back[(k - lo - 1) * 64 + b]: the candidate of window k - 1 on the best way to (k, b)
    const SeamSeq sq = a.seq[blockIdx.x];
    const int lane = threadIdx.x, K = a.K, W = sq.W;
    const double inf = __builtin_huge_val();
    int hi = W - 1, c = -1;
    // back-pointers for kSeamPathWindows windows at a time, from the sequence's end: each round runs the forward pass again from window 0 (the same values every
    // time) and keeps the pointers of (lo, hi] only.  One round for any sequence of up to 961 windows.
    for (;;) {
        const int lo = hi > kSeamPathWindows ? hi - kSeamPathWindows : 0;
        double best = lane < K ? 0.0 : inf;
        for (int k = 1; k <= hi; ++k) {
            const double* m = a.cost + (size_t)(sq.seam0 + k - 1) * K * K + lane;
            double nb = inf;
            int arg = 0;
            for (int ca = 0; ca < K; ++ca) {
                const double from = __shfl(best, ca);
                const double v = lane < K ? finite_or_inf(from + m[(size_t)ca * K]) : inf;
                if (v < nb) { nb = v; arg = ca; }
            }
            if (k > lo) back[(k - lo - 1) * 64 + lane] = (unsigned char)arg;
            best = nb;
        }
        if (c < 0) {                                                 // the first round: the end of the path and its total
            double tot = inf;
            c = 0;
            for (int cb = 0; cb < K; ++cb) {
                const double v = __shfl(best, cb);
                if (v < tot) { tot = v; c = cb; }
            }
            if (lane == 0) a.total[a.seq0 + blockIdx.x] = W == 1 ? 0.0 : tot;
        }
        __syncthreads();                                             // one wave: orders the LDS writes above before the reads below
        if (lane == 0) {
            a.choice[sq.win0 + hi] = (sq.win0 + hi) * K + c;
            for (int k = hi; k > lo; --k) {
                c = back[(k - lo - 1) * 64 + c];
                a.choice[sq.win0 + k - 1] = (sq.win0 + k - 1) * K + c;
            }
        }
        c = __shfl(c, 0);
        if (lo == 0) break;
        hi = lo;
        __syncthreads();                                             // the next round overwrites what lane 0 just read
    }
}

__global__ void __launch_bounds__(kSeamBlock) k_seam_select(const SelectArgs a) {
    const int per_p = a.F * kSmplxJoints * 3, per = per_p + (a.trans ? a.F * 3 : 0);
    const int e = blockIdx.x * kSeamBlock + threadIdx.x;
    if (e >= per) return;
    for (int r = blockIdx.y; r < a.n; r += gridDim.y) {
        const int src = a.choice[r];
        const bool ok = src >= 0 && src < a.n_in;                    // a row outside the input is never read: the output row is NaN
        if (e < per_p) a.poses_out[(size_t)r * per_p + e] = ok ? a.poses[(size_t)src * per_p + e] : __builtin_nanf("");
        else a.trans_out[(size_t)r * (a.F * 3) + (e - per_p)] = ok ? a.trans[(size_t)src * (a.F * 3) + (e - per_p)] : __builtin_nanf("");
    }
}

}  // namespace

hipError_t launch_seam_cost(const SeamArgs& a, hipStream_t stream) {
    if (a.max_seams == 0) return hipSuccess;                         // a launch of single-window sequences has no seam
    const long long elems = (long long)a.K * (a.F - a.hop) * kSmplxJoints;
    const dim3 gq((unsigned)((elems + kSeamBlock - 1) / kSeamBlock), (unsigned)(2 * a.max_seams), (unsigned)a.nseq);
    hipLaunchKernelGGL(k_seam_quats, gq, dim3(kSeamBlock), 0, stream, a);
    const int per_block = kSeamBlock / 64;
    const dim3 gc((unsigned)((a.K * a.K + per_block - 1) / per_block), (unsigned)a.max_seams, (unsigned)a.nseq);
    hipLaunchKernelGGL(k_seam_cost, gc, dim3(kSeamBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seam_path(const PathArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_seam_path, dim3((unsigned)a.nseq), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seam_select(const SelectArgs& a, hipStream_t stream) {
    const long long per = (long long)a.F * (kSmplxJoints * 3 + (a.trans ? 3 : 0));
    const dim3 grid((unsigned)((per + kSeamBlock - 1) / kSeamBlock), (unsigned)(a.n < 65535 ? a.n : 65535));
    hipLaunchKernelGGL(k_seam_select, grid, dim3(kSeamBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
