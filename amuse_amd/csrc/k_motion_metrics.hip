// Per-clip joint statistics of two motions (include/amuse_hip.h amuse_motion_metrics): the APE / AVE sums of the reference's ComputeMetrics
// (models/latent_diffusion/utils/val_metrics.py:94-137) on posed SMPL-X joints, plus this project's velocity / acceleration sums.  One workgroup per clip; a lane
// per joint (55 of a wave's 64: a wave's three loads cover one frame's 660 contiguous bytes, the root's three are one address for the whole wave), the clip's
// L frames cut into kMetricsWaves contiguous chunks, one per wave.  Inputs are fp32; everything after the load is double.  The variance is two-pass: pass 1
// sums the coordinates (and everything that needs no mean), the waves' partials meet in LDS and EVERY lane adds them in wave order - so all waves hold the same
// mean, bit for bit -, pass 2 re-reads the clip (through L2: 2 x 198 KB at F = 300 do not fit in LDS) and sums the squared deviations.  No atomics; the order of
// every sum is a function of L alone, so a clip's row does not depend on N or on where the clip sits in the batch.
#include "amuse_motion_metrics_host.hpp"

namespace amuse {

namespace {

// slots of a lane's pass-1 partials
enum : int { kApeJoint = 0, kApePose = 1, kApeTraj = 2, kVelG = 3, kVelR = 4, kAccG = 5, kAccR = 6, kSumG = 7, kSumR = 10, kSumLG = 13, kSumLR = 16 };
static_assert(kSumLR + 3 == kMetricsPartials, "the slots fill the partials");

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 load3(const float* __restrict__ p) { return V3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }

__global__ void __launch_bounds__(kMetricsBlock) k_motion_metrics(const MotionMetricsArgs a) {
    __shared__ double part[kMetricsWaves][kMetricsPartials][64];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = a.lengths[n];
    double* __restrict__ row = a.rows + (size_t)n * kMetricsRow;
    if (L < 2 || L > a.F) {                              // (uniform over the workgroup: nobody is left waiting at a barrier)
        for (int i = threadIdx.x; i < kMetricsRow; i += kMetricsBlock) row[i] = __builtin_nan("");
        return;
    }
    const bool live = lane < kSmplxJoints;
    const int j = live ? lane : 0;                       // the nine idle lanes walk joint 0 and write nothing
    const float* __restrict__ G = a.gen + (size_t)n * a.F * (kSmplxJoints * 3);
    const float* __restrict__ R = a.ref + (size_t)n * a.F * (kSmplxJoints * 3);
    const int chunk = (L + kMetricsWaves - 1) / kMetricsWaves;
    const int f0 = wave * chunk < L ? wave * chunk : L, f1 = f0 + chunk < L ? f0 + chunk : L;   // frames below L only: anything may sit beyond

    // ---- pass 1
    double acc[kMetricsPartials];
    for (int k = 0; k < kMetricsPartials; ++k) acc[k] = 0.0;
    V3 g1{0, 0, 0}, g2{0, 0, 0}, r1{0, 0, 0}, r2{0, 0, 0};      // the joint at frames f - 1 and f - 2
    if (f0 < f1 && f0 >= 1) {
        g1 = load3(G + (size_t)(f0 - 1) * 165 + j * 3);
        r1 = load3(R + (size_t)(f0 - 1) * 165 + j * 3);
    }
    if (f0 < f1 && f0 >= 2) {
        g2 = load3(G + (size_t)(f0 - 2) * 165 + j * 3);
        r2 = load3(R + (size_t)(f0 - 2) * 165 + j * 3);
    }
    for (int f = f0; f < f1; ++f) {
        const V3 xg = load3(G + (size_t)f * 165 + j * 3), xr = load3(R + (size_t)f * 165 + j * 3);
        const V3 og = load3(G + (size_t)f * 165), orr = load3(R + (size_t)f * 165);            // the roots
        const V3 lg = sub(xg, og), lr = sub(xr, orr);
        acc[kApeJoint] += norm(sub(xg, xr));
        acc[kApePose] += norm(sub(lg, lr));
        const double tx = og.x - orr.x, tz = og.z - orr.z;                                      // traj: components 0 and 2, y is up
        acc[kApeTraj] += sqrt(tx * tx + tz * tz);
        acc[kSumG] += xg.x; acc[kSumG + 1] += xg.y; acc[kSumG + 2] += xg.z;
        acc[kSumR] += xr.x; acc[kSumR + 1] += xr.y; acc[kSumR + 2] += xr.z;
        acc[kSumLG] += lg.x; acc[kSumLG + 1] += lg.y; acc[kSumLG + 2] += lg.z;
        acc[kSumLR] += lr.x; acc[kSumLR + 1] += lr.y; acc[kSumLR + 2] += lr.z;
        if (f >= 1) {
            acc[kVelG] += norm(sub(xg, g1));
            acc[kVelR] += norm(sub(xr, r1));
        }
        if (f >= 2) {                                                                           // centred on f - 1: X[f] - 2 X[f - 1] + X[f - 2]
            acc[kAccG] += norm(V3{xg.x - 2.0 * g1.x + g2.x, xg.y - 2.0 * g1.y + g2.y, xg.z - 2.0 * g1.z + g2.z});
            acc[kAccR] += norm(V3{xr.x - 2.0 * r1.x + r2.x, xr.y - 2.0 * r1.y + r2.y, xr.z - 2.0 * r1.z + r2.z});
        }
        g2 = g1; g1 = xg; r2 = r1; r1 = xr;
    }
    for (int k = 0; k < kMetricsPartials; ++k) part[wave][k][lane] = acc[k];
    __syncthreads();
    double tot[kMetricsPartials];                        // every lane adds the waves' partials in wave order: one mean for all
    for (int k = 0; k < kMetricsPartials; ++k) tot[k] = 0.0;
#pragma unroll 1                                         // (all waves' partials loaded at once would not fit the register file)
    for (int w = 0; w < kMetricsWaves; ++w)
        for (int k = 0; k < kMetricsPartials; ++k) tot[k] += part[w][k][lane];
    __syncthreads();                                     // the partials are read: pass 2 may overwrite them
    double mean[12];
    for (int k = 0; k < 12; ++k) mean[k] = tot[kSumG + k] / (double)L;

    // ---- pass 2: squared deviations, in the order of mean[]: G, R, local G, local R
    double dev[12];
    for (int k = 0; k < 12; ++k) dev[k] = 0.0;
    for (int f = f0; f < f1; ++f) {
        const V3 xg = load3(G + (size_t)f * 165 + j * 3), xr = load3(R + (size_t)f * 165 + j * 3);
        const V3 og = load3(G + (size_t)f * 165), orr = load3(R + (size_t)f * 165);
        const V3 lg = sub(xg, og), lr = sub(xr, orr);
        const double v[12] = {xg.x, xg.y, xg.z, xr.x, xr.y, xr.z, lg.x, lg.y, lg.z, lr.x, lr.y, lr.z};
        for (int k = 0; k < 12; ++k) {
            const double d = v[k] - mean[k];
            dev[k] += d * d;
        }
    }
    for (int k = 0; k < 12; ++k) part[wave][k][lane] = dev[k];
    __syncthreads();
    if (wave != 0 || !live) return;
    double var[12];
    for (int k = 0; k < 12; ++k) var[k] = 0.0;
#pragma unroll 1
    for (int w = 0; w < kMetricsWaves; ++w)
        for (int k = 0; k < 12; ++k) var[k] += part[w][k][lane];
    for (int k = 0; k < 12; ++k) var[k] /= (double)(L - 1);
    const V3 dj{var[0] - var[3], var[1] - var[4], var[2] - var[5]}, dl{var[6] - var[9], var[7] - var[10], var[8] - var[11]};
    row[kRowApeJoints + j] = tot[kApeJoint];
    row[kRowAveJoints + j] = norm(dj);
    row[kRowVelGen + j] = tot[kVelG];
    row[kRowVelRef + j] = tot[kVelR];
    row[kRowAccGen + j] = tot[kAccG];
    row[kRowAccRef + j] = tot[kAccR];
    if (j == 0) {
        row[kRowApeRoot] = tot[kApeJoint];
        row[kRowApeTraj] = tot[kApeTraj];
        row[kRowAveRoot] = norm(dj);
        row[kRowAveTraj] = sqrt(dj.x * dj.x + dj.z * dj.z);
    } else {
        row[kRowApePose + j - 1] = tot[kApePose];
        row[kRowAvePose + j - 1] = norm(dl);
    }
}

}  // namespace

hipError_t launch_motion_metrics(const MotionMetricsArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_motion_metrics, dim3((unsigned)a.N), dim3(kMetricsBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace amuse
