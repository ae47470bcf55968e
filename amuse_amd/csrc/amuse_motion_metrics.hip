// Motion metrics: the two C entry points (include/amuse_hip.h).  Context-free; the call touches HIP only after its checks, in the one launch
// amuse_motion_metrics_host.hpp makes.
#include "amuse_motion_metrics_host.hpp"

extern "C" {

int amuse_motion_metrics_row(void) { return amuse::kMetricsRow; }

int amuse_motion_metrics(const float* joints_gen, const float* joints_ref, const int* lengths_dev, int N, int F, double* rows_out, void* stream) {
    return amuse::motion_metrics(joints_gen, joints_ref, lengths_dev, N, F, rows_out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
