// Preview video: the C entry points (include/amuse_hip.h).  The tables, the plan and the header touch no HIP at all; create uploads the tables; reserve
// allocates; the calls touch HIP only after their checks, in the launches amuse_mjpeg_host.hpp makes.
#include "amuse_mjpeg_host.hpp"

extern "C" {

int amuse_mjpeg_tables(int quality, unsigned char* luma_q64, unsigned char* chroma_q64) { return amuse::mjpeg_tables(quality, luma_q64, chroma_q64); }

int amuse_mjpeg_plan(int width, int height, int frames, int* mcus_x, int* mcus_y, int* header_bytes, size_t* workspace_bytes, size_t* worst_case_bytes_per_frame) {
    amuse::MjpegPlan p{};
    if (int rc = amuse::mjpeg_plan(width, height, frames, &p)) return rc;
    if (mcus_x) *mcus_x = p.mcus_x;
    if (mcus_y) *mcus_y = p.mcus_y;
    if (header_bytes) *header_bytes = p.header_bytes;
    if (workspace_bytes) *workspace_bytes = p.workspace_bytes;
    if (worst_case_bytes_per_frame) *worst_case_bytes_per_frame = p.worst_case_bytes_per_frame;
    return AMUSE_OK;
}

amuse_mjpeg* amuse_mjpeg_create(int device, int width, int height, int quality) {
    return reinterpret_cast<amuse_mjpeg*>(amuse::mjpeg_create(device, width, height, quality));   // (the opaque handle IS the host struct)
}

int amuse_mjpeg_reserve(amuse_mjpeg* e, int frames) { return amuse::mjpeg_reserve(reinterpret_cast<amuse::Mjpeg*>(e), frames); }

void amuse_mjpeg_destroy(amuse_mjpeg* e) { amuse::mjpeg_destroy(reinterpret_cast<amuse::Mjpeg*>(e)); }

int amuse_mjpeg_encode(amuse_mjpeg* e, const unsigned char* rgb_dev, int M, unsigned char* out_dev, size_t out_capacity, unsigned long long* offsets_dev,
                       unsigned int* sizes_dev, unsigned long long* total_dev, void* stream) {
    return amuse::mjpeg_encode(reinterpret_cast<amuse::Mjpeg*>(e), rgb_dev, M, out_dev, out_capacity, offsets_dev, sizes_dev, total_dev,
                               static_cast<hipStream_t>(stream));
}

int amuse_debug_mjpeg_coefficients(amuse_mjpeg* e, const unsigned char* rgb_dev, int M, short* coef_dev, void* stream) {
    return amuse::mjpeg_coefficients(reinterpret_cast<amuse::Mjpeg*>(e), rgb_dev, M, coef_dev, static_cast<hipStream_t>(stream));
}

int amuse_debug_mjpeg_header(int width, int height, int quality, unsigned char* out_host, size_t capacity, int* bytes) {
    unsigned char luma[64], chroma[64];
    if (int rc = amuse::mjpeg_check_size(width, height)) return rc;
    if (int rc = amuse::mjpeg_tables(quality, luma, chroma)) return rc;
    if (!out_host || !bytes) return amuse_failf(AMUSE_EINVAL, "amuse_debug_mjpeg_header: out and bytes must be given");
    const std::vector<unsigned char> h = amuse::mjpeg_header(width, height, luma, chroma);
    *bytes = (int)h.size();
    if (h.size() <= capacity) memcpy(out_host, h.data(), h.size());
    return AMUSE_OK;
}

}  // extern "C"
