// mst_conv_seam.hip - the C ABI's entries that run ONE convolution of the spectrogram encoder (include/diffmst_hip.h: mst_conv3x3,
// mst_conv_wgrad and their size queries).  The work is in mst_cnn_net.hip (seam_*, declared weak in mst_cnn.h); this file only exports
// it, so that every library built from these sources has the whole ABI: one that links the encoder runs it, one that leaves the
// matrix-core kernels out (the host simulator, which cannot execute them) answers 0 bytes / hipErrorNotSupported, like its other
// encoder entries.
#include "mst_cnn.h"

using namespace mst;

static constexpr int kNotSupported = 801;  // hipErrorNotSupported

extern "C" size_t mst_conv3x3_workspace_bytes(int32_t precision, int32_t cin, int32_t cout) {
    return seam_conv3x3_workspace_bytes ? seam_conv3x3_workspace_bytes(precision, cin, cout) : 0;
}
extern "C" size_t mst_conv3x3_splitk_bytes(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dgrad) {
    return seam_conv3x3_splitk_bytes ? seam_conv3x3_splitk_bytes(n, h, w, cin, cout, dgrad) : 0;
}
extern "C" size_t mst_conv3x3_part_bytes(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dgrad) {
    return seam_conv3x3_part_bytes ? seam_conv3x3_part_bytes(n, h, w, cin, cout, dgrad) : 0;
}
extern "C" int mst_conv3x3(int32_t precision, int32_t dgrad, const void* x, const float* weight, void* out, float* part, int32_t* tiles, int32_t n,
                           int32_t h, int32_t w, int32_t cin, int32_t cout, void* workspace, size_t workspace_bytes, void* splitk,
                           size_t splitk_bytes, void* stream) {
    if (!seam_conv3x3) return kNotSupported;
    return seam_conv3x3(precision, dgrad, x, weight, out, part, tiles, n, h, w, cin, cout, workspace, workspace_bytes, splitk, splitk_bytes, stream);
}
extern "C" size_t mst_conv_wgrad_workspace_bytes(int32_t precision, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout) {
    return seam_conv_wgrad_workspace_bytes ? seam_conv_wgrad_workspace_bytes(precision, n, h, w, cin, cout) : 0;
}
extern "C" int mst_conv_wgrad(int32_t precision, const void* dy, const void* x, float* grad_weight, int32_t n, int32_t h, int32_t w, int32_t cin,
                              int32_t cout, void* workspace, size_t workspace_bytes, int32_t* splits, int32_t* steps_per_split, void* stream) {
    if (!seam_conv_wgrad) return kNotSupported;
    return seam_conv_wgrad(precision, dy, x, grad_weight, n, h, w, cin, cout, workspace, workspace_bytes, splits, steps_per_split, stream);
}
