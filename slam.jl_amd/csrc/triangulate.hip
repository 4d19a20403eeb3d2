// triangulate.hip -- two-view linear triangulation with the depth / reprojection gates of the mapper.
//
// Replaces the per-keypoint arithmetic of triangulate_stereo! and triangulate_temporal!
// (src/mapper.jl:142-183, 185-262): RecoverPose.triangulate (DLT; homogeneous point = eigenvector of A'A for
// its smallest eigenvalue), normalisation, both depth gates, both reprojection gates.  The map surgery around it
// (update_mappoint!, remove_stereo_keypoint!, remove_mappoint_obs!) stays on the host and is driven by `status`.
// One thread per keypoint: a few hundred flops each, the call is bound by its launch + the PCIe round trip of the
// keypoint lists (zero-copy mapped host block, like the tracking kernels).
#include "common.hpp"
#include "geom_device.hpp"
#include <cmath>

struct TriArgs {
    TwoViewMats M;
    const double *px1, *px2;          // (y, x) pairs
    const double *parallax;           // nullptr: stereo semantics (every gate applies)
    double max_error, min_depth, min_parallax;
    int n;
    double *out;                      // n x 3
    uint8_t *status;
};

__global__ __launch_bounds__(64) void k_triangulate(TriArgs T)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= T.n) return;
    const double x1 = T.px1[2 * i + 1], y1 = T.px1[2 * i], x2 = T.px2[2 * i + 1], y2 = T.px2[2 * i];
    double L[4];
    dlt_two_view(x1, y1, x2, y2, T.M.P1, T.M.P2, L);
    T.out[3 * i] = L[0]; T.out[3 * i + 1] = L[1]; T.out[3 * i + 2] = L[2];
    const bool gated = T.parallax == nullptr || T.parallax[i] > T.min_parallax;
    T.status[i] = two_view_gates(L, T.M.T21, T.M.cam1, T.M.cam2, x1, y1, x2, y2, T.max_error, T.min_depth, gated) ? 1 : 0;
}

extern "C" int slam_triangulate(slam_ctx *ctx, const double *P1, const double *P2, const double *T21,
                                const double *cam1, const double *cam2, const double *px1_yx, const double *px2_yx, int n,
                                double max_error, double min_depth, const double *parallax, double min_parallax,
                                double *out_xyz, uint8_t *status)
{
    ARG_TRY(ctx, ctx != nullptr && n >= 0);
    if (n == 0) return SLAM_OK;
    ARG_TRY(ctx, P1 && P2 && T21 && cam1 && cam2 && px1_yx && px2_yx && out_xyz && status);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Layout H;
    const auto o_px1 = H.take<double>((size_t)n * 2), o_px2 = H.take<double>((size_t)n * 2), o_par = H.take<double>(n), o_out = H.take<double>((size_t)n * 3); const auto o_st = H.take<uint8_t>(n);
    char *h, *d;
    int rc = slam_pinned(ctx, H.size(), (void **)&h);
    if (rc) return rc;
    HIP_TRY(ctx, hipHostGetDevicePointer((void **)&d, h, 0));
    memcpy(o_px1.at(h), px1_yx, o_px1.bytes()); memcpy(o_px2.at(h), px2_yx, o_px2.bytes());
    if (parallax) memcpy(o_par.at(h), parallax, o_par.bytes());
    TriArgs T;
    T.M.fill(P1, P2, T21, cam1, cam2);
    T.px1 = o_px1.at(d); T.px2 = o_px2.at(d); T.parallax = parallax ? o_par.at(d) : nullptr;
    T.max_error = max_error; T.min_depth = min_depth; T.min_parallax = min_parallax; T.n = n;
    T.out = o_out.at(d); T.status = o_st.at(d);
    { ProfScope span(ctx, "triangulate");
      hipLaunchKernelGGL(k_triangulate, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, T); }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    memcpy(out_xyz, o_out.at(h), o_out.bytes());
    memcpy(status, o_st.at(h), o_st.bytes());
    return SLAM_OK;
}
