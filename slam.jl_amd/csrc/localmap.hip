// localmap.hip -- the mapper's local-map re-matching: do_local_map_matching + find_best_match + mappoint_min_distance
// (src/mapper.jl:318-462, src/map_point.jl:165-174), the one consumer of the BRIEF descriptors slam_describe computes.
//
// Every local-map point is projected into the new key-frame (depth / view-angle / image gates, mapper.jl:345-352), the keypoints of the 3x3 grid
// cells around the projection (frame.jl:576-599) are tested against it (pixel distance, disjoint observers, mean reprojection of the point into
// the keypoint's observers, mapper.jl:407-442) and the survivor with the smallest Hamming distance over all descriptor pairs is its choice; a
// keypoint chosen by several points keeps the closest one (mapper.jl:370-381).  Both selections compare with <=, so among equal distances the
// candidate met LAST wins; the kernel keeps that with order-independent keys instead of lists.
//
// k_lmm_match: stream on blockIdx.y, a group of G lanes per local-map point.  Candidate slot k of the neighbourhood (cells r outer / c inner,
// list order inside a cell) belongs to lane k mod G; a lane meets its slots in ascending order, the group folds (distance, slot) under "smaller
// distance, then larger slot", and a matched point issues one 64-bit atomicMin of (distance << 32 | ~index) on the keypoint's word: smaller
// distance, then LARGER local-map index, whatever the arrival order.  Distances are integers 0 .. 256 held in doubles, so the key is exact.
//
// Per stream the call moves about M (24 + 32 D + 4 O) + N (16 + 32 D + 20 O) + 4 (cells + N) bytes (D descriptors, O observers per point on
// average): under 2 MB at M = 10 000, N = 1 000.  It is bound by latency and issue, not by bandwidth.  One packed buffer per call (lmm_host.hpp):
// one copy in, one memset of the keys, one launch, one copy out; the keys are decoded on the host.
#include "common.hpp"
#include "lmm_host.hpp"
#include <cmath>

// f.cw * to_homogeneous(point) (frame.jl:458-462): the first three rows, each summed left to right
__device__ __forceinline__ void lmm_to_camera(const double *T, double X, double Y, double Z, double c[3])
{
    for (int r = 0; r < 3; r++) c[r] = ((T[r] * X + T[r + 4] * Y) + T[r + 8] * Z) + T[r + 12] * 1.0;
}

// project_undistort -> undistort_pdn_point (camera.jl:79-82, 111-125), (y, x) order
__device__ __forceinline__ void lmm_project_undistort(const LmmStream &S, const double c[3], double &py, double &px)
{
    const double ny = c[1] / c[2], nx = c[0] / c[2];
    const double sy = ny * ny, sx = nx * nx;
    const double r2 = sy + sx;
    const double rd = (1.0 + S.k1 * r2) + S.k2 * (r2 * r2);
    const double p = ny * nx;
    const double dtx = (2.0 * S.p1) * p + S.p2 * (r2 + 2.0 * sy);
    const double dty = S.p1 * (r2 + 2.0 * sx) + (2.0 * S.p2) * p;
    const double dy = rd * ny + dty, dx = rd * nx + dtx;
    py = dy * S.fy + S.cy; px = dx * S.fx + S.cx;
}

// the per-candidate tests of find_best_match (mapper.jl:406-444) for local-map point gm against keypoint gj (indices into the concatenated
// arrays); returns the descriptor distance, or -1.0 when a test rejects the candidate
__device__ double lmm_candidate(const LmmDev &D, const LmmStream &S, int gm, int gj, double py, double px, double X, double Y, double Z)
{
    const int d2b = D.kp_desc_off[gj], d2e = D.kp_desc_off[gj + 1];
    if (d2e == d2b) return -1.0;                                        // :406, :411-415: the caller lists no descriptor for such a keypoint
    const double ey = py - D.kp_yx[2 * (size_t)gj], ex = px - D.kp_yx[2 * (size_t)gj + 1];
    if (sqrt(ey * ey + ex * ex) > S.max_proj) return -1.0;              // :407-408
    const int o1b = D.mp_obs_off[gm], o1e = D.mp_obs_off[gm + 1], o2b = D.kp_obs_off[gj], o2e = D.kp_obs_off[gj + 1];
    for (int u = o1b; u < o1e; u++) {                                   // :419-420
        const int kf = D.mp_obs_kf[u];
        for (int v = o2b; v < o2e; v++)
            if (D.kp_obs_kf[v] == kf) return -1.0;
    }
    double avg = 0.0; int n = 0;                                        // :422-442; no listed observer: 0.0 / 0 = NaN, the comparison is false, the candidate passes
    for (int v = o2b; v < o2e; v++) {
        double c[3], oy, ox;
        lmm_to_camera(D.kf_Tcw + 16 * (size_t)(S.kf0 + D.kp_obs_kf[v]), X, Y, Z, c);
        lmm_project_undistort(S, c, oy, ox);
        const double fy = D.kp_obs_yx[2 * (size_t)v] - oy, fx = D.kp_obs_yx[2 * (size_t)v + 1] - ox;
        avg += sqrt(fy * fy + fx * fx);
        n += 1;
    }
    avg /= (double)n;
    if (avg > S.max_proj) return -1.0;
    double best = 1e6;                                                  // map_point.jl:165-174
    for (int u = D.mp_desc_off[gm], ue = D.mp_desc_off[gm + 1]; u < ue; u++) {
        const uint64_t *a = D.mp_desc + 4 * (size_t)u;
        const uint64_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
        for (int v = d2b; v < d2e; v++) {
            const uint64_t *b = D.kp_desc + 4 * (size_t)v;
            const double d = (double)(__popcll(a0 ^ b[0]) + __popcll(a1 ^ b[1]) + __popcll(a2 ^ b[2]) + __popcll(a3 ^ b[3]));
            if (d < best) best = d;
        }
    }
    return best;
}

template <int G>
__global__ __launch_bounds__(256) void k_lmm_match(LmmDev D)
{
    static_assert(G == 16 || G == 32 || G == 64, "a group is a power-of-two slice of one wave");
    const LmmStream &S = D.st[blockIdx.y];
    const int lane = threadIdx.x % G;
    const int m = blockIdx.x * (256 / G) + threadIdx.x / G;
    if (m >= S.M) return;                                               // whole groups leave: every shuffle below stays inside one group
    const int gm = S.mp0 + m;
    const double X = D.mp_xyz[3 * (size_t)gm], Y = D.mp_xyz[3 * (size_t)gm + 1], Z = D.mp_xyz[3 * (size_t)gm + 2];
    // the gates, in the reference's order (mapper.jl:345-352); the same value in every lane of the group
    double c[3], py = 0.0, px = 0.0;
    lmm_to_camera(S.Tcw, X, Y, Z, c);
    bool live = !(c[2] < 0.1);
    if (live) {
        const double view = c[2] / sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        live = !(fabs(view) < S.view_thr);
    }
    if (live) {
        lmm_project_undistort(S, c, py, px);
        live = 1.0 <= py && py <= S.H && 1.0 <= px && px <= S.W;        // camera.jl:90-92
    }
    if (!live) {
        if (lane == 0) {
            D.best_kp[gm] = -1; D.best_dist[gm] = -1.0;
            D.proj[2 * (size_t)gm] = D.proj[2 * (size_t)gm + 1] = __builtin_nan("");
        }
        return;
    }
    // find_best_match over the 3x3 cells (frame.jl:579-591): cells outside the grid are skipped one by one, not clamped
    const int r0 = (int)((long long)rint(py) / S.cell + 1), c0 = (int)((long long)rint(px) / S.cell + 1);     // 1-based (SLAM.jl:42-45)
    const int32_t *cell_off = D.cell_off + S.cell0, *cell_kp = D.cell_kp + S.kp0;
    double best = S.start; int best_slot = -1, best_j = -1;
    int base = 0;                                                       // slots before the current cell
    for (int r = r0 - 1; r <= r0 + 1; r++)
        for (int q = c0 - 1; q <= c0 + 1; q++) {
            if (r < 1 || q < 1 || r > S.gr || q > S.gc) continue;
            const int cb = cell_off[(r - 1) * S.gc + (q - 1)], cn = cell_off[(r - 1) * S.gc + (q - 1) + 1] - cb;
            for (int i = (lane - base % G + G) % G; i < cn; i += G) {   // this lane's slots of the cell: base + i = lane (mod G), ascending
                const int j = cell_kp[cb + i];
                const double d = lmm_candidate(D, S, gm, S.kp0 + j, py, px, X, Y, Z);
                if (d >= 0.0 && d <= best) { best = d; best_slot = base + i; best_j = j; }      // :445: <=, the later slot wins
            }
            base += cn;
        }
    for (int off = G / 2; off > 0; off >>= 1) {
        const double od = __shfl_xor(best, off, G);
        const int os = __shfl_xor(best_slot, off, G), oj = __shfl_xor(best_j, off, G);
        if (od < best || (od == best && os > best_slot)) { best = od; best_slot = os; best_j = oj; }
    }
    if (lane == 0) {
        D.best_kp[gm] = best_j; D.best_dist[gm] = best;
        D.proj[2 * (size_t)gm] = py; D.proj[2 * (size_t)gm + 1] = px;
        if (best_j >= 0)                                                // mapper.jl:370-381 as one order-independent minimum
            atomicMin(D.keys + S.kp0 + best_j, ((unsigned long long)best << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)m));
    }
}

void lmm_launch(slam_ctx *ctx, const LmmDev &D, int max_M, int n_streams)
{
    constexpr int per_block = 256 / LMM_G;
    ProfScope kernel(ctx, "local_map_match_kernel");
    hipLaunchKernelGGL(k_lmm_match<LMM_G>, dim3((max_M + per_block - 1) / per_block, (unsigned)n_streams), dim3(256), 0, ctx->stream, D);
}

static int lmm_run(slam_ctx *ctx, int S, const int32_t *kp_offsets, const int32_t *kf_offsets, const int32_t *mp_offsets, const slam_local_map_args *a)
{
    ARG_TRY(ctx, ctx != nullptr);
    LmmPlan P; std::string err;
    if (!lmm_plan(S, kp_offsets, kf_offsets, mp_offsets, a, P, err)) return slam_fail(ctx, SLAM_ERR_ARG, "slam_local_map_match: %s", err.c_str());
    const double nan = __builtin_nan("");
    for (int j = 0; j < P.Ntot; j++) a->match[j] = -1;
    for (int m = 0; m < P.Mtot; m++) { a->best_kp[m] = -1; a->best_dist[m] = -1.0; a->proj_yx[2 * (size_t)m] = a->proj_yx[2 * (size_t)m + 1] = nan; }
    if (P.active.empty()) return SLAM_OK;                               // nothing to match anywhere: no launch
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    char *h, *d;
    int rc = slam_pinned(ctx, P.total(), (void **)&h);
    if (rc) return rc;
    rc = slam_scratch(ctx, P.total(), (void **)&d);
    if (rc) return rc;
    lmm_emit(P, kp_offsets, kf_offsets, mp_offsets, a, h);
    LmmDev D;
    D.st = (const LmmStream *)(d + P.off[LMM_ST]);
    D.kp_yx = (const double *)(d + P.off[LMM_KP_YX]); D.kp_desc_off = (const int32_t *)(d + P.off[LMM_KP_DOFF]); D.kp_desc = (const uint64_t *)(d + P.off[LMM_KP_DESC]);
    D.kp_obs_off = (const int32_t *)(d + P.off[LMM_KP_OOFF]); D.kp_obs_kf = (const int32_t *)(d + P.off[LMM_KP_OKF]); D.kp_obs_yx = (const double *)(d + P.off[LMM_KP_OYX]);
    D.kf_Tcw = (const double *)(d + P.off[LMM_KF]);
    D.mp_xyz = (const double *)(d + P.off[LMM_MP_XYZ]); D.mp_desc_off = (const int32_t *)(d + P.off[LMM_MP_DOFF]); D.mp_desc = (const uint64_t *)(d + P.off[LMM_MP_DESC]);
    D.mp_obs_off = (const int32_t *)(d + P.off[LMM_MP_OOFF]); D.mp_obs_kf = (const int32_t *)(d + P.off[LMM_MP_OKF]);
    D.cell_off = (const int32_t *)(d + P.off[LMM_CELL_OFF]); D.cell_kp = (const int32_t *)(d + P.off[LMM_CELL_KP]);
    D.best_kp = (int32_t *)(d + P.off[LMM_BEST_KP]); D.best_dist = (double *)(d + P.off[LMM_BEST_DIST]); D.proj = (double *)(d + P.off[LMM_PROJ]);
    D.keys = (unsigned long long *)(d + P.off[LMM_KEYS]);
    { ProfScope span(ctx, "local_map_match");
      HIP_TRY(ctx, hipMemcpyAsync(d, h, P.in_bytes(), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemsetAsync(d + P.off[LMM_KEYS], 0xFF, P.off[LMM_REGIONS] - P.off[LMM_KEYS], ctx->stream));
      lmm_launch(ctx, D, P.max_M, (int)P.active.size());
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(h + P.in_bytes(), d + P.in_bytes(), P.out_bytes(), hipMemcpyDeviceToHost, ctx->stream)); }
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    const int32_t *bk = (const int32_t *)(h + P.off[LMM_BEST_KP]);
    const double *bd = (const double *)(h + P.off[LMM_BEST_DIST]), *pr = (const double *)(h + P.off[LMM_PROJ]);
    const uint64_t *keys = (const uint64_t *)(h + P.off[LMM_KEYS]);
    for (int s : P.active) {                                            // the streams that were not launched keep the defaults set above
        const int m0 = mp_offsets[s], M = mp_offsets[s + 1] - m0, j0 = kp_offsets[s], N = kp_offsets[s + 1] - j0;
        memcpy(a->best_kp + m0, bk + m0, (size_t)M * 4); memcpy(a->best_dist + m0, bd + m0, (size_t)M * 8);
        memcpy(a->proj_yx + 2 * (size_t)m0, pr + 2 * (size_t)m0, (size_t)M * 16);
        for (int j = 0; j < N; j++) a->match[j0 + j] = lmm_decode(keys[j0 + j]);
    }
    return SLAM_OK;
}

extern "C" int slam_local_map_match(slam_ctx *ctx, const slam_local_map_args *args, int N, int K, int M)
{
    ARG_TRY(ctx, ctx != nullptr && N >= 0 && K >= 0 && M >= 0);
    const int32_t kp[2] = {0, N}, kf[2] = {0, K}, mp[2] = {0, M};
    return lmm_run(ctx, 1, kp, kf, mp, args);
}

extern "C" int slam_local_map_match_batch(slam_ctx *ctx, int S, const int32_t *kp_offsets, const int32_t *kf_offsets, const int32_t *mp_offsets,
                                          const slam_local_map_args *args)
{
    return lmm_run(ctx, S, kp_offsets, kf_offsets, mp_offsets, args);
}
