// geom_device.hpp -- the one copy of every device routine that the front-end geometry seams share (pose.hip, fivepoint.hip,
// triangulate.hip, kpset.hip, detect.hip, lk.hip): the sample generator, the lens model, the two-view DLT with the mapper's gates,
// the per-problem range, the ordered compactions and the winner selection of the two RANSACs.
#pragma once
#include "tri_device.hpp"
#include <cstdint>
#include <cstring>

// ---- counter-based sample generator (restated by keypoint_set.py) ------------------------------------------------------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// K distinct indices below n (n >= K) for iteration `it` of stream z: splitmix64 of seed, stream, iteration, attempt; the attempt
// counter runs on across the K draws
template <int K>
__device__ __forceinline__ void draw_distinct(unsigned long long seed, int z, int it, int n, int *idx)
{
    unsigned att = 0;
    for (int k = 0; k < K; k++) {
        for (;;) {
            const unsigned long long h = splitmix64(seed ^ ((unsigned long long)z << 48) ^ ((unsigned long long)it << 16) ^ (unsigned long long)att);
            att++;
            const int c = (int)(h % (unsigned long long)n);
            bool dup = false;
            for (int m = 0; m < k; m++) dup = dup || idx[m] == c;
            if (!dup) { idx[k] = c; break; }
        }
    }
}

// ---- lens model (camera.jl:98-125); cam = fx, fy, cx, cy; dist = k1, k2, p1, p2 -----------------------------------------------------
// undistort_pdn_point (camera.jl:111-125): normalised (y, x) -> pixel through the lens model
__device__ __forceinline__ void pdn_to_pixel(const double *cam, const double *dist, double ny, double nx, double &oy, double &ox)
{
    const double s0 = ny * ny, s1 = nx * nx, r2 = s0 + s1;
    const double rd = 1.0 + dist[0] * r2 + dist[1] * (r2 * r2);
    const double p = ny * nx;
    const double dtx = 2 * dist[2] * p + dist[3] * (r2 + 2 * s0);
    const double dty = dist[2] * (r2 + 2 * s1) + 2 * dist[3] * p;
    oy = (rd * ny + dty) * cam[1] + cam[3]; ox = (rd * nx + dtx) * cam[0] + cam[2];
}
// undistort_point (camera.jl:98-103): pixel (y, x) -> undistorted pixel
__device__ __forceinline__ void undistort_px(const double *cam, const double *dist, double y, double x, double &uy, double &ux)
{
    pdn_to_pixel(cam, dist, (y - cam[3]) / cam[1], (x - cam[2]) / cam[0], uy, ux);
}
// project(camera, R * (bx, by, 1)) -> pixel (qy, qx): the rotation-compensated position of the parallax terms (front_end.jl:277-279,
// :436-438; mapper.jl:236-237).  R column-major with column stride LD: 3 for R_compensation, 4 for the rotation of a 4 x 4 pose
template <int LD>
__device__ __forceinline__ void rotate_project(const double *R, const double *cam, double bx, double by, double &qy, double &qx)
{
    const double rx = (R[0] * bx + R[LD] * by) + R[2 * LD] * 1.0, ry = (R[1] * bx + R[LD + 1] * by) + R[2 * LD + 1] * 1.0,
                 rz = (R[2] * bx + R[LD + 2] * by) + R[2 * LD + 2] * 1.0;
    qy = cam[1] * ry / rz + cam[3]; qx = cam[0] * rx / rz + cam[2];
}

// ---- two-view DLT and the mapper's gates ---------------------------------------------------------------------------------------------
// the five matrices of a triangulation call, as the host hands them over: column-major 4 x 4 (Julia SMatrix) and fx, fy, cx, cy
struct TwoViewMats {
    double P1[16], P2[16], T21[16], cam1[4], cam2[4];
    void fill(const double *p1, const double *p2, const double *t21, const double *c1, const double *c2)
    {
        memcpy(P1, p1, sizeof P1); memcpy(P2, p2, sizeof P2); memcpy(T21, t21, sizeof T21); memcpy(cam1, c1, sizeof cam1); memcpy(cam2, c2, sizeof cam2);
    }
};
// RecoverPose.triangulate: homogeneous point = eigenvector of A'A for its smallest eigenvalue, divided by its fourth coordinate
__device__ __forceinline__ void dlt_two_view(double x1, double y1, double x2, double y2, const double *P1, const double *P2, double *L)
{
    double A[16], S[16], v[4];
    for (int j = 0; j < 4; j++) {
        A[0 + j] = x1 * P1[2 + 4 * j] - P1[0 + 4 * j];
        A[4 + j] = y1 * P1[2 + 4 * j] - P1[1 + 4 * j];
        A[8 + j] = x2 * P2[2 + 4 * j] - P2[0 + 4 * j];
        A[12 + j] = y2 * P2[2 + 4 * j] - P2[1 + 4 * j];
    }
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc += A[4 * k + r] * A[4 * k + c];
            S[4 * r + c] = acc;
        }
    sym4_min_eigvec(S, v);
    const double iw = 1.0 / v[3];
    L[0] = v[0] * iw; L[1] = v[1] * iw; L[2] = v[2] * iw; L[3] = v[3] * iw;
}
// both depth gates, then both reprojection gates (mapper.jl:160-176, 239-258); a failed gate counts only where `gated`
__device__ __forceinline__ bool two_view_gates(const double *L, const double *T21, const double *cam1, const double *cam2,
                                               double x1, double y1, double x2, double y2, double max_error, double min_depth, bool gated)
{
    bool ok = !(L[2] < min_depth && gated);
    double R[3];
    for (int r = 0; r < 3; r++) R[r] = ((T21[r] * L[0] + T21[r + 4] * L[1]) + T21[r + 8] * L[2]) + T21[r + 12] * L[3];
    if (ok && R[2] < min_depth && gated) ok = false;
    if (ok) {
        const double iz = 1.0 / L[2];
        const double py = cam1[1] * L[1] * iz + cam1[3], px = cam1[0] * L[0] * iz + cam1[2];
        const double dy = y1 - py, dx = x1 - px;
        if (sqrt(dy * dy + dx * dx) > max_error && gated) ok = false;
    }
    if (ok) {
        const double iz = 1.0 / R[2];
        const double py = cam2[1] * R[1] * iz + cam2[3], px = cam2[0] * R[0] * iz + cam2[2];
        const double dy = y2 - py, dx = x2 - px;
        if (sqrt(dy * dy + dx * dx) > max_error && gated) ok = false;
    }
    return ok;
}

// The per-pair body of triangulate_temporal! (mapper.jl:236-259), the one copy of k_kpset_tri_temporal (kpset.hip) and k_kfm_tri_temporal (kfmap_tri.inc):
// (y1, x1) = obup, the first observer's undistorted pixel, (y2, x2) = kpup, the frame's; E = the observer's 64 doubles, column-major 4 x 4 each:
// P2 = K * rel_pose_inv | rel_pose_inv | rel_pose = observer.cw * frame.wc | observer.wc.  A failed gate counts only when the rotation-compensated
// parallax exceeds min_parallax.  Returns the verdict; accepted: W = observer.wc * X (project_camera_to_world(observer_kf, .)).
__device__ __forceinline__ bool temporal_pair(const double *cam, const double *E, double y1, double x1, double y2, double x2,
                                              double max_error, double min_depth, double min_parallax, double *W)
{
    const double *P2 = E, *T21 = E + 16, *REL = E + 32, *WOB = E + 48;
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    double qy, qx;
    // parallax = |obup - project(camera, R(rel_pose) * kp.position)|, :236-237
    rotate_project<4>(REL, cam, (x2 - cx) / fx, (y2 - cy) / fy, qy, qx);
    const double pdy = y1 - qy, pdx = x1 - qx;
    const bool gated = sqrt(pdy * pdy + pdx * pdx) > min_parallax;
    // P1 = K * I
    const double P1[16] = {fx, 0, 0, 0, 0, fy, 0, 0, cx, cy, 1, 0, 0, 0, 0, 1};
    double L[4];
    dlt_two_view(x1, y1, x2, y2, P1, P2, L);
    const bool ok = two_view_gates(L, T21, cam, cam, x1, y1, x2, y2, max_error, min_depth, gated);
    if (ok) for (int r = 0; r < 3; r++) W[r] = ((WOB[r] * L[0] + WOB[r + 4] * L[1]) + WOB[r + 8] * L[2]) + WOB[r + 12] * L[3];
    return ok;
}

// ---- per-problem range of the RANSAC argument blocks: problem z owns [off[z], off[z + 1]), or, in the keypoint-set layout
// (cnt != nullptr), [z * stride, z * stride + cnt[z]) ----------------------------------------------------------------------------------
struct ProblemRange { int base, n; };
__device__ __forceinline__ ProblemRange problem_range(const int *off, const int *cnt, int stride, int z)
{
    const int base = cnt ? z * stride : off[z];
    return {base, cnt ? cnt[z] : off[z + 1] - base};
}

// ---- ordered compactions --------------------------------------------------------------------------------------------------------------
// 256 threads: ordered compaction of a stream's flagged elements: returns this thread's output position (or -1), advances *s_base
__device__ __forceinline__ int ordered_slot(bool take, int *s_w, int *s_base)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long m = __ballot(take);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wv] = __popcll(m);
    __syncthreads();
    int off = *s_base;
    for (int w = 0; w < wv; w++) off += s_w[w];
    const int pos = take ? off + before : -1;
    __syncthreads();
    if (tid == 0) *s_base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return pos;
}
// 1024 threads, one count each (detection cells, row-major): wave-level inclusive scans (shuffle) + one LDS hop across the 16 waves;
// returns where this thread's `cnt` elements start, advances *s_base by the chunk's total
__device__ __forceinline__ int cell_scan(int cnt, int *s_w, int *s_base)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int wbase = 0;
    for (int i = 0; i < wv; i++) wbase += s_w[i];
    int total = 0;
    for (int i = 0; i < 16; i++) total += s_w[i];
    const int start = *s_base + wbase + incl - cnt;
    __syncthreads();
    if (tid == 0) *s_base += total;
    __syncthreads();
    return start;
}

// ---- winner selection of a RANSAC, one workgroup of P::THREADS per problem ------------------------------------------------------------
// counts: the problem's ne candidate counts (P::PER_ITER per iteration).  Winner = most inliers, ties to the lower index; one re-score
// pass writes the inlier mask and the per-element error (LDS, or `errs` above P::ERR_LDS elements); thread 0 sums the errors in
// index order and hands (count, winner, sum) to the policy's writer.  The policy supplies stage(tid) (per-stream constants -> LDS),
// winner(tid, best, be) (the winning hypothesis -> LDS), score(i, err) -> inlier, and write(best, be, esum).
template <class P>
__device__ __forceinline__ void ransac_select(const P &pol, const int *counts, int ne, int n, double *errs, uint8_t *inliers)
{
    __shared__ int s_cnt[P::THREADS], s_idx[P::THREADS];
    __shared__ double s_err[P::ERR_LDS];
    const int tid = threadIdx.x;
    const bool in_lds = n <= P::ERR_LDS;
    pol.stage(tid);
    int bc = 0, bi = -1;
    for (int e = tid; e < ne; e += P::THREADS) {
        const int c = counts[e];
        if (c > bc) { bc = c; bi = e; }        // ascending e: the first maximum is kept
    }
    s_cnt[tid] = bc; s_idx[tid] = bi;
    __syncthreads();
    for (int o = P::THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const int c2 = s_cnt[tid + o], i2 = s_idx[tid + o];
            if (c2 > s_cnt[tid] || (c2 == s_cnt[tid] && c2 > 0 && i2 < s_idx[tid])) { s_cnt[tid] = c2; s_idx[tid] = i2; }
        }
        __syncthreads();
    }
    const int best = s_cnt[0], be = s_idx[0];
    pol.winner(tid, best, be);
    __syncthreads();
    for (int i = tid; i < n; i += P::THREADS) {
        double e = 0.0;
        const bool in = best > 0 && pol.score(i, e);
        inliers[i] = in ? 1 : 0;
        if (in_lds) s_err[i] = in ? e : 0.0; else errs[i] = in ? e : 0.0;   // + 0.0 leaves the sum unchanged
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double esum = 0.0;
        if (in_lds) {
#pragma unroll 16
            for (int i = 0; i < n; i++) esum += s_err[i];             // index order; the reads pipeline, the adds are the chain
        } else {
#pragma unroll 16
            for (int i = 0; i < n; i++) esum += errs[i];
        }
        pol.write(best, be, esum);
    }
}
