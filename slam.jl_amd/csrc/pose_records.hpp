// pose_records.hpp -- the result records of the pose seams (P3P RANSAC, five-point RANSAC, single-pose refinement) and the two conversions between
// a pose and its RotZYX angles, ONE definition of each for the kernels that write them and the host code that reads them (pose.hip, fivepoint.hip,
// ba_single.hip).  The records' bytes are part of no ABI, but both sides of a mapped block must agree on them: the static_asserts hold the offsets.
// Host/device like ba_math.hpp: no HIP call, no common.hpp -- tests/c_host/pose_records_check.cpp includes this header alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PR_HD __host__ __device__ __forceinline__
#else
#define PR_HD static inline
#endif

// k_p3p_select's record of one problem: K [R | t] and [R | t] (column-major 3 x 4), the summed inlier error, the winner's inlier count and iteration
struct P3POut { double KP[12], Rt[12], err; int32_t n_inliers, best_iter /* -1: no hypothesis had an inlier */; unsigned char pad[48]; };
static_assert(offsetof(P3POut, KP) == 0 && offsetof(P3POut, Rt) == 96 && offsetof(P3POut, err) == 192 && offsetof(P3POut, n_inliers) == 200 &&
              offsetof(P3POut, best_iter) == 204 && sizeof(P3POut) == 256, "P3POut: KP 0 | Rt 96 | err 192 | n_inliers 200 | best_iter 204, 256 bytes");

// k_5pt_select's record: [R | t] (column-major 3 x 4), E (column-major 3 x 3), the summed inlier error, the winner's inlier count and iteration
struct FPOut { double P[12], E[9], err; int32_t n_inliers, best_iter; unsigned char pad[72]; };
static_assert(offsetof(FPOut, P) == 0 && offsetof(FPOut, E) == 96 && offsetof(FPOut, err) == 168 && offsetof(FPOut, n_inliers) == 176 &&
              offsetof(FPOut, best_iter) == 180 && sizeof(FPOut) == 256, "FPOut: P 0 | E 96 | err 168 | n_inliers 176 | best_iter 180, 256 bytes");

// k_pnp / k_pnp_batch's record: the refined angles and translation, the summed squared residuals before and after, and four counts kept as doubles
// (identity != 0: fewer than 5 inliers were left after the first pass -- the caller answers with the identity pose)
struct PnPResult { double X[6], err_init, err_final, n_outliers, identity, iters1, iters2; unsigned char pad[32]; };
static_assert(offsetof(PnPResult, X) == 0 && offsetof(PnPResult, err_init) == 48 && offsetof(PnPResult, err_final) == 56 &&
              offsetof(PnPResult, n_outliers) == 64 && offsetof(PnPResult, identity) == 72 && offsetof(PnPResult, iters1) == 80 &&
              offsetof(PnPResult, iters2) == 88 && sizeof(PnPResult) == 128, "PnPResult: X 0 | 48 56 64 72 80 88, 128 bytes");

// X = (theta1, theta2, theta3, t) -> the rotation RotZYX(theta1, theta2, theta3) and the translation of a column-major 4 x 4 pose T; the bottom
// row (and the identity a caller answers with instead) is the caller's.  Products associate left to right: (c1 * s2) * s3 - s1 * c3.
PR_HD void angles_to_pose(const double X[6], double T[16])
{
    const double s1 = sin(X[0]), c1 = cos(X[0]), s2 = sin(X[1]), c2 = cos(X[1]), s3 = sin(X[2]), c3 = cos(X[2]);
    const double R[9] = {c1 * c2, c1 * s2 * s3 - s1 * c3, c1 * s2 * c3 + s1 * s3, s1 * c2, s1 * s2 * s3 + c1 * c3, s1 * s2 * c3 - c1 * s3, -s2, c2 * s3, c2 * c3};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[i + 4 * j] = R[3 * i + j];
    T[12] = X[3]; T[13] = X[4]; T[14] = X[5];
}

// RotZYX(R).theta1..3 (Rotations.jl; get_cw_ba, frame.jl:432-437) of a column-major rotation with column pitch LD (R[i][j] = M[i + LD j]: 4 for a
// 4 x 4 pose, 3 for [R | t]) and the translation t
template <int LD> PR_HD void pose_to_angles(const double *M, const double *t, double X[6])
{
    const double R11 = M[0], R21 = M[1], R31 = M[2], R12 = M[LD], R22 = M[LD + 1], R13 = M[2 * LD], R23 = M[2 * LD + 1];
    const double t1 = atan2(R21, R11), s1 = sin(t1), c1 = cos(t1);
    X[0] = t1; X[1] = atan2(-R31, sqrt(R11 * R11 + R21 * R21)); X[2] = atan2(R13 * s1 - R23 * c1, R22 * c1 - R12 * s1);
    X[3] = t[0]; X[4] = t[1]; X[5] = t[2];
}
