// kf_host.hpp -- check_new_kf_required (src/front_end.jl:361-393) for S lock-stepped streams, on the per-stream statistics that
// slam_kpset_frame_stats (kpset.hip) reduces from the device-resident lists.  No HIP calls and no HIP types, so it compiles and runs as
// plain C++ (tests/c_host/kf_decide_check.cpp).
#pragma once
#include <cstdint>

#define KF_STATS 8                    /* = SLAM_KF_STATS of include/slamhip.h: doubles per stream */
enum { KF_N = 0, KF_N3D, KF_NSTEREO, KF_NHASKF, KF_CELLS, KF_NPAR, KF_MEAN, KF_MEDIAN };
// which exit decided (the `rule` output)
enum { KF_RULE_NO_PREV = 0, KF_RULE_SPARSE_CELLS, KF_RULE_FEW_3D, KF_RULE_ENOUGH_3D, KF_RULE_PARALLAX };

// One stream.  Every comparison is the reference's, in doubles, with its products (0.33 * max_nb_keypoints ...) formed as it forms them -- no
// integer rewrite: 0.33 * 1000 rounds to 330.0, so 329 occupied cells are "sparse" there and 330 are not.  A NaN median fails both >= tests.
static inline bool kf_required_one(const double *st, int frames_delta, int prev_kf_nb_3d, bool has_prev_kf, int max_nb_keypoints, double initial_parallax,
                                   bool local_ba_on, uint8_t *rule)
{
    if (!has_prev_kf) { *rule = KF_RULE_NO_PREV; return false; }                                                                   // :362-363
    const double cells = st[KF_CELLS], nb_3d = st[KF_N3D], median = st[KF_MEDIAN], maxkp = (double)max_nb_keypoints;
    if (cells < 0.33 * maxkp && frames_delta >= 5 && !local_ba_on) { *rule = KF_RULE_SPARSE_CELLS; return true; }                  // :367-370
    if (nb_3d < 20.0 && frames_delta >= 2) { *rule = KF_RULE_FEW_3D; return true; }                                                // :371-373
    if (nb_3d > 0.5 * maxkp && (local_ba_on || frames_delta < 2)) { *rule = KF_RULE_ENOUGH_3D; return false; }                     // :374-377
    const bool cx = median >= initial_parallax / 2.0;                                                                             // :385
    const bool c0 = median >= initial_parallax;                                                                                   // :386
    const bool c1 = nb_3d < 0.75 * (double)prev_kf_nb_3d;                                                                         // :387
    const bool c2 = cells < 0.5 * maxkp && nb_3d < 0.85 * (double)prev_kf_nb_3d && !local_ba_on;                                  // :388-390
    *rule = KF_RULE_PARALLAX;
    return cx && (c0 || c1 || c2);                                                                                                // :392
}

// S streams; stats: S x KF_STATS as slam_kpset_frame_stats returns them with flags = 1.  false: a null array or S < 1, nothing written.
static inline bool kf_required(int S, const double *stats, const int32_t *frames_delta, const int32_t *prev_kf_nb_3d, const uint8_t *has_prev_kf,
                               int max_nb_keypoints, double initial_parallax, int local_ba_on, uint8_t *required, uint8_t *rule)
{
    if (S < 1 || !stats || !frames_delta || !prev_kf_nb_3d || !has_prev_kf || !required) return false;
    for (int s = 0; s < S; s++) {
        uint8_t r = 0;
        required[s] = kf_required_one(stats + (long)KF_STATS * s, frames_delta[s], prev_kf_nb_3d[s], has_prev_kf[s] != 0, max_nb_keypoints, initial_parallax,
                                      local_ba_on != 0, &r) ? 1 : 0;
        if (rule) rule[s] = r;
    }
    return true;
}
