// ba_dev_plan.hpp -- the decisions the two forms of the batched local BA share about a window that k_ba_window solves: which windows that kernel takes
// (ba_window_eligible, ba_free_span), how poses are relabelled so that the free ones are consecutive (ba_relabel_free_last / ba_label_free_last) and where
// the window is split between the kernel's two workgroups (ba_ksplit_*).  Every routine is the one copy: ba_plan / emit_window call it on the host
// (slam_local_ba_batch), k_ba_dev_probe / k_ba_dev_stage on the device (slam_local_ba_batch_dev).  No HIP call, no HIP type: the header compiles as plain
// C++, and tests/c_host/ba_dev_plan_check.cpp holds it to the numpy model (tests/np_ba_dev_stage.py, tests/test_ba_dev_plan_host.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BAP_HD __host__ __device__
#else
#define BAP_HD
#endif

// k_ba_window's limits (ba_device.hpp sizes the kernel's LDS from the same numbers: BW_FMAX, BW_PMAX, BW_OMAX, BW_WOB)
constexpr int BAP_FMAX = 5;          // free poses
constexpr int BAP_PMAX = 128;        // poses
constexpr int BAP_OMAX = 40000;      // observations
constexpr int BAP_CMAX = 168;        // observations of one map point

// the poses the reduced system spans: first .. last FREE pose where there are at least two of them, else every pose (tc[p] != 0: pose p is constant)
BAP_HD static inline void ba_free_span(const uint8_t *tc, int P, int *p0, int *pspan)
{
    int f0 = P, f1 = -1;
    for (int p = 0; p < P; p++) if (!tc[p]) { f0 = f0 < p ? f0 : p; f1 = f1 > p ? f1 : p; }
    if (f1 - f0 + 1 >= 2) { *p0 = f0; *pspan = f1 - f0 + 1; } else { *p0 = 0; *pspan = P; }
}
// the same span once the free poses are the LAST nfree labels (ba_relabel_free_last)
BAP_HD static inline void ba_free_span_relabelled(int P, int nfree, int *p0, int *pspan)
{
    if (nfree >= 2) { *p0 = P - nfree; *pspan = nfree; } else { *p0 = 0; *pspan = P; }
}
// k_ba_window takes the window: a batch call that may use the kernel (`batch`), the grouped route admissible, 1 .. 5 free poses that ARE the free span
// (so one free pose among several is not: its span is every pose), and the kernel's sizes
BAP_HD static inline bool ba_window_eligible(bool batch, bool grouped, int nfree, int pspan, int P, int O, int cmax)
{
    return batch && grouped && nfree >= 1 && nfree <= BAP_FMAX && nfree == pspan && P <= BAP_PMAX && O <= BAP_OMAX && cmax <= BAP_CMAX;
}

// Relabelling: the constant poses first, in the caller's order, then the free ones in the order free_seq[0 .. F) names them (nullptr: the caller's
// order).  order[k] = the caller's pose at the solver's position k.  Returns the number of free poses.
BAP_HD static inline int ba_relabel_free_last(const uint8_t *tc, int P, const int *free_seq, int F, int *order)
{
    int k = 0, nf = 0;
    for (int p = 0; p < P; p++) if (tc[p]) order[k++] = p;
    if (free_seq) { for (int a = 0; a < F; a++) order[k++] = free_seq[a]; return F; }
    for (int p = 0; p < P; p++) if (!tc[p]) { order[k++] = p; nf++; }
    return nf;
}
// the solver's label of the caller's pose p under ba_relabel_free_last(tc, P, nullptr, ..): the inverse of `order`, one pose at a time (a thread per pose)
BAP_HD static inline int ba_label_free_last(const uint8_t *tc, int P, int p)
{
    int nconst = 0, before = 0;
    for (int q = 0; q < P; q++) { const bool same = (tc[q] != 0) == (tc[p] != 0); if (tc[q]) nconst++; if (same && q < p) before++; }
    return tc[p] ? before : nconst + before;
}

// The split point of k_ba_window's two workgroups, by cost: an observation costs the evaluation phases ~24 cycles, an observation of a FREE pose ~6.5
// times that in the Schur phase.  start(k) = first observation of sorted point k, pfs(k) = observations of free poses of the points before k.  Point k
// stays with the first workgroup while twice the cost of the points before it is below the window's; the costs ascend with k, so the number of points
// for which ba_ksplit_before holds IS the first k for which it does not (the device counts, the host walks).
BAP_HD static inline long long ba_ksplit_total(int O, int pfs_M) { return 2LL * O + 13LL * pfs_M; }
BAP_HD static inline bool ba_ksplit_before(long long total, int start_k, int pfs_k) { return 2 * (2LL * start_k + 13LL * pfs_k) < total; }
BAP_HD static inline int ba_ksplit_clamp(int kk, int M) { const int lo = kk > 1 ? kk : 1; return lo < M - 1 ? lo : M - 1; }      // M > 1: both halves hold a point
template <class Start, class Pfs> BAP_HD static inline int ba_ksplit_cost(int M, int O, Start start, Pfs pfs)
{
    const long long total = ba_ksplit_total(O, pfs(M));
    int kk = 0;
    while (kk < M && ba_ksplit_before(total, start(kk), pfs(kk))) kk++;
    return ba_ksplit_clamp(kk, M);
}
// ... and by observation counts alone: the first point whose observations start at or behind the middle one (the value a one-point window keeps)
template <class Start> BAP_HD static inline int ba_ksplit_obs(int M, int O, Start start)
{
    int lo = 0, hi = M + 1;                                   // lower_bound of (O + 1) / 2 in start[0 .. M]
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (start(mid) < (O + 1) / 2) lo = mid + 1; else hi = mid; }
    return lo < M ? lo : M;
}
