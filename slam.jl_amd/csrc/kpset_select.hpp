// kpset_select.hpp -- the selection of slam_kpset_select as the key-frame seams launch from it: the caller's S mask bytes -> the ascending
// table of the selected streams' indices the selected kernel forms read (s = idx[blockIdx]), the mask normalised to 0 / 1, and the number
// of stream slots a launch is sized for.  No HIP calls and no HIP types, so it compiles and runs as plain C++
// (tests/c_host/kpset_select_check.cpp; the rank table and the stale-build check of the compact right batch: tests/c_host/compact_rank_check.cpp).
#pragma once
#include <cstdint>

#define KPSEL_ALL (-1)                /* no selection: every stream, the unselected kernel forms, no table */

// mask: S bytes, non-zero = selected, or nullptr = every stream.  idx (S ints) receives the selected streams ascending, the rest of it
// -1; norm (S bytes) the mask as 0 / 1.  Returns the number of selected streams, or KPSEL_ALL when the mask is null or selects every
// stream -- "all streams selected" IS "no selection": the seams then launch what they launch without one.  S < 1 or a null output: KPSEL_ALL,
// nothing written.
static inline int kpset_select_plan(int S, const uint8_t *mask, int32_t *idx, uint8_t *norm)
{
    if (S < 1 || !idx || !norm) return KPSEL_ALL;
    int n = 0;
    for (int s = 0; s < S; s++) {
        const bool on = !mask || mask[s] != 0;
        norm[s] = on ? 1 : 0;
        if (on) idx[n++] = s;
    }
    for (int i = n; i < S; i++) idx[i] = -1;
    return n == S ? KPSEL_ALL : n;
}

// The inverse of the ascending table: rank[s] = r where idx[r] == s, -1 for an unselected stream (rank: S ints).  A COMPACT right batch
// (slam_pyr_update_batch_sel_*) holds the build of the r-th selected stream in member r, so rank[s] is the member a compact stereo match
// reads stream s's target from.  n_sel as kpset_select_plan returned it: KPSEL_ALL gives the identity.
static inline void kpset_select_rank(int S, const int32_t *idx, int n_sel, int32_t *rank)
{
    if (S < 1 || !idx || !rank) return;
    for (int s = 0; s < S; s++) rank[s] = n_sel == KPSEL_ALL ? s : -1;
    if (n_sel != KPSEL_ALL) for (int r = 0; r < n_sel && r < S; r++) if (idx[r] >= 0 && idx[r] < S) rank[idx[r]] = r;
}
// The stale-build check of a compact stereo match: the mask a batch was last built for (S_built streams, normalised 0 / 1) against the
// set's current selection (S streams, normalised) -- the same streams, stream for stream.  S_built < 1: the batch holds no compact build.
static inline bool kpset_select_same(int S_built, const uint8_t *built, int S, const uint8_t *sel)
{
    if (S_built < 1 || S_built != S || !built || !sel) return false;
    for (int s = 0; s < S; s++) if ((built[s] != 0) != (sel[s] != 0)) return false;
    return true;
}

// the stream dimension of a key-frame seam's launches (grid.y of the per-cell and per-slot kernels, grid.x of the per-stream ones);
// 0: the seam launches nothing
static inline int kpset_select_streams(int S, int n_sel) { return n_sel == KPSEL_ALL ? S : n_sel; }
// the launch bound of the kernels that walk the work list: the selected streams' share of the capacity, the host's bound where it is tighter
static inline int kpset_select_bound(int S, int cap, int n_sel, int n_bound)
{
    const long long nmax = (long long)kpset_select_streams(S, n_sel) * cap;
    return (int)(n_bound > 0 && n_bound < nmax ? n_bound : nmax);
}
