// kpset_select.hpp -- the selection of slam_kpset_select as the key-frame seams launch from it: the caller's S mask bytes -> the ascending
// table of the selected streams' indices the selected kernel forms read (s = idx[blockIdx]), the mask normalised to 0 / 1, and the number
// of stream slots a launch is sized for.  No HIP calls and no HIP types, so it compiles and runs as plain C++
// (tests/c_host/kpset_select_check.cpp).
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

// the stream dimension of a key-frame seam's launches (grid.y of the per-cell and per-slot kernels, grid.x of the per-stream ones);
// 0: the seam launches nothing
static inline int kpset_select_streams(int S, int n_sel) { return n_sel == KPSEL_ALL ? S : n_sel; }
// the launch bound of the kernels that walk the work list: the selected streams' share of the capacity, the host's bound where it is tighter
static inline int kpset_select_bound(int S, int cap, int n_sel, int n_bound)
{
    const long long nmax = (long long)kpset_select_streams(S, n_sel) * cap;
    return (int)(n_bound > 0 && n_bound < nmax ? n_bound : nmax);
}
