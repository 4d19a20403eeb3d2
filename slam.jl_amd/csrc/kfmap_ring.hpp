// kfmap_ring.hpp -- the integer logic of the key-frame map (kfmap.hip, kfmap_lmm.inc, kfmap_merge.inc): where an id lives, the search in a sorted
// slab, and the serial decisions over the at most 64 slots of a stream's ring that one thread of a 256-thread workgroup takes -- which key-frames form
// the covisibility map, the order in which poses get their ids, which key-frames the filter walks and removes, the replace-or-union rule of the
// local-map history, the one-to-one rule of a merge's pairs.  Every routine is the one copy: the kernels call it from the thread that ran the loop
// before, with their LDS arrays as arguments.  No HIP call, no HIP type: the header compiles as plain C++, and tests/c_host/kfmap_ring_check.cpp holds
// it to the numpy models (tests/test_kfmap_ring_host.py).  tag[b] = key-frame id + 1 of slot b (0: empty), as KfmapView::tag.
#pragma once
#include <climits>
#include <cstdint>

#if defined(__HIPCC__)
#define KFM_HD __host__ __device__
#else
#define KFM_HD
#endif

constexpr int N_COVISIBLE = 5;        // local_bundle_adjustment!: up to 5 latest covisible key-frames (estimator.jl:317-335)

// the table entry of point `id` (ids are non-negative; taken as unsigned, any 64 bits land inside the table)
KFM_HD static inline unsigned long long kfm_entry(int64_t id, int mcap) { return (unsigned long long)id % (unsigned long long)mcap; }
// first index of ids[0 .. n) (ascending) whose id is not below `id`
KFM_HD static inline int kfm_lower(const int64_t *ids, int n, int64_t id)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
    return lo;
}
// index of `id` among the ascending ids[0 .. n), or -1
KFM_HD static inline int kfm_find(const int64_t *ids, int n, int64_t id)
{
    const int lo = kfm_lower(ids, n, id);
    return lo < n && ids[lo] == id ? lo : -1;
}

// rank[b] = rank of slot b by key-frame id among the slots with a tag, asc[rank] = b: the ascending walk of the ring.  Returns their number.
KFM_HD static inline int kfm_rank_slots(const int *tag, int R, int *rank, int *asc)
{
    int nv = 0;
    for (int b = 0; b < R; b++) if (tag[b]) {
        int r = 0;
        for (int c = 0; c < R; c++) r += tag[c] && tag[c] < tag[b];
        rank[b] = r; asc[r] = b; nv++;
    }
    return nv;
}
// sorted(cov, reverse=True)[:5] of the gather: the at most N_COVISIBLE newest slots among r0 and the slots with a score, newest first in cl[];
// mask: their bits.  Returns their number.
KFM_HD static inline int kfm_covmap_pick(const int *tag, const int *cov, int R, int r0, int *cl, unsigned long long &mask)
{
    unsigned long long used = 0;
    int ncl = 0;
    for (int k = 0; k < N_COVISIBLE; k++) {
        int best = -1;
        for (int b = 0; b < R; b++) if (tag[b] && !(used >> b & 1) && (b == r0 || cov[b] > 0) && (best < 0 || tag[b] > tag[best])) best = b;
        if (best < 0) break;
        used |= 1ull << best; cl[ncl++] = best;
    }
    mask = used;
    return ncl;
}
// dense 1-based pose ids in first-encounter order: the slots without a pose id (order[b] == 0) that a phase met (first[b] != INT_MAX: the index of
// their first observation) take the ids P + 1, P + 2, .. by ascending first[]; first[] is reset
KFM_HD static inline void kfm_assign_poses(int *order, int *first, int R, int &P)
{
    for (;;) {
        int best = -1;
        for (int b = 0; b < R; b++) if (order[b] == 0 && first[b] != INT_MAX && (best < 0 || first[b] < first[best])) best = b;
        if (best < 0) break;
        order[best] = ++P; first[best] = INT_MAX;
    }
}
// theta_const of a window's pose: key-frame 0, a key-frame outside the covisibility map, or one whose score is below min_cov_score
KFM_HD static inline bool kfm_window_const(int tag_b, bool in_covmap, int cov_b, int minc) { return tag_b == 1 || !in_covmap || cov_b < minc; }

// the filter's walk: the covisible slots (a tag, a score, not r0) ascending by key-frame id into cand[]; key-frame 0 ends the walk
// (`kfid == 0 && break`), an id >= the newest (kfid) is passed over.  valid: the slots with a tag.  Returns the number of candidates.
KFM_HD static inline int kfm_filter_candidates(const int *tag, const int *cov, int R, int r0, int kfid, int *cand, unsigned long long &valid)
{
    unsigned long long used = 0, v = 0;
    int n = 0;
    for (int b = 0; b < R; b++) if (tag[b]) v |= 1ull << b;
    for (;;) {
        int best = -1;
        for (int b = 0; b < R; b++) if (b != r0 && tag[b] && cov[b] > 0 && !(used >> b & 1) && (best < 0 || tag[b] < tag[best])) best = b;
        if (best < 0 || tag[best] == 1) break;
        used |= 1ull << best;
        if (tag[best] - 1 < kfid) cand[n++] = best;
    }
    valid = v;
    return n;
}
// map_filtering!'s decision: fewer than `few` 3-D points, or n_good / n_total > ratio in doubles (0 / 0 is NaN: kept)
KFM_HD static inline bool kfm_filter_removes(int n_total, int n_good, int few, double ratio) { return n_total < few || (double)n_good / (double)n_total > ratio; }

// the local-map history: the covisible slot of the smallest key-frame id, or -1
KFM_HD static inline int kfm_oldest_covisible(unsigned long long covmask, const int *tag)
{
    int oldest = -1;
    for (unsigned long long cm = covmask; cm; cm &= cm - 1) { const int b = __builtin_ctzll(cm); if (oldest < 0 || tag[b] < tag[oldest]) oldest = b; }
    return oldest;
}
// triangulate_temporal!'s get_observers(mp)[1] (mapper.jl:214-216): among the bits of `mask` that mean something (below R, their slot with a tag) the slot
// of the smallest key-frame id; -1 where fewer than two bits mean something (`length(observers) < 2 && continue`)
KFM_HD static inline int kfm_first_observer(unsigned long long mask, const int *tag, int R)
{
    int first = -1, n = 0;
    for (unsigned long long mm = mask; mm; mm &= mm - 1) {
        const int b = __builtin_ctzll(mm);
        if (b < R && tag[b]) { n++; if (first < 0 || tag[b] < tag[first]) first = b; }
    }
    return n >= 2 ? first : -1;
}
// map_manager.jl:350-354 and mapper.jl:274-286 on the sizes nC = |C|, nP = |P|, nU = |P | C|: replace: L = C (len(C) > 0.5 len(P), exact in integers),
// else L = P | C; chain: the oldest covisible key-frame's set is united in (a covisible key-frame, |L| < max_local, that slot's set its own).
// Returns |L| before the chain.
KFM_HD static inline int kfm_history_rule(int nC, int nP, int nU, unsigned long long covmask, bool linked, int max_local, bool &replace, bool &chain)
{
    replace = 2 * nC > nP;
    const int size = replace ? nC : nU;
    chain = covmask != 0 && size < max_local && linked;
    return size;
}

// A merge's pairs (prev_id, new_id), pairs[2 t], pairs[2 t + 1], are one-to-one: no prev id twice, no new id twice, no id on both sides of two pairs (a
// pair of one id is skipped by the validity rule, not refused).  kfm_pair_clashes: pair t against the others (the device's form, one thread per pair);
// kfm_pairs_one_to_one: no pair clashes.
KFM_HD static inline bool kfm_pair_clashes(const int64_t *pairs, int n, int t)
{
    const int64_t a = pairs[2 * t], b = pairs[2 * t + 1];
    bool bad = false;
    for (int u = 0; u < n; u++) if (u != t) { const int64_t a2 = pairs[2 * u], b2 = pairs[2 * u + 1]; bad |= a2 == a || b2 == b || a2 == b; }
    return bad;
}
KFM_HD static inline bool kfm_pairs_one_to_one(const int64_t *pairs, int n)
{
    for (int t = 0; t < n; t++) if (kfm_pair_clashes(pairs, n, t)) return false;
    return true;
}
// the same rule in n log n for the host, on the ids the caller has sorted: prev[0 .. n) and neu[0 .. n) ascending, both[0 .. nb) the ids of the pairs
// of two different ids, ascending -- a repeat in any of the three is a clash
KFM_HD static inline bool kfm_sorted_one_to_one(const int64_t *prev, const int64_t *neu, int n, const int64_t *both, int nb)
{
    for (int i = 1; i < n; i++) if (prev[i] == prev[i - 1] || neu[i] == neu[i - 1]) return false;
    for (int i = 1; i < nb; i++) if (both[i] == both[i - 1]) return false;
    return true;
}

// ---- the descriptor rows of a map point (slam_kfmap_enable_descriptor_rows): keyframes_descriptors (map_point.jl:15), one 256-bit row per key-frame id,
// bounded: D slots per point, key[j] = key-frame id + 1 (0: an empty slot), row[4 j .. 4 j + 4) its row.  Slots may have holes; readers take the
// non-empty slots ascending by key (kfm_rows_next).  tests/c_host/kfmap_rows_check.cpp holds these to tests/np_kfmap_rows.py.
constexpr int KFM_MAX_ROWS = 8;
// the slot that holds `key`, or -1
KFM_HD static inline int kfm_rows_find(const int32_t *key, int D, int32_t k)
{
    for (int j = 0; j < D; j++) if (key[j] == k) return j;
    return -1;
}
// remove_kf_observation!'s pop!(keyframes_descriptors, kfid): the slot of `k` is emptied; false where no slot holds it
KFM_HD static inline bool kfm_rows_drop(int32_t *key, int D, int32_t k)
{
    const int j = k > 0 ? kfm_rows_find(key, D, k) : -1;
    if (j >= 0) key[j] = 0;
    return j >= 0;
}
// empty!(keyframes_descriptors)
KFM_HD static inline void kfm_rows_clear(int32_t *key, int D) { for (int j = 0; j < D; j++) key[j] = 0; }
// the number of rows
KFM_HD static inline int kfm_rows_count(const int32_t *key, int D)
{
    int n = 0;
    for (int j = 0; j < D; j++) n += key[j] != 0;
    return n;
}
// the walk ascending by key: the slot of the smallest key above `after` (0 to start), or -1 (keys are unique within a point)
KFM_HD static inline int kfm_rows_next(const int32_t *key, int D, int32_t after)
{
    int best = -1;
    for (int j = 0; j < D; j++) if (key[j] > after && (best < 0 || key[j] < key[best])) best = j;
    return best;
}
// add_descriptor! (map_point.jl:124-131) under the bound: a key the point already has is skipped; else the row takes an empty slot; with no slot left
// the row of the SMALLEST key among the D + 1 goes (the arriving one, if that is it).  Returns the rows dropped by the bound: 0 or 1.
KFM_HD static inline int kfm_rows_put(int32_t *key, uint64_t *row, int D, int32_t k, const uint64_t *r)
{
    int freej = -1, minj = 0;
    for (int j = 0; j < D; j++) {
        if (key[j] == k) return 0;
        if (key[j] == 0) { if (freej < 0) freej = j; }
        else if (key[minj] == 0 || key[j] < key[minj]) minj = j;
    }
    int j = freej;
    if (j < 0) { if (k < key[minj]) return 1; j = minj; }
    key[j] = k;
    for (int w = 0; w < 4; w++) row[4 * j + w] = r[w];
    return freej < 0;
}
// merge_mappoints' copy (map_manager.jl:410-412): every row of prev into the survivor, an equal key keeps the survivor's row; more than D keys: the D
// LARGEST stay, whatever the order of the slots (evicting the smallest key one arrival at a time leaves the largest D).  Returns the rows dropped: the
// size of the union of the keys less D -- counted on the keys, not on the evictions, whose number depends on the slots' order where a key is equal.
KFM_HD static inline int kfm_rows_union(int32_t *key, uint64_t *row, const int32_t *pkey, const uint64_t *prow, int D)
{
    int n = kfm_rows_count(key, D);
    for (int j = 0; j < D; j++) n += pkey[j] && kfm_rows_find(key, D, pkey[j]) < 0;
    for (int j = 0; j < D; j++) if (pkey[j]) (void)kfm_rows_put(key, row, D, pkey[j], prow + 4 * j);
    return n > D ? n - D : 0;
}
