// kfmap.hip -- the key-frame map of S lock-stepped streams in HBM (kfmap.hpp has the layout): filled from the keypoint lists (slam_kfmap_add_keyframe),
// it emits the local-BA windows of the streams' newest key-frames in slam_local_ba_batch's layout (slam_kfmap_ba_gather) and takes the solution back, into
// the map and optionally into the live lists (slam_kfmap_ba_update).  slam_kfmap_local_ba is the three in one call with the windows kept in HBM (emit into the map's own
// block, slam_local_ba_batch_dev, the update kernels on the same arrays).  The semantics are _get_ba_parameters / _update_ba_parameters!
// (src/estimator.jl:143-306) as tests/tracked_ba.py restates them, bounded by the ring and the table (tests/np_kfmap.py is the bounded model).
// slam_kfmap_filter is map_filtering! (src/estimator.jl:358-406) on the same map, slam_kfmap_remove_keyframe the remove_keyframe! it calls
// (src/map_manager.jl:184-209); tests/np_kfmap_filter.py is their model.  The descriptor store and slam_kfmap_local_map_match (update_frame_covisibility! +
// match_local_map!, staged on the device for localmap.hip's match kernel) are in kfmap_lmm.inc, included at the end: they use the routines below.
// slam_kfmap_merge (merge_matches -> merge_mappoints -> update_keypoint!: the match's pairs applied in HBM, the touched slabs and lists rebuilt in id
// order) is in kfmap_merge.inc, included behind it; slam_kfmap_triangulate_temporal (triangulate_temporal! from the map's own observers and refined poses) in
// kfmap_tri.inc, behind that.  The integer logic -- where an id lives, the search in a slab, every serial decision over a ring's slots --
// is kfmap_ring.hpp's, host and device (tested on the CPU); the routines every kernel shares (kfm_owned, kfm_slab_point, kfm_each_observer, kfm_live_observers,
// kfm_tcw) and every host seam shares (kfmap_upload, kfmap_alloc_zeroed, kfmap_put_streams) are below, one copy each.
//
// Every kernel takes `sel`: nullptr = workgroup (or grid row) b works on stream b, else on stream sel[b] -- launches are sized by the number of streams
// acted on, so nothing of any other stream is read or written.
#include "kfmap.hpp"
#include <algorithm>
#include <climits>
#include <cmath>

#define KFM_STREAM(b) (sel ? sel[b] : (int)(b))
// THE ownership test: entry pe carries point `id` (dead or alive); kfm_valid: and the point has not been removed
__device__ __forceinline__ bool kfm_owned(const KfmapView &V, size_t pe, int64_t id) { return V.ptag[pe] == (unsigned long long)id + 1ull; }
__device__ __forceinline__ bool kfm_valid(const KfmapView &V, size_t pe, int64_t id) { return kfm_owned(V, pe, id) && !(V.pflags[pe] & KFM_DEAD); }
// observation i of slot b's slab of stream s (i < the slab's length): false for a tombstone, else its id and its point's table entry -- the caller's own
// gate (kfm_owned, kfm_valid, 3-D, descriptor) follows
__device__ __forceinline__ bool kfm_slab_point(const KfmapView &V, int s, int b, int i, int64_t &id, size_t &pe)
{
    const size_t q = ((size_t)s * V.R + b) * V.cap + i;
    if (!V.klive[q]) return false;
    id = V.kid[q]; pe = (size_t)s * V.mcap + kfm_entry(id, V.mcap);
    return true;
}
// the live observation of `id` in slot b's slab of stream s, or -1
__device__ __forceinline__ int kfm_find_live(const KfmapView &V, int s, int b, int64_t id)
{
    const size_t sl = ((size_t)s * V.R + b) * V.cap;
    const int i = kfm_find(V.kid + sl, min(V.kn[s * V.R + b], V.cap), id);
    return i >= 0 && V.klive[sl + i] ? i : -1;
}
// THE observer-mask walk: f(b) for the bits of `mask` that mean something -- below R, their slot with a tag (tag: the stream's R tags, the map's or a copy in
// LDS) -- in ascending slot order
template <class F> __device__ __forceinline__ void kfm_each_observer(unsigned long long mask, const int *tag, int R, F f)
{
    for (unsigned long long mm = mask; mm; mm &= mm - 1) { const int b = __ffsll((long long)mm) - 1; if (b < R && tag[b]) f(b); }
}
// of those, the slots whose slab still holds `id` alive (an observer whose key-frame or pixel is gone does not count)
__device__ __forceinline__ unsigned long long kfm_live_observers(const KfmapView &V, int s, unsigned long long mask, const int *tag, int64_t id)
{
    unsigned long long wm = 0;
    kfm_each_observer(mask, tag, V.R, [&](int b) { if (kfm_find_live(V, s, b, id) >= 0) wm |= 1ull << b; });
    return wm;
}
// Tcw of a key-frame from its six parameters: angles_to_pose and the bottom row 0 0 0 1 (column-major 4 x 4)
__device__ __forceinline__ void kfm_tcw(const double *theta, double *T) { angles_to_pose(theta, T); T[3] = 0.0; T[7] = 0.0; T[11] = 0.0; T[15] = 1.0; }

// Kernels that clear an observer bit come as <bool ROWS>; <true>: the row store is on and they take the whole view (KfmapRows), <false>: the kernel as it
// always was, on the KfmapView.
// The row store's share of remove_kf_observation! (map_point.jl:88-122) for entry pe, which has just lost the observer of key-frame `key` - 1 and keeps the
// observers `left`: the row under that key goes; with no valid observer left every row goes and the point is no longer described.  A thread zeroes its
// own key's slot alone; the clear-all belongs to the one thread whose update left no observer (several slabs may lose one point in the filter's closing pass).
__device__ __forceinline__ void kfm_rows_lost(const KfmapRows &V, int s, size_t pe, int32_t key, unsigned long long left)
{
    int32_t *rk = V.rkey + pe * V.D;
    bool any = false;
    kfm_each_observer(left, V.tag + s * V.R, V.R, [&](int) { any = true; });
    if (any) (void)kfm_rows_drop(rk, V.D, key);
    else { kfm_rows_clear(rk, V.D); V.dhas[pe] = 0; }
}
// remove_kf_observation! for observation i of slot r's slab (i < the slab's length): a live observation's point, where its entry still carries that id,
// loses observer bit r.  THE rule of remove_keyframe! (map_manager.jl:184-209) as far as the map goes -- the forgetting of a re-used slot, the filter's
// removals and slam_kfmap_remove_keyframe all come here.  Ids are unique within a slab, but several slabs may lose the same point in one launch (the
// filter's closing pass): the atomic keeps every read-modify-write whole, and its return value tells the rows (ROWS) whether the bit was set and what is left.
template <bool ROWS> __device__ __forceinline__ void kfm_forget_slab(const KfmView<ROWS> &V, int s, int r, int i)
{
    int64_t id;
    size_t pe;
    if (!kfm_slab_point(V, s, r, i, id, pe) || !kfm_owned(V, pe, id)) return;
    const unsigned long long old = atomicAnd(&V.pmask[pe], ~(1ull << r));
    if constexpr (ROWS) { if ((old >> r & 1) && !(V.pflags[pe] & KFM_DEAD)) kfm_rows_lost(V, s, pe, V.tag[s * V.R + r], old & ~(1ull << r)); }
}

// ---- recording: slot-parallel, one thread per list slot (grid.y = stream) -------------------------------------------------------------------------------
// the key-frame whose slot the new one takes is forgotten: every point it observed loses that observer
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_forget(KfmView<ROWS> V, const int *kfcount, const int *sel)
{
    const int s = KFM_STREAM(blockIdx.y), i = blockIdx.x * 256 + threadIdx.x, kfid = kfcount[s] - 1;
    if (kfid < 0) return;
    const int r = kfid % V.R, t = V.tag[s * V.R + r];
    if (t == 0 || t == kfid + 1 || i >= min(V.kn[s * V.R + r], V.cap)) return;
    kfm_forget_slab<ROWS>(V, s, r, i);
}
// "for mp in rec.mps.values(): mp.observed = False"
__global__ __launch_bounds__(256) void k_kfm_clear_observed(KfmapView V, const int *kfcount, const int *sel)
{
    const int s = KFM_STREAM(blockIdx.y), e = blockIdx.x * 256 + threadIdx.x;
    if (kfcount[s] < 1 || e >= V.mcap) return;
    V.pflags[(size_t)s * V.mcap + e] &= (uint8_t)~KFM_OBS;
}
// who owns a table entry after this key-frame: the largest id that maps to it (a newer id replaces an older one); kfresh: whether the point is new
__global__ __launch_bounds__(256) void k_kfm_claim(KfmapView V, KpsetView K, const int *sel)
{
    const int s = KFM_STREAM(blockIdx.y), i = blockIdx.x * 256 + threadIdx.x;
    if (K.kfcount[s] < 1 || i >= min(K.count[s], V.cap)) return;
    const int64_t id = K.id[(size_t)s * K.cap + i];
    const size_t pe = (size_t)s * V.mcap + kfm_entry(id, V.mcap);
    const unsigned long long mine = (unsigned long long)id + 1ull;
    const uint8_t fl = V.pflags[pe];                             // (flags are written by the record pass only: a kernel boundary away)
    uint8_t fresh;
    if (V.ptag[pe] == mine && (fl & KFM_GONE)) fresh = 2;
    else { const unsigned long long old = atomicMax(&V.ptag[pe], mine); fresh = old != mine || (fl & KFM_DEAD) ? 1 : 0; }
    V.kfresh[(size_t)s * V.cap + i] = fresh;
}
// tracked_ba.add_keyframe: the slab of the new key-frame, and every listed point's entry (one thread per entry: its owner's)
// kpx: the raw-pixel store (nullptr: off) -- the list's pixel as it is goes beside the undistorted one
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_record(KfmView<ROWS> V, KpsetView K, const double *par, const int *sel, double *kpx)
{
    const int s = KFM_STREAM(blockIdx.y), i = blockIdx.x * 256 + threadIdx.x, kfid = K.kfcount[s] - 1;
    if (kfid < 0) return;
    const int r = kfid % V.R, n = min(K.count[s], V.cap);
    const double *P = par + KP_PAR * (size_t)s;
    if (i == 0) {
        double X[6];
        pose_to_angles<4>(P, P + 12, X);
        for (int k = 0; k < 6; k++) V.ktheta[6 * ((size_t)s * V.R + r) + k] = X[k];
        V.tag[s * V.R + r] = kfid + 1; V.kn[s * V.R + r] = n; V.cur[s] = kfid + 1;
    }
    if (i >= n) return;
    const size_t ql = (size_t)s * K.cap + i, q = ((size_t)s * V.R + r) * V.cap + i;
    const int64_t id = K.id[ql];
    double cam[4], dist[4], y = K.yx[2 * ql], x = K.yx[2 * ql + 1];
    load_cam(P, cam, dist);
    if (kpx) { kpx[2 * q] = y; kpx[2 * q + 1] = x; }
    if (dist[0] != 0.0 || dist[1] != 0.0 || dist[2] != 0.0 || dist[3] != 0.0) undistort_px(cam, dist, y, x, y, x);     // (all zero: the pixel as it is, a copy)
    const uint8_t fresh = V.kfresh[(size_t)s * V.cap + i];
    V.kid[q] = id; V.kupx[2 * q] = y; V.kupx[2 * q + 1] = x; V.klive[q] = fresh != 2;
    const size_t pe = (size_t)s * V.mcap + kfm_entry(id, V.mcap);
    if (fresh == 2 || !kfm_owned(V, pe, id)) return;                            // not recorded; or an older id whose entry a newer point holds: an orphan
    const bool t3 = K.is3d[ql] != 0;
    if (fresh) {
        for (int k = 0; k < 3; k++) V.pxyz[3 * pe + k] = K.xyz[3 * ql + k];
        V.pmask[pe] = 1ull << r; V.pflags[pe] = KFM_OBS | (t3 ? KFM_3D : 0);
        if (V.dhas) V.dhas[pe] = 0;                                              // a new owner: the old point's descriptor goes with it
        if constexpr (ROWS) kfm_rows_clear(V.rkey + pe * V.D, V.D);              // and its rows
    } else {
        const uint8_t fl = V.pflags[pe];
        V.pmask[pe] |= 1ull << r;
        if (t3 && !(fl & KFM_BA)) for (int k = 0; k < 3; k++) V.pxyz[3 * pe + k] = K.xyz[3 * ql + k];
        V.pflags[pe] = fl | KFM_OBS | (t3 ? KFM_3D : 0);
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------------------
// exclusive scan of one count per thread over the 256 threads (wave shuffles + one LDS hop); *s_base carries the running total across calls
__device__ __forceinline__ int kfm_scan(int cnt, int *s_w, int *s_base)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int off = *s_base + incl - cnt;
    for (int w = 0; w < wv; w++) off += s_w[w];
    __syncthreads();
    if (tid == 0) *s_base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return off;
}
// update_frame_covisibility!'s counts (map_manager.jl:302-340) over the slab of the newest key-frame (slot r0), by the whole workgroup: s_cov[b] += 1 for
// every live, owned point the slab shares with another slot b whose tag is valid (LDS atomics; s_tag: the ring's tags, 64 entries, 0 beyond R).  Returns the
// thread's share of the key-frame's 3-D points.  The gather's plan and the filter both take their covisibility map from here.
__device__ __forceinline__ int kfm_covisibility(const KfmapView &V, int s, int r0, const int *s_tag, int *s_cov)
{
    const int n0 = min(V.kn[s * V.R + r0], V.cap);
    int nb3 = 0;
    for (int i = threadIdx.x; i < n0; i += 256) {
        int64_t id;
        size_t pe;
        if (!kfm_slab_point(V, s, r0, i, id, pe) || !kfm_valid(V, pe, id)) continue;
        nb3 += (V.pflags[pe] & KFM_3D) != 0;
        kfm_each_observer(V.pmask[pe] & ~(1ull << r0), s_tag, V.R, [&](int b) { atomicAdd(&s_cov[b], 1); });
    }
    return nb3;
}
// The plan of one stream's window (tracked_ba.gather up to its arrays), one 256-thread workgroup per stream, no workgroup waits for another:
//   covisibility   one pass over the newest key-frame's slab: nb_3d and, per other observer slot, the shared points (LDS atomics)
//   covmap         the at most 5 newest covisible key-frames (one thread; R <= 64), walked newest first
//   phase          per co-key-frame a pass over its slab in chunks of 256: a thread takes its slot's point if it is 3-D and not yet processed, demotes it
//                  (is_bad) or accepts it and validates its observers (binary search per observer slab); the point's rank is a ballot prefix
//                  (ordered_slot), its first observation index a scan of the observer counts; a pose's first observation index is an LDS atomicMin
//   poses          after each phase the key-frames first met in it take the next pose ids in the order of those indices (one thread): membership in
//                  `poses` decides whether a later low-score co-key-frame is walked, hence the phases are dependent
// Everything the emit pass and the update need goes into the stream's pending-window regions; hdr = status (0 window, 1 none), kfid, P, M, O.
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_plan(KfmView<ROWS> V, const int *minc_all, const int *sel)
{
    __shared__ int s_cov[64], s_first[64], s_order[64], s_asc[64], s_rank[64], s_tag[64], s_w[4], s_base, s_obase, s_cl[N_COVISIBLE], s_ncl, s_P, s_nb3, s_nv, s_nbad;
    __shared__ unsigned long long s_covmask;
    const int s = KFM_STREAM(blockIdx.x), tid = threadIdx.x, R = V.R, cap = V.cap, mcap = V.mcap;
    int *hdr = V.whdr + KFM_HDR * (size_t)s;
    const int minc = minc_all[s], kfid = V.cur[s] - 1;
    const size_t pb = (size_t)s * mcap;
    if (tid < 64) { s_cov[tid] = 0; s_first[tid] = INT_MAX; s_order[tid] = 0; s_rank[tid] = 0; s_tag[tid] = tid < R ? V.tag[s * R + tid] : 0; }
    if (tid == 0) { s_nb3 = 0; s_P = 0; s_base = 0; s_obase = 0; s_nbad = 0; s_ncl = 0; s_nv = 0; }
    for (int e = tid; e < mcap; e += 256) V.went[pb + e] = 0;
    __syncthreads();
    if (kfid < 0) { if (tid == 0) { hdr[0] = 1; hdr[1] = -1; hdr[2] = hdr[3] = hdr[4] = 0; hdr[5] = minc; hdr[6] = 0; } return; }
    const int r0 = kfid % R;
    {   // nb_3d of the key-frame and the covisibility counts
        const int nb3 = kfm_covisibility(V, s, r0, s_tag, s_cov);
        if (nb3) atomicAdd(&s_nb3, nb3);
    }
    __syncthreads();
    const int nb3 = s_nb3;
    if (nb3 < minc) { if (tid == 0) { hdr[0] = 1; hdr[1] = kfid; hdr[2] = hdr[3] = hdr[4] = 0; hdr[5] = minc; hdr[6] = 0; } return; }
    if (tid == 0) {
        s_cov[r0] = nb3;
        unsigned long long used;
        s_ncl = kfm_covmap_pick(s_tag, s_cov, R, r0, s_cl, used);        // sorted(cov, reverse=True)[:5]
        s_covmask = used;
        s_nv = kfm_rank_slots(s_tag, R, s_rank, s_asc);                  // observers are walked in ascending key-frame id
    }
    __syncthreads();
    const int ncl = s_ncl, nv = s_nv;
    for (int c = 0; c < ncl; c++) {
        const int rc = s_cl[c], score = s_cov[rc];
        if (score == 0) continue;                                                        // (every branch here is uniform over the workgroup)
        if (s_order[rc] == 0 && (score < minc || s_tag[rc] == 1)) continue;              // low score or key-frame 0, and not yet a pose of the window: constant, not walked
        const int n = min(V.kn[s * R + rc], cap);
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int i = c0 + tid;
            bool acc = false;
            int cnt = 0;
            unsigned long long wm = 0;
            int64_t id = 0;
            size_t pe = 0;
            if (i < n && kfm_slab_point(V, s, rc, i, id, pe)) {
                const uint8_t fl = kfm_valid(V, pe, id) ? V.pflags[pe] : 0;
                if ((fl & KFM_3D) && V.went[pe] == 0) {                                  // ids_3d, not yet processed (one thread per entry: ids are unique in a slab)
                    const unsigned long long m = V.pmask[pe];
                    if (__popcll(m) < 2 && !(fl & KFM_OBS)) {                            // is_bad! (map_point.jl:155-161) demotes the point
                        V.pflags[pe] = fl & (uint8_t)~KFM_3D; V.went[pe] = -1;
                        V.wpid[pb + mcap - 1 - atomicAdd(&s_nbad, 1)] = id;
                    } else {
                        acc = true;
                        wm = kfm_live_observers(V, s, m, s_tag, id);                     // an observer whose key-frame or pixel is gone loses the point (remove_obs)
                        cnt = __popcll(wm);
                        if (wm != m) {
                            V.pmask[pe] = wm;
                            if constexpr (ROWS) {                                        // the lost observers' rows go; no observer left: all of them
                                int32_t *rk = V.rkey + pe * V.D;
                                kfm_each_observer(m & ~wm, s_tag, R, [&](int b) { (void)kfm_rows_drop(rk, V.D, s_tag[b]); });
                                if (wm == 0) { kfm_rows_clear(rk, V.D); V.dhas[pe] = 0; }
                            }
                        }
                    }
                }
            }
            const int pos = ordered_slot(acc, s_w, &s_base);
            const int off = kfm_scan(cnt, s_w, &s_obase);
            if (acc) {
                V.went[pe] = pos + 1; V.wpid[pb + pos] = id; V.wpmask[pb + pos] = wm; V.wpoff[pb + pos] = off;
                int j = 0;
                for (int k = 0; k < nv; k++) { const int b = s_asc[k]; if (wm >> b & 1) { if (s_order[b] == 0) atomicMin(&s_first[b], off + j); j++; } }
            }
        }
        __syncthreads();
        if (tid == 0) { int P = s_P; kfm_assign_poses(s_order, s_first, R, P); s_P = P; }      // dense 1-based pose ids in first-encounter order
        __syncthreads();
    }
    if (tid < R) {
        const int b = tid;
        V.wtag[s * R + b] = s_tag[b]; V.worder[s * R + b] = s_order[b]; V.wrank[s * R + b] = s_rank[b];
        V.wconst[s * R + b] = kfm_window_const(s_tag[b], s_covmask >> b & 1, s_cov[b], minc);
    }
    if (tid == 0) {
        V.wcov[s] = s_covmask;
        hdr[0] = s_obase > 0 ? 0 : 1; hdr[1] = kfid; hdr[2] = s_P; hdr[3] = s_base; hdr[4] = s_obase; hdr[5] = minc; hdr[6] = s_nbad;
    }
}

// the caller's arrays on the device, windows back to back (slam_local_ba_batch's layout + the bookkeeping)
struct KfmOut { double *theta; uint8_t *tconst; double *px; int64_t *pose_ids, *point_ids, *poses_remap, *points_remap, *obs_kf, *obs_kp; uint8_t *incov; };
struct KfmWin { int s, pose0, point0, obs0; long long theta0; };          // a window's stream and where its arrays start
// the ascending walk of a stream's slots as the gather saw them: s_asc[rank] = slot; returns their number
__device__ __forceinline__ int kfm_window_slots(const KfmapView &V, int s, int *s_asc)
{
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if ((int)threadIdx.x < V.R && V.wtag[s * V.R + threadIdx.x]) { s_asc[V.wrank[s * V.R + threadIdx.x]] = threadIdx.x; atomicAdd(&s_n, 1); }
    __syncthreads();
    return s_n;
}
// Emit: point-parallel (grid.x chunks of 256 points, grid.y = window); the poses are written by the first chunk
__global__ __launch_bounds__(256) void k_kfm_emit(KfmapView V, const KfmWin *wins, KfmOut Q)
{
    __shared__ int s_asc[64];
    const KfmWin W = wins[blockIdx.y];
    const int s = W.s, R = V.R, j = blockIdx.x * 256 + threadIdx.x;
    const int *hdr = V.whdr + KFM_HDR * (size_t)s;
    const int P = hdr[2], M = hdr[3];
    const int nv = kfm_window_slots(V, s, s_asc);
    if (blockIdx.x == 0 && (int)threadIdx.x < R) {
        const int b = threadIdx.x, o = V.worder[s * R + b];
        if (o > 0) {
            for (int k = 0; k < 6; k++) Q.theta[W.theta0 + 6 * (o - 1) + k] = V.ktheta[6 * ((size_t)s * R + b) + k];
            Q.tconst[W.pose0 + o - 1] = (uint8_t)V.wconst[s * R + b]; Q.poses_remap[W.pose0 + o - 1] = V.wtag[s * R + b] - 1;
        }
    }
    if (j >= M) return;
    const size_t pb = (size_t)s * V.mcap;
    const int64_t id = V.wpid[pb + j];
    const size_t pe = pb + kfm_entry(id, V.mcap);
    for (int k = 0; k < 3; k++) Q.theta[W.theta0 + 6 * P + 3 * (size_t)j + k] = V.pxyz[3 * pe + k];
    Q.points_remap[W.point0 + j] = id;
    const unsigned long long wm = V.wpmask[pb + j], cov = V.wcov[s];
    size_t o = (size_t)W.obs0 + V.wpoff[pb + j];
    for (int k = 0; k < nv; k++) {
        const int b = s_asc[k];
        if (!(wm >> b & 1)) continue;
        const int i = max(kfm_find_live(V, s, b, id), 0);        // (found: the plan validated it in this stream order)
        const size_t q = ((size_t)s * R + b) * V.cap + i;
        Q.px[2 * o] = V.kupx[2 * q]; Q.px[2 * o + 1] = V.kupx[2 * q + 1];
        Q.pose_ids[o] = V.worder[s * R + b]; Q.point_ids[o] = j + 1;
        Q.obs_kf[o] = V.wtag[s * R + b] - 1; Q.obs_kp[o] = id; Q.incov[o] = cov >> b & 1;
        o++;
    }
}

// ---- update (tracked_ba.update): two kernels, because is_bad is evaluated after ALL of a window's removals ------------------------------------------------
struct KfmUpd { int s; long long theta0, obs0; };
// poses, and the removals of the outlier observations: one thread per point of the window walks the point's observations.  A thread touches its own
// point's entry alone; the tombstone it writes is its own observation's: any thread order gives the same map.  Everything goes by key-frame and keypoint
// id: a slot whose tag is no longer the gather's holds another key-frame now and is skipped, a point whose entry another id holds is skipped.
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_upd_obs(KfmView<ROWS> V, const KfmUpd *wins, const double *theta, const uint8_t *outl)
{
    __shared__ int s_asc[64];
    const KfmUpd W = wins[blockIdx.y];
    const int s = W.s, R = V.R, j = blockIdx.x * 256 + threadIdx.x;
    const int *hdr = V.whdr + KFM_HDR * (size_t)s;
    const int kfid = hdr[1], M = hdr[3];
    const int nv = kfm_window_slots(V, s, s_asc);
    if (blockIdx.x == 0 && (int)threadIdx.x < R) {
        const int b = threadIdx.x, o = V.worder[s * R + b];
        if (o > 0 && V.tag[s * R + b] == V.wtag[s * R + b])
            for (int k = 0; k < 6; k++) V.ktheta[6 * ((size_t)s * R + b) + k] = theta[W.theta0 + 6 * (o - 1) + k];
    }
    if (j >= M) return;
    const size_t pb = (size_t)s * V.mcap;
    const int64_t id = V.wpid[pb + j];
    const size_t pe = pb + kfm_entry(id, V.mcap);
    const bool have = kfm_valid(V, pe, id);
    const unsigned long long wm = V.wpmask[pb + j], cov = V.wcov[s];
    unsigned long long mask = have ? V.pmask[pe] : 0;
    uint8_t fl = have ? V.pflags[pe] : 0;
    size_t o = (size_t)W.obs0 + V.wpoff[pb + j];
    for (int k = 0; k < nv; k++) {
        const int b = s_asc[k];
        if (!(wm >> b & 1)) continue;
        if (outl[o++]) {
            if ((cov >> b & 1) && V.tag[s * R + b] == V.wtag[s * R + b]) {               // remove_mappoint_obs! (map_manager.jl:224-)
                const int i = kfm_find_live(V, s, b, id);
                if (i >= 0) V.klive[((size_t)s * R + b) * V.cap + i] = 0;
                if constexpr (ROWS) { if (have && (mask >> b & 1)) (void)kfm_rows_drop(V.rkey + pe * V.D, V.D, V.wtag[s * R + b]); }
                mask &= ~(1ull << b);
            }
            if (V.wtag[s * R + b] - 1 == kfid) fl = (fl & (uint8_t)~KFM_OBS) | KFM_GONE;     // remove_obs_from_current_frame!
        }
    }
    if constexpr (ROWS) { if (have && mask != V.pmask[pe]) kfm_rows_lost(V, s, pe, 0, mask); }       // (the rows went above; no valid observer left: all go)
    if (have) { V.pmask[pe] = mask; V.pflags[pe] = fl; }
}
// remove_mappoint! (map_manager.jl:139-168): the point's observations become tombstones, the entry dies; an observed point's id has left the frame
__device__ __forceinline__ void kfm_remove_point(const KfmapView &V, int s, size_t pe, int64_t id, uint8_t fl)
{
    kfm_each_observer(V.pmask[pe], V.tag + s * V.R, V.R, [&](int b) {
        const int i = kfm_find_live(V, s, b, id);
        if (i >= 0) V.klive[((size_t)s * V.R + b) * V.cap + i] = 0;
    });
    V.pmask[pe] = 0; V.pflags[pe] = KFM_DEAD | ((fl & KFM_OBS) ? KFM_GONE : 0) | (fl & KFM_GONE);
}
// is_bad on every point of the window and on the gather's bad set: removed, or (window points) the refined position.  Thread t < M owns point t of the
// window, thread t < M + nbad the bad point t - M: all different entries.
__global__ __launch_bounds__(256) void k_kfm_upd_points(KfmapView V, const KfmUpd *wins, const double *theta)
{
    const KfmUpd W = wins[blockIdx.y];
    const int s = W.s, t = blockIdx.x * 256 + threadIdx.x;
    const int *hdr = V.whdr + KFM_HDR * (size_t)s;
    const int P = hdr[2], M = hdr[3], nbad = hdr[6];
    if (t >= M + nbad) return;
    const size_t pb = (size_t)s * V.mcap;
    const int64_t id = t < M ? V.wpid[pb + t] : V.wpid[pb + V.mcap - 1 - (t - M)];
    const size_t pe = pb + kfm_entry(id, V.mcap);
    if (!kfm_valid(V, pe, id)) return;
    const uint8_t fl = V.pflags[pe];
    const int nobs = __popcll(V.pmask[pe]);
    if (nobs < 2 && !(fl & KFM_OBS) && ((fl & KFM_3D) || nobs == 0)) { kfm_remove_point(V, s, pe, id, fl); return; }
    if (t < M) {
        for (int k = 0; k < 3; k++) V.pxyz[3 * pe + k] = theta[W.theta0 + 6 * P + 3 * (size_t)t + k];
        V.pflags[pe] = fl | KFM_BA;
    }
}
// the live lists follow: an id that has left the frame is flagged for the compaction, a 3-D keypoint whose point the window kept takes its position
__global__ __launch_bounds__(256) void k_kfm_upd_list(KfmapView V, KpsetView K, const KfmUpd *wins, uint8_t *flags)
{
    const int s = wins[blockIdx.y].s, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K.count[s]) return;
    const size_t q = (size_t)s * K.cap + i, pb = (size_t)s * V.mcap;
    const int64_t id = K.id[q];
    const size_t pe = pb + kfm_entry(id, V.mcap);
    if (!kfm_owned(V, pe, id)) return;
    const uint8_t fl = V.pflags[pe];
    if (fl & KFM_GONE) { flags[q] = 1; return; }
    const int w = V.went[pe];
    if (!(fl & KFM_DEAD) && K.is3d[q] && w > 0 && V.wpid[pb + w - 1] == id) for (int k = 0; k < 3; k++) K.xyz[3 * q + k] = V.pxyz[3 * pe + k];
}

// ---- filtering (map_filtering!, estimator.jl:358-406; tests/np_kfmap_filter.py is the model) -------------------------------------------------------------
// One 256-thread workgroup per stream, no workgroup waits for another:
//   candidates     the covisibility map of the newest key-frame (kfm_covisibility); one thread ranks it ascending by key-frame id and applies the walk's
//                  gates: key-frame 0 ends the walk (`kfid == 0 && break`), an id >= the newest is passed over
//   phase          per candidate a pass over its slab in chunks of 256: a thread looks its observation's point up and, if it is 3-D, counts it (n_total) and
//                  whether more than four key-frames observe it (n_good); a wave reduction and one LDS hop give every thread both sums, so the decision --
//                  n_total < min_cov_score / 2, else n_good / n_total > filtering_ratio in doubles (0 / 0 is NaN: kept) -- is uniform
//   removal        the set X of key-frames removed so far is a register of every thread (uniform); observers are counted as popcount(mask & valid & ~X), so
//                  no phase reads anything an earlier phase wrote and the map is written once, in a closing pass over the removed slabs (kfm_forget_slab),
//                  after the last phase's barrier; then their tags and lengths are reset
// frem[s] = X: bit k % R per removed key-frame.  new_kf_available has no counterpart: lock-stepped streams never race.
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_filter(KfmView<ROWS> V, const double *ratio_all, const int *minc_all, int first_kfid, const int *sel)
{
    __shared__ int s_cov[64], s_tag[64], s_cand[64], s_ncand, s_tot[2][4], s_good[2][4];
    __shared__ unsigned long long s_valid;
    const int s = KFM_STREAM(blockIdx.x), tid = threadIdx.x, R = V.R, cap = V.cap;
    const double ratio = ratio_all[s];
    const int kfid = V.cur[s] - 1, few = minc_all[s] / 2;
    if (ratio >= 1.0 || kfid < first_kfid) { if (tid == 0) V.frem[s] = 0; return; }      // (uniform; first_kfid >= 0: a stream without a key-frame leaves here)
    if (tid < 64) { s_cov[tid] = 0; s_tag[tid] = tid < R ? V.tag[s * R + tid] : 0; }
    __syncthreads();
    const int r0 = kfid % R;
    (void)kfm_covisibility(V, s, r0, s_tag, s_cov);
    __syncthreads();
    if (tid == 0) {
        unsigned long long valid;
        s_ncand = kfm_filter_candidates(s_tag, s_cov, R, r0, kfid, s_cand, valid);       // ascending by key-frame id
        s_valid = valid;
    }
    __syncthreads();
    const int ncand = s_ncand, lane = tid & 63, wv = tid >> 6;
    const unsigned long long valid = s_valid;
    unsigned long long X = 0;
    for (int c = 0; c < ncand; c++) {
        const int rc = s_cand[c];
        const int n = min(V.kn[s * R + rc], cap);
        const unsigned long long seen = valid & ~X;
        int tot = 0, good = 0;
        for (int i = tid; i < n; i += 256) {
            int64_t id;
            size_t pe;
            if (!kfm_slab_point(V, s, rc, i, id, pe) || !kfm_valid(V, pe, id) || !(V.pflags[pe] & KFM_3D)) continue;      // an orphan is skipped and left as it is
            tot++; good += __popcll(V.pmask[pe] & seen) > 4;
        }
        for (int o = 32; o; o >>= 1) { tot += __shfl_down(tot, o, 64); good += __shfl_down(good, o, 64); }
        if (lane == 0) { s_tot[c & 1][wv] = tot; s_good[c & 1][wv] = good; }
        __syncthreads();                                         // (two buffers: a wave that writes phase c + 2's sums has passed phase c + 1's barrier, behind every read of phase c's)
        const int n_total = s_tot[c & 1][0] + s_tot[c & 1][1] + s_tot[c & 1][2] + s_tot[c & 1][3];
        const int n_good = s_good[c & 1][0] + s_good[c & 1][1] + s_good[c & 1][2] + s_good[c & 1][3];
        if (kfm_filter_removes(n_total, n_good, few, ratio)) X |= 1ull << rc;
    }
    for (unsigned long long m = X; m; m &= m - 1) {              // every phase's reads lie behind its barrier: now the removals, all at once
        const int b = __ffsll((long long)m) - 1, n = min(V.kn[s * R + b], cap);
        for (int i = tid; i < n; i += 256) kfm_forget_slab<ROWS>(V, s, b, i);
    }
    __syncthreads();                                             // the lengths are read above, reset below
    if (tid < R && (X >> tid & 1)) { V.tag[s * R + tid] = 0; V.kn[s * R + tid] = 0; }
    if (tid == 0) V.frem[s] = X;
}
// slam_kfmap_remove_keyframe: slab-parallel, then (a launch later: every block has read the tag) the slot is emptied
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_remove(KfmView<ROWS> V, int s, int kfid)
{
    const int r = kfid % V.R, i = blockIdx.x * 256 + threadIdx.x;
    if (V.tag[s * V.R + r] != kfid + 1 || V.cur[s] == kfid + 1 || i >= min(V.kn[s * V.R + r], V.cap)) return;
    kfm_forget_slab<ROWS>(V, s, r, i);
}
__global__ void k_kfm_drop_slot(KfmapView V, int s, int kfid)
{
    const int q = s * V.R + kfid % V.R;
    if (V.tag[q] == kfid + 1 && V.cur[s] != kfid + 1) { V.tag[q] = 0; V.kn[q] = 0; }
}

// A <bool ROWS> kernel's launch, 256 threads a workgroup, the view first among its arguments: <true> with the whole view where the row store is on, else
// <false> with the view as it always was
#define KFM_LAUNCH_ROWS(km, kernel, grid, ...) \
    do { if ((km)->v.rkey) hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, ctx->stream, (km)->v, __VA_ARGS__); \
         else hipLaunchKernelGGL(kernel<false>, grid, dim3(256), 0, ctx->stream, static_cast<const KfmapView &>((km)->v), __VA_ARGS__); } while (0)
// Every region of the map's one allocation, each named once (kfmap.hpp has the formula): without a block for the total, with it to bind the pointers
static size_t kfmap_regions(slam_kfmap *km, char *base)
{
    Layout Lo;
    KfmapView &v = km->v;
    const size_t S = v.S, sr = S * v.R, n = sr * v.cap, m = S * v.mcap;
    Lo.bind(v.tag, sr * 4, base); Lo.bind(v.kn, sr * 4, base); Lo.bind(v.ktheta, sr * 48, base); Lo.bind(v.kid, n * 8, base); Lo.bind(v.kupx, n * 16, base); Lo.bind(v.klive, n, base); Lo.bind(v.kfresh, S * v.cap, base);
    Lo.bind(v.ptag, m * 8, base); Lo.bind(v.pxyz, m * 24, base); Lo.bind(v.pmask, m * 8, base); Lo.bind(v.pflags, m, base);
    Lo.bind(v.cur, S * 4, base); Lo.bind(v.frem, S * 8, base);
    Lo.bind(v.whdr, S * KFM_HDR * 4, base); Lo.bind(v.wtag, sr * 4, base); Lo.bind(v.worder, sr * 4, base); Lo.bind(v.wrank, sr * 4, base); Lo.bind(v.wconst, sr * 4, base); Lo.bind(v.wcov, S * 8, base);
    Lo.bind(v.wpid, m * 8, base); Lo.bind(v.wpmask, m * 8, base); Lo.bind(v.wpoff, m * 4, base); Lo.bind(v.went, m * 4, base);
    return Lo.size();
}
// the streams the gather acts on (those of the last add_keyframe), ascending; returns their number
static int kfmap_streams(const slam_kfmap *km, int *list)
{
    int n = 0;
    for (int s = 0; s < km->v.S; s++) if (km->n_sel == KPSEL_ALL || km->sel_host[s]) list[n++] = s;
    return n;
}

// a call's table of the streams it acts on, into its region of a staging block
static void kfmap_put_streams(const Region<int> &o_sel, char *h, const int *list, int ns) { memcpy(o_sel.at(h), list, (size_t)ns * 4); }
// the map's pinned staging block for an enqueue-only call's inputs, at least `bytes` long, once the copy that last read it has completed (an event never
// recorded is complete); the caller records pin_ev behind its own copy
static int kfmap_pin(slam_ctx *ctx, slam_kfmap *km, size_t bytes, char **out)
{
    HIP_TRY(ctx, hipEventSynchronize(km->pin_ev));
    if (km->pin_bytes < bytes) {
        if (km->pin) (void)hipHostFree(km->pin);
        km->pin = nullptr; km->pin_bytes = 0;
        HIP_TRY(ctx, hipHostMalloc((void **)&km->pin, bytes + bytes / 4));
        km->pin_bytes = bytes + bytes / 4;
    }
    *out = km->pin;
    return SLAM_OK;
}
// An enqueue-only call's inputs: `bytes` of the map's pinned block, filled by fill(h), copied to scratch (*scr) on the stream, pin_ev recorded behind the
// copy.  Nothing waits.  room > bytes: the scratch block is that long (the call's device-only regions lie behind its inputs).
template <class Fill> static int kfmap_upload(slam_ctx *ctx, slam_kfmap *km, size_t bytes, char **scr, Fill fill, size_t room = 0)
{
    char *h;
    int rc = kfmap_pin(ctx, km, bytes, &h);
    if (rc) return rc;
    rc = slam_scratch(ctx, std::max(bytes, room), (void **)scr);
    if (rc) return rc;
    fill(h);
    HIP_TRY(ctx, hipMemcpyAsync(*scr, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(km->pin_ev, ctx->stream));
    return SLAM_OK;
}
// One of the map's long-lived allocations: `bytes` of HBM, zeroed on the stream, waited for.  An error frees the block and fails under the entry point's name.
static int kfmap_alloc_zeroed(slam_ctx *ctx, const char *who, size_t bytes, char **out)
{
    char *base = nullptr;
    hipError_t e = hipMalloc((void **)&base, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(base, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = slam_stream_wait(ctx->stream);
    if (e != hipSuccess) { if (base) (void)hipFree(base); return slam_fail(ctx, SLAM_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
    *out = base;
    return SLAM_OK;
}

// the count pass of the gather and of slam_kfmap_local_ba: table + thresholds up, k_kfm_plan, the S headers back (a wait)
static int kfmap_plan_headers(slam_ctx *ctx, slam_kfmap *km, const int32_t *min_cov_score, const int *list, int ns, std::vector<int> &hdr)
{
    const KfmapView &V = km->v;
    const int S = V.S;
    Layout D;
    const auto o_sel = D.take<int>(S), o_minc = D.take<int>(S); const size_t in_b = D.size();
    char *scr, *h;
    int rc = slam_scratch(ctx, D.size(), (void **)&scr);
    if (rc) return rc;
    rc = slam_pinned(ctx, std::max<size_t>(D.size(), (size_t)S * KFM_HDR * 4), (void **)&h);
    if (rc) return rc;
    kfmap_put_streams(o_sel, h, list, ns); memcpy(o_minc.at(h), min_cov_score, (size_t)S * 4);
    HIP_TRY(ctx, hipMemcpyAsync(scr, h, in_b, hipMemcpyHostToDevice, ctx->stream));
    { ProfScope span(ctx, "kfmap_gather_plan");
      KFM_LAUNCH_ROWS(km, k_kfm_plan, dim3(ns), (const int *)o_minc.at(scr), (const int *)o_sel.at(scr)); }
    HIP_TRY(ctx, hipGetLastError());
    rc = kpset_read_back(ctx, h, {{0, V.whdr, (size_t)S * KFM_HDR * 4, nullptr}});
    if (rc) return rc;
    hdr.resize((size_t)S * KFM_HDR);
    memcpy(hdr.data(), h, hdr.size() * 4);
    return SLAM_OK;
}

// the update kernels over the windows of the device table wd, theta / outl in HBM (windows back to back, KfmUpd::theta0 / obs0), then the lists' compaction
static int kfmap_update_enqueue(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, const KfmUpd *wd, int n_windows, int maxM, const double *theta, const uint8_t *outl)
{
    const KfmapView &V = km->v;
    uint8_t *flags = nullptr;
    if (ks) {
        const int rc = slam_scratch2(ctx, (size_t)ks->S * ks->v.cap, (void **)&flags);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(flags, 0, (size_t)ks->S * ks->v.cap, ctx->stream));
    }
    { ProfScope span(ctx, "kfmap_update");
      KFM_LAUNCH_ROWS(km, k_kfm_upd_obs, dim3((maxM + 255) / 256, n_windows), wd, theta, outl);
      hipLaunchKernelGGL(k_kfm_upd_points, dim3((V.mcap + 255) / 256, n_windows), dim3(256), 0, ctx->stream, V, wd, theta);
      if (ks) hipLaunchKernelGGL(k_kfm_upd_list, dim3((ks->v.cap + 255) / 256, n_windows), dim3(256), 0, ctx->stream, V, ks->v, wd, flags); }
    HIP_TRY(ctx, hipGetLastError());
    if (ks) return kpset_compact(ctx, ks, 1, flags);             // (a stream without a flag keeps every slot where it is)
    return SLAM_OK;
}

extern "C" {

int slam_kfmap_destroy(slam_kfmap *km);

int slam_kfmap_create(slam_ctx *ctx, int S, int cap, int R, int mcap, slam_kfmap **out)
{
    ARG_TRY(ctx, ctx != nullptr && out != nullptr && S >= 1 && S <= 128 && cap >= 1 && R >= 2 && R <= KFM_MAX_R && mcap >= 1 && mcap <= (1 << 22) &&
                     (size_t)S * R * cap < (1u << 30) && (size_t)S * mcap < (1u << 30));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    slam_kfmap *km = new slam_kfmap();
    km->device = ctx->device; km->v.S = S; km->v.cap = cap; km->v.R = R; km->v.mcap = mcap;
    km->bytes = kfmap_regions(km, nullptr);
    const int rc = kfmap_alloc_zeroed(ctx, "slam_kfmap_create", km->bytes, &km->base);
    if (rc) { slam_kfmap_destroy(km); return rc; }
    const hipError_t e = hipEventCreateWithFlags(&km->pin_ev, hipEventDisableTiming);
    if (e != hipSuccess) { slam_kfmap_destroy(km); return slam_fail(ctx, SLAM_ERR_HIP, "slam_kfmap_create: %s", hipGetErrorString(e)); }
    kfmap_regions(km, km->base);
    *out = km;
    return SLAM_OK;
}

int slam_kfmap_destroy(slam_kfmap *km)
{
    if (!km) return SLAM_OK;
    (void)hipSetDevice(km->device);
    (void)hipDeviceSynchronize();
    if (km->base) (void)hipFree(km->base);
    if (km->pin) (void)hipHostFree(km->pin);
    if (km->dbase) (void)hipFree(km->dbase);
    if (km->rbase) (void)hipFree(km->rbase);
    if (km->kpx) (void)hipFree(km->kpx);
    if (km->lm_base) (void)hipFree(km->lm_base);
    if (km->mg_base) (void)hipFree(km->mg_base);
    if (km->hs_base) (void)hipFree(km->hs_base);
    if (km->ba_base) (void)hipFree(km->ba_base);
    if (km->pin_ev) (void)hipEventDestroy(km->pin_ev);
    delete km;
    return SLAM_OK;
}

int slam_kfmap_add_keyframe(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, const double *params)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && ks != nullptr && params != nullptr && ks->S == km->v.S && ks->v.cap <= km->v.cap);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    km->n_sel = ks->n_sel; memcpy(km->sel_host, ks->sel_host, sizeof km->sel_host);
    if (kpset_none_selected(ks)) return SLAM_OK;
    const double *par;
    const int rc = kpset_stage_params(ctx, ks, params, (size_t)ks->S * KP_PAR, &par);
    if (rc) return rc;
    const int *sel = kpset_sel_table(ks), ns = kpset_sel_streams(ks);
    const KfmapView &V = km->v;
    const dim3 gl((ks->v.cap + 255) / 256, ns), gs((V.cap + 255) / 256, ns), gm((V.mcap + 255) / 256, ns);
    { ProfScope span(ctx, "kfmap_add");
      KFM_LAUNCH_ROWS(km, k_kfm_forget, gs, (const int *)ks->v.kfcount, sel);
      hipLaunchKernelGGL(k_kfm_clear_observed, gm, dim3(256), 0, ctx->stream, V, (const int *)ks->v.kfcount, sel);
      hipLaunchKernelGGL(k_kfm_claim, gl, dim3(256), 0, ctx->stream, V, ks->v, sel);
      KFM_LAUNCH_ROWS(km, k_kfm_record, gl, ks->v, par, sel, km->kpx); }
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

int slam_kfmap_ba_gather(slam_ctx *ctx, slam_kfmap *km, const int32_t *min_cov_score, const slam_kfmap_windows *out, int32_t *n_windows)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && min_cov_score != nullptr && out != nullptr && n_windows != nullptr && out->status && out->win_stream &&
                     out->Pn && out->Mn && out->On && out->theta && out->theta_const && out->pixels_yx && out->pose_ids && out->point_ids &&
                     out->cap_windows >= 0 && out->cap_poses >= 0 && out->cap_points >= 0 && out->cap_obs >= 0);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const int S = V.S;
    int list[128];
    const int ns = kfmap_streams(km, list);
    *n_windows = 0;
    for (int s = 0; s < S; s++) { out->status[s] = 3; }
    for (int k = 0; k < ns; k++) km->pend[list[k]].valid = 0;
    if (ns == 0) return SLAM_OK;
    // count pass: table + thresholds up, the plan, the headers back (the first of the call's two waits)
    std::vector<int> hdr;
    char *scr, *h;
    int rc = kfmap_plan_headers(ctx, km, min_cov_score, list, ns, hdr);
    if (rc) return rc;
    // scan over the streams: where each window goes, which ones fit
    std::vector<KfmWin> wins;
    long long nP = 0, nM = 0, nO = 0, nT = 0;
    for (int k = 0; k < ns; k++) {
        const int s = list[k], *hd = hdr.data() + (size_t)KFM_HDR * s, P = hd[2], M = hd[3], O = hd[4];
        if (hd[0] != 0) { out->status[s] = 1; continue; }
        if ((int)wins.size() + 1 > out->cap_windows || nP + P > out->cap_poses || nM + M > out->cap_points || nO + O > out->cap_obs) { out->status[s] = 2; continue; }
        out->status[s] = 0;
        const int w = (int)wins.size();
        out->win_stream[w] = s; out->Pn[w] = P; out->Mn[w] = M; out->On[w] = O;
        wins.push_back({s, (int)nP, (int)nM, (int)nO, nT});
        km->pend[s] = {1, hd[1], P, M, O};
        nP += P; nM += M; nO += O; nT += 6ll * P + 3ll * M;
    }
    const int nw = (int)wins.size();
    *n_windows = nw;
    if (nw == 0) return SLAM_OK;
    // emit pass into one block laid out as the caller's arrays, then the call's one copy of results
    Layout E;
    const auto e_win = E.take<KfmWin>(nw);
    const auto e_th = E.take<double>((size_t)nT), e_px = E.take<double>(2 * (size_t)nO);
    const auto e_pi = E.take<int64_t>((size_t)nO), e_li = E.take<int64_t>((size_t)nO), e_ok = E.take<int64_t>((size_t)nO), e_op = E.take<int64_t>((size_t)nO);
    const auto e_pr = E.take<int64_t>((size_t)nP), e_lr = E.take<int64_t>((size_t)nM);
    const auto e_tc = E.take<uint8_t>((size_t)nP), e_ic = E.take<uint8_t>((size_t)nO);
    rc = slam_scratch(ctx, E.size(), (void **)&scr);
    if (rc) return rc;
    rc = slam_pinned(ctx, E.size(), (void **)&h);
    if (rc) return rc;
    memcpy(e_win.at(h), wins.data(), e_win.bytes());
    HIP_TRY(ctx, hipMemcpyAsync(e_win.at(scr), e_win.at(h), e_win.bytes(), hipMemcpyHostToDevice, ctx->stream));
    int maxM = 1;
    for (int w = 0; w < nw; w++) maxM = std::max(maxM, (int)out->Mn[w]);
    const KfmOut Q = {e_th.at(scr), e_tc.at(scr), e_px.at(scr), e_pi.at(scr), e_li.at(scr), e_pr.at(scr), e_lr.at(scr), e_ok.at(scr), e_op.at(scr), e_ic.at(scr)};
    { ProfScope span(ctx, "kfmap_gather_emit");
      hipLaunchKernelGGL(k_kfm_emit, dim3((maxM + 255) / 256, nw), dim3(256), 0, ctx->stream, V, (const KfmWin *)e_win.at(scr), Q); }
    HIP_TRY(ctx, hipGetLastError());
    const size_t lo = e_th.off, len = E.size() - lo;
    HIP_TRY(ctx, hipMemcpyAsync(h + lo, scr + lo, len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    auto give = [&](void *dst, const auto &r) { if (dst && r.count) memcpy(dst, r.at(h), r.bytes()); };
    give(out->theta, e_th); give(out->theta_const, e_tc); give(out->pixels_yx, e_px); give(out->pose_ids, e_pi); give(out->point_ids, e_li);
    give(out->poses_remap, e_pr); give(out->points_remap, e_lr); give(out->obs_kf, e_ok); give(out->obs_kp, e_op); give(out->obs_in_covmap, e_ic);
    return SLAM_OK;
}

int slam_kfmap_ba_update(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, int n_windows, const int32_t *win_stream, const double *theta, const uint8_t *outliers)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && n_windows >= 0 && n_windows <= km->v.S && (n_windows == 0 || (win_stream && theta && outliers)) &&
                     (ks == nullptr || (ks->S == km->v.S && ks->v.cap <= km->v.cap)));
    const KfmapView &V = km->v;
    std::vector<KfmUpd> wins((size_t)n_windows);
    long long nT = 0, nO = 0;
    int maxM = 1;
    uint8_t seen[128] = {};
    for (int w = 0; w < n_windows; w++) {                        // every check before anything is enqueued
        const int s = win_stream[w];
        if (s < 0 || s >= V.S || seen[s] || !km->pend[s].valid)
            return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_ba_update: window %d names stream %d, which has no pending window", w, s);
        seen[s] = 1;
        wins[w] = {s, nT, nO};
        nT += 6ll * km->pend[s].P + 3ll * km->pend[s].M; nO += km->pend[s].O; maxM = std::max(maxM, km->pend[s].M);
    }
    if (n_windows == 0) return SLAM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Layout D;
    const auto o_win = D.take<KfmUpd>(n_windows); const auto o_th = D.take<double>((size_t)nT); const auto o_ol = D.take<uint8_t>((size_t)nO);
    char *scr;
    int rc = kfmap_upload(ctx, km, D.size(), &scr, [&](char *h) {
        memcpy(o_win.at(h), wins.data(), o_win.bytes()); memcpy(o_th.at(h), theta, o_th.bytes()); memcpy(o_ol.at(h), outliers, o_ol.bytes());
    });
    if (rc) return rc;
    rc = kfmap_update_enqueue(ctx, km, ks, o_win.at(scr), n_windows, maxM, o_th.at(scr), o_ol.at(scr));
    if (rc) return rc;
    for (int w = 0; w < n_windows; w++) km->pend[win_stream[w]].valid = 0;
    return SLAM_OK;
}

// The estimator step on the map, the windows never leaving HBM (include/slamhip.h): plan + headers back, emit into the map's own device block, the device-input
// batch solve on those arrays, the update kernels on the same arrays.  Windows the device batch does not take (SLAM_BA_DEV_INELIGIBLE) take the host route inside
// the call: their slices come down, slam_local_ba_batch solves them, theta and flags go back up into the block -- and ONE update launch applies all solved windows.
int slam_kfmap_local_ba(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, const int32_t *min_cov_score, const double *cams,
                        int iters_fast, int iterations, double repr_eps, int32_t *status, double *stats)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && min_cov_score != nullptr && cams != nullptr && status != nullptr && iters_fast >= 0 && iterations >= 0 &&
                     (ks == nullptr || (ks->S == km->v.S && ks->v.cap <= km->v.cap)));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const int S = V.S;
    int list[128];
    const int ns = kfmap_streams(km, list);
    for (int s = 0; s < S; s++) { status[s] = 3; km->last_win[s][0] = km->last_win[s][1] = km->last_win[s][2] = 0; }
    if (stats) memset(stats, 0, (size_t)S * 8 * sizeof(double));
    for (int k = 0; k < ns; k++) km->pend[list[k]].valid = 0;
    if (ns == 0) return SLAM_OK;
    std::vector<int> hdr;
    int rc = kfmap_plan_headers(ctx, km, min_cov_score, list, ns, hdr);
    if (rc) return rc;
    std::vector<KfmWin> wins;
    std::vector<int32_t> Pn, Mn, On;
    std::vector<double> cw;
    long long nP = 0, nM = 0, nO = 0, nT = 0;
    int maxM = 1;
    for (int k = 0; k < ns; k++) {
        const int s = list[k], *hd = hdr.data() + (size_t)KFM_HDR * s, P = hd[2], M = hd[3], O = hd[4];
        if (hd[0] != 0) { status[s] = 1; continue; }
        status[s] = 0;
        wins.push_back({s, (int)nP, (int)nM, (int)nO, nT});
        Pn.push_back(P); Mn.push_back(M); On.push_back(O); cw.insert(cw.end(), cams + 4 * s, cams + 4 * s + 4);
        km->pend[s] = {1, hd[1], P, M, O};
        km->last_win[s][0] = P; km->last_win[s][1] = M; km->last_win[s][2] = O;
        nP += P; nM += M; nO += O; nT += 6ll * P + 3ll * M; maxM = std::max(maxM, M);
    }
    const int nw = (int)wins.size();
    if (nw == 0) return SLAM_OK;
    // the windows' arrays, laid out as the gather's block, plus the outlier flags and the update's table: the map's own block in HBM
    Layout E;
    const auto e_win = E.take<KfmWin>(nw); const auto e_upd = E.take<KfmUpd>(nw);
    const auto e_th = E.take<double>((size_t)nT), e_px = E.take<double>(2 * (size_t)nO);
    const auto e_pi = E.take<int64_t>((size_t)nO), e_li = E.take<int64_t>((size_t)nO), e_ok = E.take<int64_t>((size_t)nO), e_op = E.take<int64_t>((size_t)nO);
    const auto e_pr = E.take<int64_t>((size_t)nP), e_lr = E.take<int64_t>((size_t)nM);
    const auto e_tc = E.take<uint8_t>((size_t)nP), e_ic = E.take<uint8_t>((size_t)nO), e_ol = E.take<uint8_t>((size_t)nO + 1);
    if (km->ba_bytes < E.size()) {
        HIP_TRY(ctx, slam_stream_wait(ctx->stream));
        if (km->ba_base) (void)hipFree(km->ba_base);
        km->ba_base = nullptr; km->ba_bytes = 0;
        HIP_TRY(ctx, hipMalloc((void **)&km->ba_base, E.size() + E.size() / 4));
        km->ba_bytes = E.size() + E.size() / 4;
    }
    char *blk = km->ba_base, *h;
    const size_t tab_b = e_th.off;                               // the two tables stand first
    rc = kfmap_pin(ctx, km, tab_b, &h);
    if (rc) return rc;
    memcpy(e_win.at(h), wins.data(), e_win.bytes());
    HIP_TRY(ctx, hipMemcpyAsync(e_win.at(blk), e_win.at(h), e_win.bytes(), hipMemcpyHostToDevice, ctx->stream));
    const KfmOut Q = {e_th.at(blk), e_tc.at(blk), e_px.at(blk), e_pi.at(blk), e_li.at(blk), e_pr.at(blk), e_lr.at(blk), e_ok.at(blk), e_op.at(blk), e_ic.at(blk)};
    { ProfScope span(ctx, "kfmap_gather_emit");
      hipLaunchKernelGGL(k_kfm_emit, dim3((maxM + 255) / 256, nw), dim3(256), 0, ctx->stream, V, (const KfmWin *)e_win.at(blk), Q); }
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> wst((size_t)nw, 0);
    std::vector<double> wsv((size_t)nw * 8, 0.0);
    rc = slam_local_ba_batch_dev(ctx, nw, cw.data(), Pn.data(), Mn.data(), On.data(), e_th.at(blk), e_tc.at(blk), e_px.at(blk), e_pi.at(blk), e_li.at(blk), e_ol.at(blk),
                                 iters_fast, iterations, repr_eps, wsv.data(), wst.data());
    if (rc) return rc;
    // the in-call host route of the windows the device batch does not take
    std::vector<int> hostw;
    for (int w = 0; w < nw; w++) if (wst[w] == SLAM_BA_DEV_INELIGIBLE) hostw.push_back(w);
    if (!hostw.empty()) {
        const int nh = (int)hostw.size();
        std::vector<int32_t> hP(nh), hM(nh), hO(nh), hst(nh, 0);
        std::vector<double> hc, hsv((size_t)nh * 8, 0.0);
        size_t tT = 0, tP = 0, tO = 0;
        for (int k = 0; k < nh; k++) { const int w = hostw[k]; hP[k] = Pn[w]; hM[k] = Mn[w]; hO[k] = On[w]; hc.insert(hc.end(), cw.begin() + 4 * w, cw.begin() + 4 * w + 4); tT += 6 * (size_t)Pn[w] + 3 * (size_t)Mn[w]; tP += Pn[w]; tO += On[w]; }
        std::vector<double> th(tT + 1), px(2 * tO + 2);
        std::vector<uint8_t> tc(tP + 1), ol(tO + 1, 0);
        std::vector<int64_t> pi(tO + 1), li(tO + 1);
        size_t aT = 0, aP = 0, aO = 0;
        for (int k = 0; k < nh; k++) {
            const int w = hostw[k]; const size_t n = 6 * (size_t)Pn[w] + 3 * (size_t)Mn[w], O = On[w];
            HIP_TRY(ctx, hipMemcpyAsync(th.data() + aT, e_th.at(blk) + wins[w].theta0, n * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(tc.data() + aP, e_tc.at(blk) + wins[w].pose0, (size_t)Pn[w], hipMemcpyDeviceToHost, ctx->stream));
            if (O) {
                HIP_TRY(ctx, hipMemcpyAsync(px.data() + 2 * aO, e_px.at(blk) + 2 * (size_t)wins[w].obs0, O * 16, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(pi.data() + aO, e_pi.at(blk) + wins[w].obs0, O * 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(li.data() + aO, e_li.at(blk) + wins[w].obs0, O * 8, hipMemcpyDeviceToHost, ctx->stream));
            }
            aT += n; aP += Pn[w]; aO += O;
        }
        HIP_TRY(ctx, slam_stream_wait(ctx->stream));
        rc = slam_local_ba_batch(ctx, nh, hc.data(), hP.data(), hM.data(), hO.data(), th.data(), tc.data(), px.data(), pi.data(), li.data(), ol.data(),
                                 iters_fast, iterations, repr_eps, hsv.data(), hst.data());
        if (rc) return rc;
        aT = 0; aO = 0;
        for (int k = 0; k < nh; k++) {
            const int w = hostw[k]; const size_t n = 6 * (size_t)Pn[w] + 3 * (size_t)Mn[w], O = On[w];
            wst[w] = hst[k]; memcpy(wsv.data() + 8 * (size_t)w, hsv.data() + 8 * (size_t)k, 64);
            if (hst[k] == SLAM_OK) {
                HIP_TRY(ctx, hipMemcpyAsync(e_th.at(blk) + wins[w].theta0, th.data() + aT, n * 8, hipMemcpyHostToDevice, ctx->stream));
                if (O) HIP_TRY(ctx, hipMemcpyAsync(e_ol.at(blk) + wins[w].obs0, ol.data() + aO, O, hipMemcpyHostToDevice, ctx->stream));
            }
            aT += n; aO += O;
        }
        HIP_TRY(ctx, slam_stream_wait(ctx->stream));             // (the host vectors end with this scope)
    }
    // the update, for the windows that were solved: the existing kernels on the arrays where they lie
    KfmUpd *uh = (KfmUpd *)e_upd.at(h);                          // (the pinned block: its earlier copy has completed -- the batch waited)
    int nu = 0, umaxM = 1;
    for (int w = 0; w < nw; w++) {
        const int s = wins[w].s;
        status[s] = wst[w];
        if (stats) memcpy(stats + 8 * (size_t)s, wsv.data() + 8 * (size_t)w, 64);
        if (wst[w] != SLAM_OK) continue;
        uh[nu++] = {s, wins[w].theta0, (long long)wins[w].obs0};
        umaxM = std::max(umaxM, (int)Mn[w]);
    }
    if (nu == 0) return SLAM_OK;
    HIP_TRY(ctx, hipMemcpyAsync(e_upd.at(blk), uh, (size_t)nu * sizeof(KfmUpd), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(km->pin_ev, ctx->stream));
    rc = kfmap_update_enqueue(ctx, km, ks, e_upd.at(blk), nu, umaxM, e_th.at(blk), e_ol.at(blk));
    if (rc) return rc;
    for (int k = 0; k < nu; k++) km->pend[uh[k].s].valid = 0;
    return SLAM_OK;
}
// P, M, O of the window each stream had in the last slam_kfmap_local_ba (zeros: none), S x 3 ints; host bookkeeping, no device work
int slam_kfmap_last_windows(slam_kfmap *km, int32_t *pmo)
{
    if (!km || !pmo) return SLAM_ERR_ARG;
    for (int s = 0; s < km->v.S; s++) for (int k = 0; k < 3; k++) pmo[3 * s + k] = km->last_win[s][k];
    return SLAM_OK;
}

int slam_kfmap_filter(slam_ctx *ctx, slam_kfmap *km, const double *filtering_ratio, const int32_t *min_cov_score, int first_kfid, uint64_t *removed)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && filtering_ratio != nullptr && min_cov_score != nullptr && first_kfid >= 0);
    const KfmapView &V = km->v;
    const int S = V.S;
    for (int s = 0; s < S; s++)                                  // every check before anything is enqueued
        if (!(std::isfinite(filtering_ratio[s]) || filtering_ratio[s] >= 1.0) || min_cov_score[s] < 0)
            return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_filter: stream %d: filtering_ratio %g (finite or >= 1), min_cov_score %d (>= 0)", s, filtering_ratio[s], (int)min_cov_score[s]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int list[128];
    const int ns = kfmap_streams(km, list);
    if (removed) memset(removed, 0, (size_t)S * 8);
    if (ns == 0) return SLAM_OK;
    Layout D;
    const auto o_sel = D.take<int>(S), o_minc = D.take<int>(S); const auto o_ratio = D.take<double>(S);
    char *scr, *h;
    int rc = kfmap_upload(ctx, km, D.size(), &scr, [&](char *h) {
        kfmap_put_streams(o_sel, h, list, ns); memcpy(o_minc.at(h), min_cov_score, (size_t)S * 4); memcpy(o_ratio.at(h), filtering_ratio, (size_t)S * 8);
    });
    if (rc) return rc;
    { ProfScope span(ctx, "kfmap_filter");
      KFM_LAUNCH_ROWS(km, k_kfm_filter, dim3(ns), (const double *)o_ratio.at(scr), (const int *)o_minc.at(scr), first_kfid, (const int *)o_sel.at(scr)); }
    HIP_TRY(ctx, hipGetLastError());
    if (!removed) return SLAM_OK;
    rc = slam_pinned(ctx, (size_t)S * 8, (void **)&h);
    if (rc) return rc;
    rc = kpset_read_back(ctx, h, {{0, V.frem, (size_t)S * 8, nullptr}});
    if (rc) return rc;
    for (int k = 0; k < ns; k++) memcpy(&removed[list[k]], h + (size_t)list[k] * 8, 8);       // (a stream the call did not act on keeps its 0)
    return SLAM_OK;
}

int slam_kfmap_remove_keyframe(slam_ctx *ctx, slam_kfmap *km, int s, int kfid)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && kfid >= 0);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    int cur = 0;                                                 // the argument check needs the stream's newest id, which the device alone knows: one 4-byte read
    HIP_TRY(ctx, hipMemcpyAsync(&cur, V.cur + s, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    if (cur >= 1 && kfid == cur - 1) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_remove_keyframe: key-frame %d is the newest of stream %d", kfid, s);
    if (kfid >= cur || kfid + V.R < cur) return SLAM_OK;         // never added, or long forgotten: not in the ring
    { ProfScope span(ctx, "kfmap_remove");
      KFM_LAUNCH_ROWS(km, k_kfm_remove, dim3((V.cap + 255) / 256), s, kfid);
      hipLaunchKernelGGL(k_kfm_drop_slot, dim3(1), dim3(1), 0, ctx->stream, V, s, kfid); }
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

int slam_kfmap_newest(slam_ctx *ctx, slam_kfmap *km, int32_t *newest)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && newest != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(newest, km->v.cur, (size_t)km->v.S * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    for (int s = 0; s < km->v.S; s++) newest[s] -= 1;
    return SLAM_OK;
}

int slam_kfmap_download_keyframe(slam_ctx *ctx, slam_kfmap *km, int s, int kfid, double *theta, int64_t *ids, double *upx_yx, uint8_t *live, int cap_out, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && kfid >= 0 && n_out != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const size_t sr = (size_t)s * V.R + kfid % V.R;
    int tn[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&tn[0], V.tag + sr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&tn[1], V.kn + sr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    if (tn[0] != kfid + 1) { *n_out = -1; return SLAM_OK; }      // not in the ring (never added, or forgotten)
    const int n = tn[1];
    *n_out = n;
    if (n > cap_out) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_kfmap_download_keyframe: %d observations but cap = %d", n, cap_out);
    if (theta) HIP_TRY(ctx, hipMemcpyAsync(theta, V.ktheta + 6 * sr, 48, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 0 && ids) HIP_TRY(ctx, hipMemcpyAsync(ids, V.kid + sr * V.cap, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 0 && upx_yx) HIP_TRY(ctx, hipMemcpyAsync(upx_yx, V.kupx + 2 * sr * V.cap, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 0 && live) HIP_TRY(ctx, hipMemcpyAsync(live, V.klive + sr * V.cap, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    return SLAM_OK;
}

// the raw-pixel store: as large as kupx, and a copy of it for whatever was recorded before the call (the raw pixel of a pinhole observation)
int slam_kfmap_enable_pixels(slam_ctx *ctx, slam_kfmap *km)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr);
    if (km->kpx) return SLAM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const size_t bytes = (size_t)V.S * V.R * V.cap * 16;
    if (km->mg_base) {                                           // the merge scratch was laid out without the raw pixels' slab: the next merge makes it anew.
        HIP_TRY(ctx, hipDeviceSynchronize());                    // First, while the store is still off: a failure here leaves the map as it was
        (void)hipFree(km->mg_base); km->mg_base = nullptr; km->mg = KfmMerge{};
    }
    double *px = nullptr;
    hipError_t e = hipMalloc((void **)&px, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(px, V.kupx, bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = slam_stream_wait(ctx->stream);
    if (e != hipSuccess) { if (px) (void)hipFree(px); return slam_fail(ctx, SLAM_ERR_HIP, "slam_kfmap_enable_pixels: %s", hipGetErrorString(e)); }
    km->kpx = px;                                                // published last: every later layout and launch sees the store whole
    return SLAM_OK;
}

int slam_kfmap_download_pixels(slam_ctx *ctx, slam_kfmap *km, int s, int kfid, double *px_yx, int cap_out, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && kfid >= 0 && n_out != nullptr);
    if (!km->kpx) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_download_pixels: raw pixels are not enabled (slam_kfmap_enable_pixels)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const size_t sr = (size_t)s * V.R + kfid % V.R;
    int tn[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&tn[0], V.tag + sr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&tn[1], V.kn + sr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    if (tn[0] != kfid + 1) { *n_out = -1; return SLAM_OK; }      // not in the ring (never added, or forgotten)
    const int n = tn[1];
    *n_out = n;
    if (n > cap_out) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_kfmap_download_pixels: %d observations but cap = %d", n, cap_out);
    if (n > 0 && px_yx) {
        HIP_TRY(ctx, hipMemcpyAsync(px_yx, km->kpx + 2 * sr * V.cap, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    }
    return SLAM_OK;
}

int slam_kfmap_download_points(slam_ctx *ctx, slam_kfmap *km, int s, int64_t *ids, double *xyz, uint8_t *flags, int32_t *obs_off, int32_t *obs_kf,
                               int cap_out, int cap_obs, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && n_out != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const size_t m = V.mcap, pb = (size_t)s * m;
    std::vector<unsigned long long> tag(m), mask(m);
    std::vector<double> pos(3 * m);
    std::vector<uint8_t> fl(m);
    std::vector<int> ring(V.R);
    HIP_TRY(ctx, hipMemcpyAsync(tag.data(), V.ptag + pb, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(mask.data(), V.pmask + pb, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(pos.data(), V.pxyz + 3 * pb, m * 24, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(fl.data(), V.pflags + pb, m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ring.data(), V.tag + (size_t)s * V.R, (size_t)V.R * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    std::vector<std::pair<int64_t, size_t>> live;
    size_t nobs = 0;
    for (size_t e = 0; e < m; e++) if (tag[e] && !(fl[e] & KFM_DEAD)) { live.push_back({(int64_t)(tag[e] - 1), e}); nobs += __builtin_popcountll(mask[e]); }
    std::sort(live.begin(), live.end());
    *n_out = (int)live.size();
    if ((int)live.size() > cap_out || (obs_kf && nobs > (size_t)cap_obs))
        return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_kfmap_download_points: %zu points with %zu observers, caps %d and %d", live.size(), nobs, cap_out, cap_obs);
    int at = 0;
    for (size_t k = 0; k < live.size(); k++) {
        const size_t e = live[k].second;
        if (ids) ids[k] = live[k].first;
        if (xyz) for (int c = 0; c < 3; c++) xyz[3 * k + c] = pos[3 * e + c];
        if (flags) flags[k] = fl[e];
        if (obs_off) obs_off[k] = at;
        std::vector<int> kf;
        for (int b = 0; b < V.R; b++) if ((mask[e] >> b & 1) && ring[b]) kf.push_back(ring[b] - 1);
        std::sort(kf.begin(), kf.end());
        for (int o : kf) { if (obs_kf) obs_kf[at] = o; at++; }
    }
    if (obs_off) obs_off[live.size()] = at;
    return SLAM_OK;
}

int slam_kfmap_reset(slam_ctx *ctx, slam_kfmap *km, int s)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    // an empty ring, an empty table, no key-frame yet, no window: the tags alone decide what the rest means
    HIP_TRY(ctx, hipMemsetAsync(V.tag + (size_t)s * V.R, 0, (size_t)V.R * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(V.ptag + (size_t)s * V.mcap, 0, (size_t)V.mcap * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(V.pflags + (size_t)s * V.mcap, 0, (size_t)V.mcap, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(V.pmask + (size_t)s * V.mcap, 0, (size_t)V.mcap * 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(V.cur + s, 0, 4, ctx->stream));
    if (V.dhas) HIP_TRY(ctx, hipMemsetAsync(V.dhas + (size_t)s * V.mcap, 0, (size_t)V.mcap, ctx->stream));
    if (km->v.rkey) {                                            // no rows, nothing dropped (the rows' bits mean nothing without their keys)
        HIP_TRY(ctx, hipMemsetAsync(km->v.rkey + (size_t)s * V.mcap * km->v.D, 0, (size_t)V.mcap * km->v.D * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(km->v.rdrop + s, 0, 4, ctx->stream));
    }
    HIP_TRY(ctx, hipMemsetAsync(V.whdr + (size_t)s * KFM_HDR, 0, KFM_HDR * 4, ctx->stream));
    if (km->hs_base) {                                           // the stream's stored sets, their owners and the shadow tags (= the emptied table's)
        const KfmHist &H = km->hs;
        HIP_TRY(ctx, hipMemsetAsync(H.bits + (size_t)s * H.W * V.R, 0, (size_t)H.W * V.R * 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(H.htag + (size_t)s * V.R, 0, (size_t)V.R * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(H.shadow + (size_t)s * V.mcap, 0, (size_t)V.mcap * 8, ctx->stream));
    }
    km->pend[s].valid = 0; km->lm_np[s] = 0;
    return SLAM_OK;
}

}  // extern "C"

#include "kfmap_lmm.inc"
#include "kfmap_merge.inc"
#include "kfmap_tri.inc"
