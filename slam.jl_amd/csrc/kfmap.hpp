// kfmap.hpp -- the per-stream key-frame map of S lock-stepped streams (slam_kfmap, kfmap.hip): what the estimator's _get_ba_parameters /
// _update_ba_parameters! (src/estimator.jl:143-306) read and write of the map manager's dictionaries, held in HBM beside the keypoint lists.
//
// The integer logic of the map (entry of an id, search in a slab, the serial decisions over a ring's slots) is kfmap_ring.hpp, included below: plain C++
// for host and device.  Every allocation's regions are named once, in a *_regions(km, base) function built on Layout::bind (layout.hpp).
//
// ONE allocation, every region starting on a 256-byte boundary (Layout); with n = S R cap, m = S mcap its size is the sum, each term rounded up to 256, of
//   ring    tag 4 S R | n_kf 4 S R | theta 48 S R | ids 8 n | upx 16 n | live n | fresh S cap
//   table   tag 8 m | xyz 24 m | observers 8 m | flags m
//   state   cur 4 S | removed mask 8 S
//   window  header 32 S | tags, pose order, rank, constant 4 S R each | covmap mask 8 S | point ids 8 m | point observers 8 m | obs offsets 4 m | entry -> window 4 m
// i.e. about 25 R cap + 65 mcap bytes per stream (cap 1 400, R 32, mcap 16 384: 2.2 MB).
//
// Ring: key-frame k of stream s lives in slot k % R while tag == k + 1 (0: empty).  Its slab holds the list as it was (ids ascending: ids are per-stream
// and ascending, compaction is stable), the undistorted pixel (y, x) and a live byte per observation -- a removed observation is a tombstone, the slab stays
// sorted and a lookup is a binary search.  Reusing a slot forgets the old key-frame: every point it observed loses that observer bit (remove_keyframe!,
// map_manager.jl:184-209); slam_kfmap_filter and slam_kfmap_remove_keyframe empty a slot the same way (tag 0, length 0) before its turn comes.
// Table: point `id` lives in entry id % mcap while tag == id + 1.  A newer id replaces an older one; the old point is then gone and its observations in the
// slabs are orphans (looked up, not found, skipped like a missing dictionary entry).  observers: bit k % R, meaningful only while that slot's tag matches -- the
// forgetting rule keeps the two in step.  flags: KFM_3D is_3d, KFM_OBS `observed` = seen by the LAST key-frame added (set by add_keyframe, cleared by update;
// NOT refreshed every frame as the reference's is_observed is), KFM_BA position set by a bundle adjustment, KFM_GONE the id has left the current frame (an
// outlier observation of the window's own key-frame, an observed point that was removed): later lists that still carry it are not recorded, KFM_DEAD the
// point was removed (the entry keeps its tag so that KFM_GONE outlives it).
//
// Descriptors (slam_kfmap_enable_descriptors; a second allocation, made by that call): one 256-bit row and a "has descriptor" byte per table entry,
// 33 mcap bytes per stream.  The row of point `id` lives at entry id % mcap under the table's ownership rule: slam_kfmap_add_descriptors writes it only
// where the entry carries that id, and an entry that changes owner (a larger id claims it, or a removed id is recorded anew) loses the byte with the point.
// Without the row store (below) ONE descriptor per point is the whole of the reference's keyframes_descriptors: map_manager.jl:116-131 describes only the
// keypoints a key-frame has just extracted, and further rows would come from merges: slam_kfmap_merge then keeps the new point's own row and lets prev's
// row go with prev (the reference appends prev's rows to keyframes_descriptors, and mappoint_min_distance takes the minimum over all of them).
//
// Descriptor rows (slam_kfmap_enable_descriptor_rows, kfmap_lmm.inc; an allocation of its own, made by that call; needs the descriptors): keyframes_descriptors
// (map_point.jl:15), one row per key-frame id, D = 2 .. 8 slots per table entry.  With m = S mcap, each region rounded up to 256:
//   keys     4 m D    key-frame id + 1 of the slot's row (0: an empty slot)
//   rows     32 m D   the slot's 256-bit row
//   dropped  4 S      rows the bound D has dropped on the stream
// i.e. about 36 D mcap bytes per stream (D 4, mcap 16 384: 2.4 MB; S = 128: 300 MB).  Slots may have holes; readers take the non-empty slots ascending by key.
// The row-set logic is kfmap_ring.hpp's kfm_rows_*.  dhas becomes the reference's "mp.descriptor is not empty": set by add_descriptors (and by a merge
// that hands a point its first row), cleared when the entry changes owner and when the point's last valid observer goes; a described point without a row is
// legal, staged with an empty row range and never chosen.  ddesc stays what add_descriptors wrote and is not staged.  Upkeep, every kernel a <bool ROWS>
// instantiation (a map without the store launches the <false> kernels, which are the kernels as they were):
//   add_descriptors   the row also goes under the key of the stream's newest key-frame (add_mappoint!'s current_keyframe_id; add_descriptor!: a key the
//                     point already has is skipped)
//   observers         wherever an observer bit of a live, owned point is cleared -- kfm_forget_slab (ring reuse in k_kfm_forget, the filter's closing pass,
//                     k_kfm_remove), the outlier tombstone of k_kfm_upd_obs, the vanished pixel of k_kfm_plan -- the row keyed by that slot's key-frame goes;
//                     no valid observer left: all keys and dhas are cleared (remove_kf_observation!, map_point.jl:88-122).  Several slabs may lose one point
//                     concurrently (the filter): a thread zeroes its own key's slot, the clear-all is the thread's whose atomicAnd left no observer
//   owners            k_kfm_record clears the keys of an entry that takes a new owner; slam_kfmap_reset clears the stream's rows and counter
//   merge             the pair's thread of k_kfm_merge_resolve forms the union of new's and prev's rows by key (the pair owns both entries); on an equal key
//                     new's row stays; prev's keys are cleared with the point (map_manager.jl:410-412)
//   match             the stager writes every row of a local-map point and of a keypoint ascending by key, mp_doff / kp_doff are a scan of the row counts,
//                     the staging's descriptor regions hold D rows per record (DR in the formula below); k_lmm_match is untouched
// Deviations: the bound -- a union of more than D rows keeps the D rows with the LARGEST keys, whatever the order of slots, arrivals or pairs, and the excess
// is added to the stream's counter; the reference's most representative `descriptor` (map_point.jl:98-120, :132-144) is read by nothing but the emptiness test
// and is not modelled; a reused ring slot counts as remove_keyframe!.
//
// Raw pixels (slam_kfmap_enable_pixels; an allocation of its own, made by that call): kpx [S R cap][2], kp.pixel (y, x) of every observation beside
// kupx, 16 S R cap bytes (cap 1 400, R 32: 0.7 MB per stream; S = 128: 92 MB).  It is not part of the view: KfmapView / KfmapRows, hence the
// argument block of every kernel that does not deal with pixels, are what they were.  The three kernels that keep or read the store take the pointer by
// value, nullptr while the store is off; a map without it launches the same kernels on the same views, but THEIR argument blocks have grown -- k_kfm_record
// (both ROWS forms) by a trailing parameter, the merge kernels by two trailing members of KfmMerge, the stagers by a trailing member of KfmLm -- and
// k_kfm_record / k_kfm_merge_slabs test the pointer (uniform) where they had no branch.  Their results for such a map are unchanged:
//   k_kfm_record        files the list's pixel as it is beside undistort_px of it
//   k_kfm_merge_slabs   moves it with the observation (KfmMerge::kpx / t_px; the merge scratch grows by 16 S R cap bytes)
//   k_kfm_lm_stage(_hist)   read kp_yx and kp_oyx -- hence the cell grid, add_keypoint_to_grid! -- through KfmLm::px_src: kpx with the store, else kupx
// The gather, the update, the filter and slam_kfmap_triangulate_temporal read kupx.  A tombstone keeps its raw pixel as it keeps its undistorted one.
//
// Local-map staging (slam_kfmap_local_map_match, kfmap_lmm.inc; a third allocation, made by the first call and re-made when max_local or the grid grows):
// the packed buffer of k_lmm_match (lmm_host.hpp) with FIXED per-stream strides -- no count pass, no scan over the streams, hence no host round trip between
// staging and match.  With N1 = cap + 1, M1 = max_local + 1, C1 = the call's largest cell count + 1, per stream, each region rounded up to 256 over S:
//   keypoints   N1 (16 yx + 4 + 4 offsets + 32 DR descriptors + 8 id + 4 cell list + 8 key) + 20 N1 R observers (row, pixel)
//   key-frames  128 R
//   local map   M1 (24 xyz + 4 + 4 offsets + 32 DR descriptors + 8 id + 4 + 8 + 16 best_kp, best_dist, proj_yx) + 4 M1 R observers
//   cells       8 C1 (offsets, cursors) | mark 4 mcap | LmmStream 280 | counts 8
//   results     status 4 | pairs 4 | cap (16 ids + 8 distance)
// (DR = 1 descriptor row per record, or D with the row store) i.e. about cap (68 + 32 DR + 20 R) + max_local (68 + 32 DR + 4 R) + 4 mcap bytes per
// stream (cap 1 400, R 32, max_local 14 000, mcap 16 384, DR 1: 4.3 MB; S = 128: 550 MB; DR 4: 5.8 MB; 740 MB).  The observer regions are sized for the worst case (every point seen by every key-frame of the ring); they are what a count -> scan -> emit
// staging would save, at the price of a second pass over the table and a scan launch.
//
// Deviations of slam_kfmap_local_map_match from update_frame_covisibility! + match_local_map! (map_manager.jl:302-355, mapper.jl:265-462):
//   distortion    find_best_match and the frame grid use kp.pixel with project_world_to_image_distort.  With the raw-pixel store (above) so does the
//                 match, for any lens.  Without it the slabs hold UNDISTORTED pixels only; the two coincide only without lens distortion, so a
//                 stream with non-zero k1, k2, p1, p2 is then an argument error
//   persistence   without slam_kfmap_enable_local_map_history frame.local_map_ids is not kept between key-frames (the local map is what this key-frame's
//                 covisibility pass yields).  With it (below) the replace-or-union rule (map_manager.jl:350-354) and the union with the oldest covisible
//                 key-frame's local map (mapper.jl:274-286) hold, with three differences: a stored set holds the ids that passed the match's gates
//                 when it was stored (the reference stores raw ids and gates at match time; an id that fails a gate never passes one later, so only the
//                 sizes the two rules compare can differ), an id whose table entry another id has taken leaves every stored set (the purge), and
//                 "oldest" is the covisible key-frame of the smallest id (the reference takes the first key of a Dict)
//   clean-ups     no remove_mappoint_obs! clean-ups (mapper.jl:412, :429-434), as in the array form: a missing or dead observation is skipped
//   merges        the call reports pairs and changes nothing in the map: slam_kfmap_merge (below) applies them
//   order         the local map is walked ascending by id (the reference iterates a Set); among equal distances the larger local-map index wins
//   grid          a keypoint whose pixel lies in no cell of the grid is in no cell list (the array form rejects such a call)
//
// Local-map history (slam_kfmap_enable_local_map_history, kfmap_lmm.inc; an allocation of its own, made by that call): frame.local_map_ids of every
// key-frame of the ring as a bitset over the table's entries -- a point is named by its entry, the id is the entry's tag.  With W = ceil(mcap / 64), each
// region rounded up to 256 over S:
//   sets     8 S W R   word w of slot b's set at [s][w][b]: the R words of one group of 64 entries are adjacent
//   owners   4 S R     the key-frame id + 1 a slot's set belongs to (0: none; a key-frame whose match was skipped leaves its slot's set to the old one)
//   shadow   8 S mcap  the table's tags as of the stream's last match: an entry whose tag differs has changed owner, its bit goes from all R sets
// i.e. about R mcap / 8 + 8 mcap bytes per stream (R 32, mcap 16 384: 192 KB; S = 128: 25 MB).  Storing ids instead would cost 8 R max_local per stream
// (S = 128: 460 MB).  A match with history sweeps a stream's sets and shadow twice (k_kfm_lm_stage_hist); without the call nothing of this exists and the
// match launches the kernels it always did.  Sets grow along the chain, so max_local >= mcap (status 2 cannot occur) is the setting to use with it.
// P of the replace-or-union rule is non-empty only when the match runs twice for one key-frame: in the reference the key-frame is a deepcopy of a current
// frame whose set is never written (map_manager.jl:174).  slam_kfmap_merge does not touch the sets (prev_id goes at the next purge once a larger id takes
// its entry, and is gated out meanwhile: it is dead); slam_kfmap_reset clears the stream's.
//
// Merge scratch (slam_kfmap_merge, kfmap_merge.inc; a fourth allocation, made by the first merge call that has pairs): merge_matches -> merge_mappoints ->
// update_keypoint! (mapper.jl:296-310, map_manager.jl:378-427, frame.jl:290-307) renames a keypoint in every key-frame that observes it, and every slab
// and live list is sorted by id, so the touched slabs and lists are rebuilt in order through scratch.  With Z = S (R + 1) (a stream's R slabs, then its
// list), n = S R cap, l = S cap, each region rounded up to 256:
//   renames   count 4 Z | position 4 Z cap | new id 8 Z cap | new ids ascending 8 Z cap | rank by position 4 Z cap | kept before 4 Z (cap + 1)
//   slabs     ids 8 n | upx 16 n | live n | raw px 16 n (with the raw-pixel store)
//   pairs     applied l | counts 16 S
//   lists     yx, stereo yx, key-frame yx, first yx 16 l each | xyz 24 l | id 8 l | is3d, stereo, haskf l each | first key-frame 4 l
// i.e. about (53 R + 132) cap bytes per stream (cap 1 400, R 32: 2.6 MB; S = 128: 330 MB; with raw pixels 69 R + 132: 3.3 MB; 420 MB).  The main
// allocation's layout is untouched.
// slam_kfmap_merge against the reference (the first three are deviations, the last two the reference's own rules as they show in slabs):
//   covisibility  add_covisibility! has no counterpart: covisibility is derived from the observer masks (as for the filter's remove_covisible_kf!)
//   descriptors   without the row store one row per point: new keeps its own, prev's goes with prev; with it new takes prev's rows by key (above)
//   gone          without a keypoint set (ks == NULL) prev's entry is also marked KFM_GONE, so that later lists that still carry prev_id are not
//                 recorded as a fresh point (the reference always has the current frame at hand)
//   orphans       pop!(map_points, prev_id) is not remove_mappoint!: where a slab holds both ids (has_new) prev's observation stays, alive, without a point
//   tombstones    a tombstone whose id equals an arriving new_id is dropped from the slab (a lower bound must not land on it); the slab shrinks by one
//
// Temporal triangulation (slam_kfmap_triangulate_temporal, kfmap_tri.inc; no allocation: S R 64 doubles of observer matrices and 4 S counters in the
// context's scratch): triangulate_temporal! (mapper.jl:185-262) for the newest key-frame's 2-D points, each against its FIRST observer as the mask names it
// now (kfm_first_observer, kfmap_ring.hpp) and with both poses from ktheta, i.e. as the last bundle adjustment left them.  Accepted: pxyz, KFM_3D (not
// KFM_BA), and the list slot that carries the id (binary search).  Rejected: a tombstone in the newest slab, observer bit cleared, with rows the row keyed k.
// Deviations from the reference:
//   list          the live list KEEPS a rejected keypoint, as the reference's current frame does (slam_kpset_triangulate_temporal compacts it away)
//   clean-ups     no remove_mappoint_obs! clean-up for a missing point (mapper.jl:209-210), as elsewhere in the map: an orphan is skipped and left as it is
//   first         the first observer is the smallest key-frame id among the point's valid observer bits (the reference's observers are an ordered set)
#pragma once
#include "kpset.hpp"
#include "kfmap_ring.hpp"
#include "lmm_host.hpp"

constexpr int KFM_MAX_R = 64;
constexpr uint8_t KFM_3D = 1, KFM_OBS = 2, KFM_BA = 4, KFM_GONE = 8, KFM_DEAD = 16;
constexpr int KFM_HDR = 8;            // ints per pending-window header: status, kfid, P, M, O, min_cov_score, number of bad points, 0

// passed by value to every kernel of kfmap.hip: the order of the members is their kernel-argument layout
struct KfmapView {
    int S, cap, R, mcap;
    int *tag, *kn;                        // [S R] key-frame id + 1 (0: empty), observations in the slab
    double *ktheta;                       // [S R][6] get_cw_ba: RotZYX angles of Rcw, tcw
    int64_t *kid;                         // [S R cap] keypoint ids, ascending
    double *kupx;                         // [S R cap][2] undistorted pixel (y, x)
    uint8_t *klive;                       // [S R cap] 0: tombstone
    uint8_t *kfresh;                      // [S cap] add_keyframe's claim pass -> record pass: 0 known point, 1 new point, 2 not recorded (KFM_GONE)
    unsigned long long *ptag;             // [S mcap] point id + 1 (0: empty)
    double *pxyz;                         // [S mcap][3]
    unsigned long long *pmask;            // [S mcap] observer bits
    uint8_t *pflags;                      // [S mcap] KFM_*
    int *cur;                             // [S] newest key-frame id + 1
    unsigned long long *frem;             // [S] the last slam_kfmap_filter's removals: bit k % R per removed key-frame
    // the pending window of a stream: what slam_kfmap_ba_update needs of the last gather
    int *whdr;                            // [S][KFM_HDR]
    int *wtag, *worder, *wrank, *wconst;  // [S R] the ring's tags at the gather; a slot's 1-based pose id in the window (0: none); its rank by key-frame id; theta_const
    unsigned long long *wcov;             // [S] slots in the covisibility map
    int64_t *wpid;                        // [S mcap] point ids in window order from the front, the gather's `bad` ids from the back
    unsigned long long *wpmask;           // [S mcap] the point's observers in the window
    int *wpoff;                           // [S mcap] index of its first observation
    int *went;                            // [S mcap] by table entry: 0 untouched, -1 bad, j + 1 = point j of the window
    // the descriptor store (nullptr until slam_kfmap_enable_descriptors)
    uint64_t *ddesc;                      // [S mcap][4] the 256-bit row of the entry's point
    uint8_t *dhas;                        // [S mcap] 1: the row belongs to the entry's current owner (with rows: the point's `descriptor` is not empty)
};
// the view with the row store (slam_kfmap_enable_descriptor_rows): keyframes_descriptors, D slots per entry (kfmap_ring.hpp's kfm_rows_*).  Only the
// <true> instantiations of the <bool ROWS> kernels take it; every other kernel takes the KfmapView in it, so a map without rows launches the kernels it
// always did with the argument block they always had.
struct KfmapRows : KfmapView {
    int32_t *rkey;                        // [S mcap][D] key-frame id + 1 of the slot's row (0: empty; nullptr: the store is off)
    uint64_t *rrow;                       // [S mcap][D][4]
    int32_t *rdrop;                       // [S] rows dropped by the bound D so far
    int D;                                // rows per point (0: the store is off)
};
template <bool ROWS> struct KfmViewOf { using type = KfmapView; };
template <> struct KfmViewOf<true> { using type = KfmapRows; };
template <bool ROWS> using KfmView = typename KfmViewOf<ROWS>::type;

// what the host works out per stream for a staged local-map call (everything of LmmStream that does not depend on the map)
struct KfmLmArg { double cam[10], max_proj, start, view_thr; int32_t cell, gr, gc, pad; };
// the staged call's regions (kfmap.hpp's size formula), by value to the staging kernels; stream s owns [s N1, ..) of the keypoint regions, [s M1, ..) of
// the local-map regions, [s R, ..) of the key-frame rows, [s C1, ..) of the cell regions, [s N1 R, ..) / [s M1 R, ..) of the observer regions
struct KfmLm {
    int N1, M1, C1, max_local;
    int DR;                               // descriptor rows a record's share of kp_desc / mp_desc holds: 1, or D with the row store
    LmmStream *st;                        // [S] by LAUNCH index: row z is the z-th stream acted on
    double *kp_yx; int32_t *kp_doff; uint64_t *kp_desc; int32_t *kp_ooff, *kp_okf; double *kp_oyx; int64_t *kp_id;
    double *kf_Tcw;
    double *mp_xyz; int32_t *mp_doff; uint64_t *mp_desc; int32_t *mp_ooff, *mp_okf; int64_t *mp_id;
    int32_t *cell_off, *cell_kp, *cell_cur;
    int32_t *best_kp; double *best_dist, *proj;
    unsigned long long *keys;
    int32_t *mark;                        // [S mcap] 1: the entry's point is in the local map
    int32_t *cnt;                         // [S][2] N, M of the last staging (0, 0 unless status 0)
    int32_t *status, *rn; int64_t *rpairs; double *rdist;        // results, one block: [S] | [S] | [S cap][2] | [S cap]
    const double *px_src;                 // [S R cap][2] where kp_yx / kp_oyx come from: the slabs' raw pixels (slam_kfmap_enable_pixels), else kupx
};

// the match kernel's argument block over the staged regions
inline LmmDev kfm_lmm_dev(const KfmLm &Q)
{
    LmmDev L;
    L.st = Q.st; L.kp_yx = Q.kp_yx; L.kp_desc_off = Q.kp_doff; L.kp_desc = Q.kp_desc; L.kp_obs_off = Q.kp_ooff; L.kp_obs_kf = Q.kp_okf; L.kp_obs_yx = Q.kp_oyx;
    L.kf_Tcw = Q.kf_Tcw; L.mp_xyz = Q.mp_xyz; L.mp_desc_off = Q.mp_doff; L.mp_desc = Q.mp_desc; L.mp_obs_off = Q.mp_ooff; L.mp_obs_kf = Q.mp_okf;
    L.cell_off = Q.cell_off; L.cell_kp = Q.cell_kp; L.best_kp = Q.best_kp; L.best_dist = Q.best_dist; L.proj = Q.proj; L.keys = Q.keys;
    return L;
}

// the local-map history's regions (above), by value to k_kfm_lm_stage_hist
struct KfmHist {
    unsigned long long *bits;             // [S W R] the stored sets
    int *htag;                            // [S R] key-frame id + 1 of the slot's set
    unsigned long long *shadow;           // [S mcap] ptag as of the stream's last match with history
    int W;                                // words per set: ceil(mcap / 64)
};

// slam_kfmap_merge's scratch allocation (kfmap_merge.inc), by value to its kernels; Z = S (R + 1): a stream's R slabs, then its list
struct KfmMerge {
    int *cnt;                             // [Z] renames of the slab / list
    int *rn_pos; int64_t *rn_id, *rs_id; int *rank_at, *kept;   // [Z cap] ([Z (cap + 1)]: kept) KfmRename's regions
    int64_t *t_id; double *t_upx; uint8_t *t_live;              // [S R cap] the scratch slabs
    uint8_t *applied;                     // [S cap] per pair: 1 applied
    int32_t *stat;                        // [S][4] pairs applied, pairs skipped, observations renamed, status (1: the pairs are not one-to-one)
    // the scratch record array of the lists [S cap]: every field k_kpset_compact carries
    double *q_yx, *q_syx, *q_xyz, *q_kyx, *q_fyx; int64_t *q_id; uint8_t *q_is3d, *q_stereo, *q_haskf; int *q_fkf;
    // last, so that every member above lies where it did: the raw pixels' scratch slab and the store itself, [S R cap][2] (nullptr both: the store is off)
    double *t_px, *kpx;
};

struct slam_kfmap {
    int device = 0;
    char *base = nullptr; size_t bytes = 0;
    KfmapRows v = {};
    // the streams the last add_keyframe acted on (the set's selection at that call): gather's streams
    int n_sel = KPSEL_ALL; uint8_t sel_host[128] = {};
    struct Pending { int valid = 0, kfid = -1, P = 0, M = 0, O = 0; } pend[128];      // host copy of the pending windows' sizes
    // update's staging (theta, outlier flags, window table): a pinned block of the map's own with the event of the copy that last read it
    char *pin = nullptr; size_t pin_bytes = 0; hipEvent_t pin_ev = nullptr;
    char *dbase = nullptr;                // the descriptor store
    char *rbase = nullptr;                // the row store (nullptr: off)
    double *kpx = nullptr;                // the raw-pixel store [S R cap][2] (nullptr: off)
    char *lm_base = nullptr; size_t lm_bytes = 0, lm_res_off = 0, lm_res_bytes = 0; KfmLm lm = {};        // the local-map staging (lm.max_local, lm.C1: what it was laid out for)
    int lm_np[128] = {};                  // pairs per stream in the result block of the last local-map match, until a merge has consumed them
    char *mg_base = nullptr; size_t mg_bytes = 0; KfmMerge mg = {};       // the merge's scratch
    char *hs_base = nullptr; size_t hs_bytes = 0; KfmHist hs = {};        // the local-map history (nullptr: off)
    char *ba_base = nullptr; size_t ba_bytes = 0;                         // slam_kfmap_local_ba: the windows' arrays in HBM (grow-only)
    int last_win[128][3] = {};            // P, M, O of the window each stream had in the last slam_kfmap_local_ba (0s: none)
};
