// kfmap.hpp -- the per-stream key-frame map of S lock-stepped streams (slam_kfmap, kfmap.hip): what the estimator's _get_ba_parameters /
// _update_ba_parameters! (src/estimator.jl:143-306) read and write of the map manager's dictionaries, held in HBM beside the keypoint lists.
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
#pragma once
#include "kpset.hpp"

constexpr int KFM_MAX_R = 64;
constexpr uint8_t KFM_3D = 1, KFM_OBS = 2, KFM_BA = 4, KFM_GONE = 8, KFM_DEAD = 16;
constexpr int KFM_HDR = 8;            // ints per pending-window header: status, kfid, P, M, O, min_cov_score, number of bad points, 0
constexpr int N_COVISIBLE = 5;        // local_bundle_adjustment!: up to 5 latest covisible key-frames (estimator.jl:317-335)

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
};

struct slam_kfmap {
    int device = 0;
    char *base = nullptr; size_t bytes = 0;
    KfmapView v = {};
    // the streams the last add_keyframe acted on (the set's selection at that call): gather's streams
    int n_sel = KPSEL_ALL; uint8_t sel_host[128] = {};
    struct Pending { int valid = 0, kfid = -1, P = 0, M = 0, O = 0; } pend[128];      // host copy of the pending windows' sizes
    // update's staging (theta, outlier flags, window table): a pinned block of the map's own with the event of the copy that last read it
    char *pin = nullptr; size_t pin_bytes = 0; hipEvent_t pin_ev = nullptr;
};
