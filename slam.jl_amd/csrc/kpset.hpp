// kpset.hpp -- the device-resident keypoint lists (slam_kpset, kpset.hip): the one definition of a keypoint's record, of the set, of the
// per-stream parameter slot, and the plumbing the files that touch a set share (kpset.hip, lk.hip, detect.hip, pose.hip, fivepoint.hip).
#pragma once
#include "common.hpp"
#include "kpset_select.hpp"
#include "geom_device.hpp"
#include <initializer_list>

// The per-keypoint arrays of S lock-stepped streams: stream s owns the slots [s * cap, s * cap + count[s]) of every
// array.  Passed by value to k_kpset_compact, k_kpset_keyframe, detect_append and both triangulation kernels: the order of the
// members is their kernel-argument layout.  A new field goes here, into kpset_regions and into the load and the store block of
// k_kpset_compact (both kpset.hip; tests/test_gpu_kpset_record.py carries every field through both compaction modes).
struct KpsetView {
    double *yx;                  // [S cap][2] pixel (y, x) in the current left image
    double *oyx;                 // [S cap][2] positions returned by the last temporal match (scratch)
    double *syx;                 // [S cap][2] stereo pixel (right image), valid where stereo != 0
    double *xyz;                 // [S cap][3] map point, valid where is3d != 0
    double *kyx;                 // [S cap][2] pixel (y, x) in the previous key-frame, valid where haskf != 0 (slam_kpset_keyframe)
    double *fyx;                 // [S cap][2] pixel (y, x) in the FIRST key-frame that observed the keypoint (the one that detected it)
    int64_t *id;                 // [S cap] keypoint id (per stream, ascending in creation order)
    uint8_t *is3d, *stereo, *st, *haskf;   // [S cap] flags; st: status of the last match (0 lost, 1 tracked, 2 skipped); haskf: the previous key-frame observes the keypoint
    int *fkf;                    // [S cap] id of the first key-frame (per-stream counter), valid where haskf != 0
    int *kfcount;                // [S] number of key-frames created so far = id of the next one
    int *count;                  // [S] list lengths
    int cap;
};

// The per-stream parameters of a call: KP_PAR doubles per stream, staged by kpset_stage_params (keypoint_set.py restates the numbers).
//   [0 .. 15]                     Tcw of the target camera, column-major 4 x 4: the pose prior of a match (k_kpset_match, prior 1)
//   [0 .. 8]                      or R_compensation, dense column-major 3 x 3: k_kfive_gather, k_kpset_frame_stats
//   [KP_PAR_CAM .. + 3]           fx fy cx cy: k_kpset_match, k_kpose_gather, k_kpose_prep and the host's K of slam_kpset_compute_pose, k_kfive_gather, k_kpset_tri_temporal, k_kpset_frame_stats
//   [KP_PAR_DIST .. + 3]          k1 k2 p1 p2: the same kernels but k_kpose_prep
//   [KP_PAR_SHIFT, + 1]           prior shift (y, x): k_kpset_match, prior 2
constexpr int KP_PAR = 32, KP_PAR_CAM = 16, KP_PAR_DIST = 20, KP_PAR_SHIFT = 24;
__device__ __forceinline__ void load_cam(const double *par, double *cam, double *dist) { for (int k = 0; k < 4; k++) { cam[k] = par[KP_PAR_CAM + k]; dist[k] = par[KP_PAR_DIST + k]; } }

// Where a match starts looking for a 3-D keypoint at (py, px) (map_manager.jl:484-504): prior 0 the pixel itself, 1 the projection of its map
// point X through the stream's slot P (Tcw, intrinsics, distortion), 2 the pixel + the slot's shift.  The ONE copy: k_kpset_worklist computes it
// into the keypoint's work record, the record-less prologue of k_kpset_match (SLAMHIP_NO_MATCH_REC) computes it itself -- same operations in the
// same order, no contraction (-ffp-contract=off): the same bits at both sites (tests/test_gpu_match_records.py).
__device__ __forceinline__ void kp_match_prior(int prior, const double *X, const double *P, double py, double px, double &pry, double &prx)
{
    pry = py; prx = px;
    if (prior == 1) {
        const double X0 = X[0], X1 = X[1], X2 = X[2];
        const double cx = ((P[0] * X0 + P[4] * X1) + P[8] * X2) + P[12];
        const double cy = ((P[1] * X0 + P[5] * X1) + P[9] * X2) + P[13];
        const double cz = ((P[2] * X0 + P[6] * X1) + P[10] * X2) + P[14];
        pdn_to_pixel(P + KP_PAR_CAM, P + KP_PAR_DIST, cy / cz, cx / cz, pry, prx);     // project_undistort (camera.jl:79-82)
    } else if (prior == 2) { pry = py + P[KP_PAR_SHIFT]; prx = px + P[KP_PAR_SHIFT + 1]; }
}
__device__ __forceinline__ bool kp_in_image(double y, double x, int H, int W) { return 1 <= y && y <= (double)H && 1 <= x && x <= (double)W; }   // in_image (camera.jl:90-92)

// What k_kpset_match needs of a keypoint before its first level visit, written by k_kpset_worklist for every entry of the work list when
// the caller is a match (KpWorkRecs::rec != nullptr): the match's prologue is then ONE wave-uniform fetch whose address depends on kernel
// arguments alone, instead of the chain ntot -> work[idx] -> yx / is3d / par -> xyz.  Placement: work_order.hpp (work_rec_slot).
struct alignas(16) KpWorkRec {
    double py, px;               // the keypoint's pixel (yx[q])
    double pry, prx;             // its prior (kp_match_prior; the pixel itself for a 2-D keypoint)
    int q, s;                    // slot in the set's arrays, stream
    int flags;                   // KPREC_3D: is3d[q] != 0, KPREC_INSIDE: the prior lies in the image
    int zt;                      // the member of the TARGET batch the match reads: s, or the stream's rank among the selected ones (a compact stereo match)
};
constexpr int KPREC_3D = 1, KPREC_INSIDE = 2;
static_assert(sizeof(KpWorkRec) == 48 && alignof(KpWorkRec) == 16, "the fetch of k_kpset_match (lk.hip) restates the layout");
// the record side of a work-list launch (rec == nullptr: none are written -- the triangulation seams, the pose seams, SLAMHIP_NO_MATCH_REC)
struct KpWorkRecs {
    KpWorkRec *rec; int stride;  // 8 x stride records (work_rec_stride)
    int prior; const double *par, *xyz; const uint8_t *is3d;
    int compact;                 // the caller is a compact stereo match: a record's zt is its workgroup's index in the selected launch, else the stream
};

// The set: the lists (v) and what is not per-keypoint state of them; all arrays but the kf_* ones live in one allocation.
struct slam_kpset {
    int device = 0, S = 0;
    char *base = nullptr;
    KpsetView v = {};
    int *work = nullptr;         // [S cap] live slots, streams back to back (each stream's segment in the order of work_order.hpp)
    int sort_pad = 0;            // power of two >= cap the work list's sort pads a segment to; 0: slot order (decided at creation)
    int *ntot = nullptr;         // [4]: number of live slots, ...
    KpWorkRec *rec = nullptr;    // [8 rec_stride] the work list's records for k_kpset_match (written by the work list of a match; placement: work_order.hpp)
    int rec_stride = 0;          // ceil(S cap / 8)
    int64_t *next_id = nullptr;  // [S]
    // per-stream parameters of a call (prior shift / pose): ring of 8 slots of S x KP_PAR doubles, staged through pinned host
    // memory with an event per slot, so that the enqueue-only calls never wait for an earlier call's copy
    double *par = nullptr, *par_host = nullptr;
    hipEvent_t par_ev[8] = {};
    int par_slot = 0;
    // slam_kpset_frame_stats (allocations of their own, made by its first call): the S x 8 results when the caller passes no buffer, and
    // S x cap parallax terms for the streams whose terms do not fit the kernel's LDS array (only for cap > that array)
    double *kf_stats = nullptr;
    unsigned long long *kf_terms = nullptr;
    // slam_kpset_select: the streams the six key-frame seams act on (detect, detect_describe, keyframe, stereo_match, triangulate,
    // triangulate_temporal; every other seam acts on all streams).  n_sel == KPSEL_ALL: no selection, the seams launch what they launch
    // without one.  Otherwise sel_idx[0 .. n_sel) are the selected streams ascending and sel_mask[s] is 0 / 1 (both device, one block of
    // the set's allocation; sel_host is the host's copy of the mask), staged through a pinned ring of 8 slots with an event each (made by
    // the first call that sets a selection), like `par`.  Not members of KpsetView: that struct is a kernel-argument block.
    // sel_rank[s]: the rank of stream s among the selected ones (-1: unselected; kpset_select_rank) -- the member of a compact right batch that holds its
    // build, read by the record-less prologue of a compact stereo match; the same block, between the table and the mask.
    int n_sel = KPSEL_ALL;
    int *sel_idx = nullptr, *sel_rank = nullptr; uint8_t *sel_mask = nullptr;
    uint8_t sel_host[128] = {};
    char *sel_pin = nullptr;
    hipEvent_t sel_ev[8] = {};
    int sel_slot = 0;
};

// ---- plumbing (kpset.hip) --------------------------------------------------------------------------------------------------------------
// stage `n` doubles (<= S x KP_PAR) of per-stream parameters into the next ring slot; returns the device pointer
int kpset_stage_params(slam_ctx *ctx, slam_kpset *ks, const double *host, size_t n, const double **dev_out);
// `selected` (both): the caller is a key-frame seam and honours the set's selection -- only the selected streams' segments / lists; the caller has returned
// before when no stream is selected (kpset_none_selected)
// what a match hands the work list for the records: its prior mode, its staged parameters (device), whether its target batch is compact
struct KpMatchPrior { int prior; const double *par; bool compact; };
bool kpset_match_records();                                      // false under SLAMHIP_NO_MATCH_REC=1 (read once per process)
int kpset_build_worklist(slam_ctx *ctx, slam_kpset *ks, int H, int W, bool selected = false, const KpMatchPrior *match = nullptr);   // H <= 0: slot order (no image, or an order would not pay)
int kpset_compact(slam_ctx *ctx, slam_kpset *ks, int mode, const uint8_t *flags_dev, bool selected = false);
inline bool kpset_none_selected(const slam_kpset *ks) { return ks->n_sel == 0; }
// the stream dimension of a key-frame seam's launch, and the table its selected kernel form reads (nullptr: the unselected form)
inline int kpset_sel_streams(const slam_kpset *ks) { return kpset_select_streams(ks->S, ks->n_sel); }
inline const int *kpset_sel_table(const slam_kpset *ks) { return ks->n_sel == KPSEL_ALL ? nullptr : ks->sel_idx; }
// the number of keypoints a launch over the work list is sized for: the host's bound of the live slots where it has one, else S x cap
inline int kpset_grid_bound(const slam_kpset *ks, int n_bound) { const int nmax = ks->S * ks->v.cap; return n_bound > 0 && n_bound < nmax ? n_bound : nmax; }
// the same for a key-frame seam: the selected streams' share of the capacity (no selection: kpset_grid_bound's value)
inline int kpset_sel_grid_bound(const slam_kpset *ks, int n_bound) { return kpset_select_bound(ks->S, ks->v.cap, ks->n_sel, n_bound); }
// the tail of a seam that returns results: `bytes` from `dev` to h + at (a region of the caller's Layout in its pinned block), one wait, then on into `out` (skipped where null)
struct KpReadBack { size_t at; const void *dev; size_t bytes; void *out; };
int kpset_read_back(slam_ctx *ctx, char *h, std::initializer_list<KpReadBack> parts);
