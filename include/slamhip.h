/*
 * slamhip.h -- C ABI of libslamhip.so: the MI355X (gfx950) implementation of
 * SLAM.jl's data-parallel hot path (extractor -> LK pyramid -> forward-backward
 * Lucas-Kanade -> local bundle adjustment).
 *
 * The reference (pxl-th/SLAM.jl) is pure Julia and has no FFI: the boundary is a
 * set of Julia function seams.  Each entry point below replaces one seam; the
 * Julia-side `ccall` shim that rebinds the seams is slam.jl_amd/julia/SLAMHip.jl
 * (see INTEGRATION.md).  Reference file:line cited per function are relative to
 * the reference repository root.
 *
 * Conventions (identical to the reference so the shim is copy-free):
 *   - Float64 everywhere; images are column-major H x W (Julia `Matrix`, y
 *     fastest), values in [0,1];
 *   - points are (y, x) Float64 pairs, 1-based pixel coordinates; keypoint
 *     indices are (row, col) Int64 pairs, 1-based; ids are Int64, 1-based;
 *   - the caller owns every host buffer; the library copies in/out before
 *     returning and never retains host pointers.  Pointers named `*_dev` are
 *     device (HBM) pointers owned by the caller;
 *   - every call returns 0 on success, a negative slam_status on failure;
 *     slam_last_error(ctx) gives the message.  No C++ exception crosses the ABI;
 *   - one slam_ctx per calling task/thread (it owns a HIP stream and scratch);
 *     calls on one ctx are synchronous unless the name ends in `_async` or the
 *     call has a `sync` argument / is documented as enqueue-only;
 *     pyramid handles may be READ by several contexts concurrently.  A pyramid (or
 *     a pyramid batch: its members share checkpoint scratch, the blur scratch
 *     plane and the cached hipGraph of the build) is BUILT through one stream at a
 *     time: enqueue its updates from one context, or order the contexts with
 *     slam_ctx_wait_for / slam_event_* before switching -- concurrent builds of
 *     one pyramid or of two members of one batch race on that scratch.
 */
#ifndef SLAMHIP_H
#define SLAMHIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slam_ctx slam_ctx;
typedef struct slam_pyr slam_pyr;   /* device-resident LKPyramid */
typedef struct slam_ba  slam_ba;    /* device-resident sharded-BA state */

enum slam_status {
    SLAM_OK = 0,
    SLAM_ERR_ARG = -1,          /* bad argument */
    SLAM_ERR_HIP = -2,          /* HIP runtime error (message has hipGetErrorString) */
    SLAM_ERR_LAYERS = -3,       /* "Not enough layers in pyramids." lucas_kanade.jl:15 */
    SLAM_ERR_CAPACITY = -4,     /* output buffer too small */
    SLAM_ERR_NUMERIC = -5,      /* reduced camera system not positive definite */
    /* per-window code of slam_local_ba_batch_dev, not an error of the call: the window is none the one-workgroup kernel takes; its arrays are
     * untouched (solve it through slam_local_ba_batch) */
    SLAM_BA_DEV_INELIGIBLE = 4
};

/* ---- context --------------------------------------------------------------- */
int  slam_ctx_create(int device, slam_ctx **out);
/* the same, with the context's stream restricted to the compute units set in cu_mask (bit i of word i / 32 = CU i):
 * partitions the chip between stages that run concurrently on different contexts */
int  slam_ctx_create_cumask(int device, const uint32_t *cu_mask, int n_words, slam_ctx **out);
/* the same, with the stream in its own scheduling class (priority > 0 high, < 0 low): its own hardware queue, which a
 * replayed hipGraph's branches never share -- for the latency-critical stage of a multi-context pipeline */
int  slam_ctx_create_priority(int device, int priority, slam_ctx **out);
/* waits for the context's stream, frees its scratch; the STREAM itself is parked for the next context of the same device and scheduling
 * class instead of being destroyed -- events another library recorded on it (PyTorch's pinned-memory allocator does, for copies issued on
 * the stream) stay valid for the life of the process */
int  slam_ctx_destroy(slam_ctx *ctx);
int  slam_ctx_synchronize(slam_ctx *ctx);
/* Device-side ordering between two contexts of one device: work enqueued on `ctx`
 * after this call waits for everything enqueued on `other` so far (no host block).
 * Lets a caller overlap asynchronous calls on two contexts the way the reference
 * overlaps its front-end and mapper tasks (SLAM.jl:166, mapper.jl:37-66), e.g.
 * slam_pyr_update_dev(other, next frame, sync=0) while `ctx` tracks the current one. */
int  slam_ctx_wait_for(slam_ctx *ctx, slam_ctx *other);
/* Markers for deeper pipelines: slam_event_record(ctx, e) marks what `ctx` has enqueued so far; slam_ctx_wait_event(ctx2, e)
 * makes later work of ctx2 wait (on the device) for that point, even after more work has been enqueued on `ctx`
 * (e.g. the pyramid builds of frames t+1 and t+2 are both in flight while tracking waits for t+1 only). */
typedef struct slam_event slam_event;
int  slam_event_create(slam_ctx *ctx, slam_event **out);
int  slam_event_record(slam_ctx *ctx, slam_event *e);
int  slam_ctx_wait_event(slam_ctx *ctx, slam_event *e);
int  slam_event_destroy(slam_event *e);
/* the same with timing enabled: a pair brackets a stage on a context's stream; slam_event_elapsed_ms waits for `b` */
int  slam_event_create_timed(slam_ctx *ctx, slam_event **out);
int  slam_event_elapsed_ms(slam_event *a, slam_event *b, double *ms);
/* the ctx's hipStream_t (as void*), for callers that record HIP events on it */
void *slam_ctx_stream(slam_ctx *ctx);
/* message of the last failing call on ctx (ctx == NULL: last ctx-less failure) */
const char *slam_last_error(slam_ctx *ctx);
/* library version / build arch string, e.g. "slamhip 0.1 gfx950" */
const char *slam_version(void);
/* Optional device-side timing: when enabled, named spans (e.g. "pyr_update",
 * "k_iir_rows", "fb_track", "detect", "local_ba") are bracketed with hipEvents
 * on the ctx stream; slam_prof_get synchronises and returns the accumulated
 * device time and span count.  The reference's equivalent is its @debug
 * time() prints (front_end.jl:82-114, mapper.jl:50-132, estimator.jl:90-106). */
int  slam_prof_enable(slam_ctx *ctx, int on);
int  slam_prof_reset(slam_ctx *ctx);
int  slam_prof_get(slam_ctx *ctx, const char *name, double *total_ms, int64_t *count);

/* ---- Extractor -------------------------------------------------------------- */
/* detect(e::Extractor, image, current_points; sigma_mask) -- src/extractor.jl:63-95
 * (+ get_mask :116-122, _shi_tomasi :24-42).  Extractor fields (extractor.jl:7-20,
 * built at SLAM.jl:149-160) are passed explicitly.  out_rc receives (row, col)
 * pairs in the reference's order (cells row-major, column-major inside a cell);
 * cap = capacity in keypoints; n_out may exceed max_points (as in the reference).
 * Returns n_out = 0 when n_cur >= max_points (extractor.jl:64). */
int slam_detect(slam_ctx *ctx, const double *image, int H, int W,
                const double *cur_yx, int n_cur,
                int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                double sigma_mask, double min_response,
                int64_t *out_rc, int cap, int *n_out);
/* Same, on the image already resident as layer 1 of a device pyramid (the frame
 * passed to create_keyframe! is the one the current pyramid was built from:
 * front_end.jl:461-464, map_manager.jl:98-105).  No image upload. */
int slam_detect_pyr(slam_ctx *ctx, const slam_pyr *pyr,
                    const double *cur_yx, int n_cur,
                    int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                    double sigma_mask, double min_response,
                    int64_t *out_rc, int cap, int *n_out);
/* detect() for the S members of a pyramid batch (slam_pyr_create_batch) in one launch:
 * cur_yx holds the current keypoints of all streams back to back, stream s owning
 * [cur_off[s], cur_off[s+1]) (cur_off[0] = 0); the new keypoints of stream s are
 * out_rc[out_off[s] .. out_off[s+1]).  cap = total capacity in keypoints.  Per stream
 * identical to slam_detect_pyr on that stream's pyramid (map_manager.jl:105 called for S
 * independent streams). */
int slam_detect_batch(slam_ctx *ctx, const slam_pyr *pyr0, int S,
                      const double *cur_yx, const int32_t *cur_off,
                      int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                      double sigma_mask, double min_response,
                      int64_t *out_rc, int cap, int32_t *out_off);

/* describe(e, image, keypoints) -> create_descriptor(img, kps, BRIEF) --
 * src/extractor.jl:103-105.  pattern: n_bits x 4 int32 (dy1, dx1, dy2, dx2)
 * sampling table supplied by the caller (ImageFeatures draws it from Julia's
 * seeded RNG, which cannot be reproduced outside Julia).  n_bits % 64 == 0.
 * out_bits: n x (n_bits/64) uint64; out_rc: surviving keypoints (border-dropped
 * ones removed, order kept). */
int slam_describe(slam_ctx *ctx, const double *image, int H, int W,
                  const int64_t *rc, int n, const int32_t *pattern, int n_bits,
                  double sigma, int window,
                  uint64_t *out_bits, int64_t *out_rc, int *n_out);
/* describe() (src/extractor.jl:103-105, called at map_manager.jl:106) on the image resident as layer 0 of a device pyramid; no image
 * upload.  Results identical to slam_describe on the image the pyramid was built from.  Odd window <= 15 (the neighbourhood of a
 * keypoint is smoothed in LDS: csrc/brief.hip, k_brief_patch); a larger window is SLAM_ERR_ARG. */
int slam_describe_pyr(slam_ctx *ctx, const slam_pyr *pyr, const int64_t *rc, int n,
                      const int32_t *pattern, int n_bits, double sigma, int window,
                      uint64_t *out_bits, int64_t *out_rc, int *n_out);
/* describe() for the first S members of a pyramid batch in one launch (map_manager.jl:106 called for S streams): stream s owns
 * rc[off[s] .. off[s+1]) and out_bits / out_rc[out_off[s] .. out_off[s+1]) (as slam_detect_batch; off and out_off hold S + 1 entries).
 * The caller's out_bits / out_rc hold off[S] keypoints. */
int slam_describe_batch(slam_ctx *ctx, const slam_pyr *pyr0, int S, const int64_t *rc, const int32_t *off,
                        const int32_t *pattern, int n_bits, double sigma, int window,
                        uint64_t *out_bits, int64_t *out_rc, int32_t *out_off);

/* ---- LKPyramid -------------------------------------------------------------- */
/* LKPyramid(image, levels; sigma, reusable=true) / update!(lk, img) / copy! /
 * deepcopy -- src/optical_flow/pyramid.jl:16-137, lucas_kanade.jl:102-138.
 * pyramid_levels = levels above the base (Params.pyramid_levels = 3 -> 4 layers). */
int slam_pyr_create(slam_ctx *ctx, int H, int W, int pyramid_levels, slam_pyr **out);
int slam_pyr_destroy(slam_pyr *pyr);
/* Update mode flag (OR it into `mode` = 1 or 3): the pyramid will only be the TARGET of matches -- the mapper's right pyramid
 * (mapper.jl:51-56, optical_flow_matching!(..., left, right, true)).  optflow! samples a target's layers at every level and
 * fb_tracking!'s backward pass (pyramid_levels = 0, tracker.jl:51-57) uses it as template at level 1 only, so the gradient,
 * product and integral planes of the coarser levels are never read: level 0 is built in full, the other levels get their layers
 * only (about a quarter of the build).  Passing such a pyramid as the SOURCE of a match is an error (SLAM_ERR_ARG). */
#define SLAM_PYR_TARGET_ONLY 16
/* Update mode flag: replay the build as ONE chain on the calling context's stream (no forked integral-image branch).  One build
 * alone takes ~15 % longer (441 vs 376 us for a 370 x 1226 image), but it occupies one hardware queue instead of two and costs the
 * host a third per call (31 vs 84 us): the choice for a host that keeps the builds of several consecutive frames in flight on several
 * contexts (preprocess! of frames t+1 .. t+3 while frame t is tracked: 170 us per build with three in flight). */
#define SLAM_PYR_CHAIN 32
/* mode 0: constructor semantics (pyramid.jl:40-79: NA() blur, Fill(0) Scharr);
 * mode 1: update! semantics (pyramid.jl:81-137: replicate borders);
 * mode 3: update! semantics with SEGMENTED recurrences: each IIR / cumulative-sum
 *         line is cut into <= 16 segments whose entry states are obtained from
 *         zero-state end states and powers of the filter's companion matrix.  Same
 *         arithmetic inside a segment, different rounding of the entry states:
 *         planes agree with mode 1 to ~1e-13 relative (mode 1 is bit-exact against
 *         the sequential reference order and is what the parity tests pin). */
int slam_pyr_update(slam_ctx *ctx, slam_pyr *pyr, const double *image, int mode, double sigma);
/* image already in HBM (column-major f64); returns after enqueueing when sync == 0 */
int slam_pyr_update_dev(slam_ctx *ctx, slam_pyr *pyr, const double *image_dev, int mode, double sigma, int sync);
/* Same, from the 8-bit image the KITTI reader decodes (example/kitty/kitty.jl:52-102) before
 * `Gray{Float64}.(frame)` (example/kitty/main.jl:39-41): the conversion raw/255 runs on the device,
 * so the host link carries 1 byte per pixel instead of 8. */
int slam_pyr_update_u8(slam_ctx *ctx, slam_pyr *pyr, const uint8_t *image_u8, int mode, double sigma);
/* the same from an 8-bit image already resident in HBM; returns after enqueueing when sync == 0 */
int slam_pyr_update_u8_dev(slam_ctx *ctx, slam_pyr *pyr, const uint8_t *image_u8_dev, int mode, double sigma, int sync);
/* copy!(dst, src) pyramid.jl:28-38 (same shape required) */
int slam_pyr_copy(slam_ctx *ctx, slam_pyr *dst, const slam_pyr *src);
/* deepcopy(lk) SLAM.jl:218 */
int slam_pyr_clone(slam_ctx *ctx, const slam_pyr *src, slam_pyr **out);
/* introspection for parity tests: plane 0..5 = layers, Iy, Ix, Iyy, Ixx, Iyx;
 * level 0-based.  out must hold H_l * W_l doubles. */
int slam_pyr_shape(const slam_pyr *pyr, int level, int *H, int *W);
int slam_pyr_levels(const slam_pyr *pyr);
int slam_pyr_download(slam_ctx *ctx, const slam_pyr *pyr, int plane, int level, double *out);

/* ---- forward-backward Lucas-Kanade ----------------------------------------- */
/* fb_tracking!(prev, cur, keypoints; displacement, iterations, window_size,
 * pyramid_levels, max_distance) -- src/tracker.jl:17-82 over optflow!
 * src/optical_flow/lucas_kanade.jl:9-100.  disp0_yx may be NULL (zeros);
 * it is given in coarsest-level pixels like the reference's `displacement`.
 * out_yx[i] is defined only where status[i] != 0.  n == 0 is a no-op. */
int slam_fb_track(slam_ctx *ctx, const slam_pyr *prev, const slam_pyr *cur,
                  const double *pts_yx, const double *disp0_yx, int n,
                  int pyramid_levels, int window, int iterations,
                  double eig_thr, double eps, double max_distance,
                  double *out_yx, uint8_t *status);

/* The array-level body of optical_flow_matching!(map_manager, frame, from, to, stereo)
 * -- src/map_manager.jl:451-564 -- in one call: keypoints flagged is_3d are first
 * tracked with the prior displacement (proj - pt) / 2^pyramid_levels_3d on
 * pyramid_levels_3d levels (:494,504,517-521); the ones that fail join the 2-D
 * keypoints and are tracked without prior on pyramid_levels levels (:533-552).
 * Results are identical to issuing the two slam_fb_track calls of the reference
 * protocol (points are independent).  proj_yx is read only where is_3d != 0. */
int slam_flow_match(slam_ctx *ctx, const slam_pyr *from, const slam_pyr *to,
                    const double *pts_yx, const uint8_t *is_3d, const double *proj_yx, int n,
                    int pyramid_levels, int pyramid_levels_3d, int window, int iterations,
                    double eig_thr, double eps, double max_distance,
                    double *out_yx, uint8_t *status);

/* ---- lock-stepped batches of streams --------------------------------------- */
/* The recurrences of the pyramid build are latency-bound for one image; S independent images
 * (left + right of a key-frame, or S camera streams) share every launch when their pyramids live in one batch.
 * slam_pyr_create_batch fills out[0..S) (1 <= S <= 128) with ordinary pyramid handles backed by one allocation; each can be used
 * with every single-pyramid call above.  slam_pyr_update_batch_dev rebuilds all S in one launch set (pyrs must
 * be the S members of one batch, in order; images already in HBM); slam_flow_match_batch tracks the keypoints
 * of all S streams in one launch (img_index[i] = stream of point i; from0 / to0 = member 0 of two batches).
 * Batch updates: mode 1 or 3 as for slam_pyr_update.
 *   mode 1 -- every plane bit-identical to mode 1 on a single pyramid (the parity reference and the default); launches with >= 40 MB
 *     of plane data use the checkpointed IIR kernels (forward state every 32 samples, forward values recomputed: 2 reads + 1 write
 *     per sample instead of 2 + 2) and the fused dim-1 stage, still bit-identical.
 *   mode 3 with S >= 4 (round 4) -- the TOLERANCE-mode batch build: per level one dim-1 kernel that leaves the product planes as
 *     suffix sums along y and one dim-2 kernel that finishes filter, running sum and imresize! with one read and one write per plane
 *     (2.2x instead of 3.9x the algorithmic bytes).  Every plane within 1e-11 of the mode-1 plane relative to the
 *     plane's largest magnitude; tracked positions within 1e-6 px.  Keypoint INDICES are not affected: slam_detect* work on the raw
 *     frame / the base layer, which is the same bytes in both modes.  Levels too small for those kernels (and S < 4: the segmented
 *     single-image kernels of slam_pyr_update's mode 3) fall back per level; a batch may be updated in either mode at any time.
 *     NOTE: in this mode the ARITHMETIC is no longer the reference's operation sequence -- the dim-2 kernel contracts its multiply-adds
 *     into FMAs and evaluates the recurrences through affine maps of row segments, the dim-1 kernel leaves suffix sums instead of
 *     filtered values -- only the RESULT is held to the reference's (1e-11 relative).  Matches between two pyramids last built in
 *     mode 3 (slam_kpset_flow_match / _stereo_match) likewise take a tracking kernel with contracted arithmetic (two-operation
 *     lerps, FMA accumulation; positions within 1e-6 px of the sequential-order oracle, csrc/lk.hip TOL). */
int slam_pyr_create_batch(slam_ctx *ctx, int H, int W, int pyramid_levels, int S, slam_pyr **out);
int slam_pyr_update_batch_dev(slam_ctx *ctx, slam_pyr *const *pyrs, const double *const *images_dev, int S,
                              int mode, double sigma, int sync);
/* Same from 8-bit frames resident in HBM (column-major H x W bytes, the KITTI reader's decode before
 * `Gray{Float64}.(frame)`, example/kitty/main.jl:39-41): raw / 255 on the device. */
int slam_pyr_update_batch_u8_dev(slam_ctx *ctx, slam_pyr *const *pyrs, const uint8_t *const *images_u8_dev, int S,
                                 int mode, double sigma, int sync);
/* COMPACT batch builds: a key-frame is a per-stream event (slam_kpset_select), and a member's planes depend on that member's image alone, so
 * the right frames of the streams that take a key-frame are built into the FIRST n_sel members of the right batch and nothing else is.
 *   pyrs       the n_members members of ONE slam_pyr_create_batch call, in order.  n_members may be smaller than S: a right batch of K
 *              members holds K x 7 planes, not S x 7.
 *   images     S device pointers indexed by STREAM (Float64 images, or 8-bit frames for _u8).  The pointers of unselected streams are never
 *              read and may be NULL; a selected stream's pointer must not be.
 *   selected   S bytes on the host, non-zero = selected (required[] of slam_keyframe_required passes as it is), or NULL = every stream.
 *   *n_built   receives n_sel, the number of selected streams.
 * MEMBER ORDER: member r receives the build of the r-th selected stream, ascending by stream index -- bit for bit (mode 1) what member s of
 * an ordinary S-member build of the same frames holds, by the kernels, routes, chunking and graph of an n_sel-member build.  Members at
 * index n_sel or above KEEP THEIR BYTES (planes, target_only / tolerance marks); n_sel == 0 enqueues nothing.  n_sel > n_members:
 * SLAM_ERR_ARG, nothing enqueued, nothing changed.  mode, sigma, sync as for slam_pyr_update_batch_dev.
 * STALE-BUILD RULE: the batch remembers, on the host, the mask it was last built for; these two calls set that record, an ordinary
 * slam_pyr_update_batch_* clears it.  slam_kpset_stereo_match_compact (below) refuses a batch whose record is not the set's current
 * selection -- the one guard against matching into another key-frame's pyramids.  A build of a member count not seen before constructs its
 * launch graph on first use (one executable per distinct count and mode, kept for the batch's lifetime). */
int slam_pyr_update_batch_sel_dev(slam_ctx *ctx, slam_pyr *const *pyrs, int n_members, const double *const *images_dev, int S,
                                  const uint8_t *selected, int mode, double sigma, int sync, int *n_built);
int slam_pyr_update_batch_sel_u8_dev(slam_ctx *ctx, slam_pyr *const *pyrs, int n_members, const uint8_t *const *images_u8_dev, int S,
                                     const uint8_t *selected, int mode, double sigma, int sync, int *n_built);
int slam_flow_match_batch(slam_ctx *ctx, const slam_pyr *from0, const slam_pyr *to0, int S, const int32_t *img_index,
                          const double *pts_yx, const uint8_t *is_3d, const double *proj_yx, int n,
                          int pyramid_levels, int pyramid_levels_3d, int window, int iterations,
                          double eig_thr, double eps, double max_distance, double *out_yx, uint8_t *status);
/* slam_flow_match_batch followed by the list surgery of optical_flow_matching! (map_manager.jl:523-560): the keypoints
 * whose tracking succeeded, in input order, with their new positions (kept_yx), 3-D flags, stream indices and input
 * indices (kept_src); arrays sized for n entries.  status (n, nullable) reports every input keypoint. */
int slam_flow_match_batch_kept(slam_ctx *ctx, const slam_pyr *from0, const slam_pyr *to0, int S, const int32_t *img_index,
                               const double *pts_yx, const uint8_t *is_3d, const double *proj_yx, int n,
                               int pyramid_levels, int pyramid_levels_3d, int window, int iterations,
                               double eig_thr, double eps, double max_distance,
                               double *kept_yx, uint8_t *kept_is3d, int32_t *kept_img, int32_t *kept_src, int *n_kept,
                               uint8_t *status);

/* ---- device-resident keypoint lists --------------------------------------------------------------
 * The reference keeps a frame's keypoints in a Dict and optical_flow_matching! (map_manager.jl:451-564) copies them into
 * arrays per call; here the lists of S lock-stepped streams live in HBM: stream s owns slots [s cap, s cap + count[s]) of
 * every per-keypoint array (pixel, is_3d, map point, id, stereo pixel / flag).  Tracking, removal of lost keypoints, map
 * culling, the avoidance list and merge of key-frame detection, stereo matching and triangulation read and write those
 * arrays; compaction is stable and runs on the device (wave ballot + prefix counts).  Every call except create / upload /
 * download / counts returns after ENQUEUEING on ctx's stream; slam_kpset_counts is the one small device -> host copy a step
 * needs.  n_bound: an upper bound of the number of live keypoints known to the host (sizes launches; <= 0: S x cap).
 * Per-stream call parameters `params`: S x 32 doubles, [0..15] Tcw of the target camera (column-major 4x4), [16..19] fx fy cx
 * cy and [20..23] k1 k2 p1 p2 of the target camera, [24..25] prior shift (y, x); prior = 0: none, 1: projection of the map
 * point through Tcw and the lens model (project_world_to_image_distort, frame.jl:478-484), 2: pixel + shift.
 * THE SELECTION (slam_kpset_select): a key-frame is a per-stream event (check_new_kf_required, slam_keyframe_required below), so the SIX
 * KEY-FRAME SEAMS -- slam_kpset_detect, _detect_describe, _keyframe, _stereo_match, _triangulate, _triangulate_temporal -- act on the
 * selected streams only.  EVERY OTHER SEAM IGNORES THE SELECTION and acts on all S streams: slam_kpset_flow_match, _remove,
 * _compute_pose, _compute_pose_5pt, _frame_stats, _counts and the uploads / downloads (slam_frontend_step owns a set of one stream and
 * never selects).  An unselected stream comes out of the six seams as it went in -- every per-keypoint array, its list length, its
 * key-frame counter and its id counter byte for byte -- and none of the per-stream inputs a seam takes for it (params row, Twc, tab,
 * kf_cur, kf_lo) has any effect; a selected stream's result does not depend on which other streams are selected.  Launches are sized
 * by the number of selected streams; with none selected the six seams check their arguments and enqueue nothing.
 * slam_kfmap_add_keyframe (the key-frame map, below) reads the lists of a key-frame and honours the selection like the six: an unselected
 * stream's map comes out byte for byte as it went in. */
typedef struct slam_kpset slam_kpset;
int slam_kpset_create(slam_ctx *ctx, int S, int cap, slam_kpset **out);
int slam_kpset_destroy(slam_kpset *ks);
int slam_kpset_streams(const slam_kpset *ks);
int slam_kpset_capacity(const slam_kpset *ks);
/* Set the streams the six key-frame seams act on: selected = S bytes on the host, non-zero = selected (required[] of
 * slam_keyframe_required can be passed as it is), or NULL = every stream (the state of a new set; a mask that selects every stream is the
 * same thing).  The selection is a property of the set and holds until the next call.  Enqueue-only on ctx's stream: the bytes are staged,
 * the caller's array is free on return.  The table the kernels read is written in ctx's stream order, so a host that drives one set from
 * several contexts orders slam_kpset_select against the seams exactly as it orders the seams against each other today (events /
 * slam_ctx_synchronize between contexts): a key-frame seam enqueued on another context must not run before the select it relies on has,
 * nor may the next select run while it still does.  slam_kpset_selection: the current selection as S bytes of 0 / 1 (all 1 when none is set). */
int slam_kpset_select(slam_ctx *ctx, slam_kpset *ks, const uint8_t *selected /* S bytes, host; NULL = every stream */);
int slam_kpset_selection(const slam_kpset *ks, uint8_t *selected_out /* S bytes */);
/* replace / read stream s's list (initialisation, tests, host consumers); NULL arrays are skipped; ids == NULL: 0 .. n-1 */
int slam_kpset_upload(slam_ctx *ctx, slam_kpset *ks, int s, const double *yx, const uint8_t *is_3d, const double *xyz,
                      const int64_t *ids, int n);
int slam_kpset_download(slam_ctx *ctx, slam_kpset *ks, int s, double *yx, uint8_t *is_3d, double *xyz, int64_t *ids,
                        double *stereo_yx, uint8_t *has_stereo, int cap_out, int *n_out);
int slam_kpset_counts(slam_ctx *ctx, slam_kpset *ks, int32_t *counts /* S */);
/* optical_flow_matching!(map_manager, frame, from, to, false): 3-D keypoints first with their prior on pyramid_levels_3d
 * levels, failures and 2-D keypoints without prior on pyramid_levels levels (map_manager.jl:517-552); 3-D keypoints whose
 * projection is outside the image are left as they are (:501-506); lost keypoints are removed (:559), the others take
 * their new position.  from0 / to0: member 0 of two pyramid batches with >= S members. */
int slam_kpset_flow_match(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *from0, const slam_pyr *to0, const double *params, int prior,
                          int pyramid_levels, int pyramid_levels_3d, int window, int iterations, double eig_thr, double eps,
                          double max_distance, int n_bound);
/* optical_flow_matching!(..., true) left0 -> right0 (params: the RIGHT camera): a match passes maybe_stereo_update!
 * (map_manager.jl:579-590: |left row - undistorted right row| <= epipolar_error; the left row is kept) and is stored as the
 * keypoint's stereo pixel; 3-D keypoints projected outside the right image are removed (:491-498).  The left camera is taken as
 * rectified (its undistorted row = the pixel row). */
int slam_kpset_stereo_match(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *left0, const slam_pyr *right0, const double *params, int prior,
                            int pyramid_levels, int pyramid_levels_3d, int window, int iterations, double eig_thr, double eps,
                            double max_distance, double epipolar_error, int n_bound);
/* The same into a COMPACT right batch (slam_pyr_update_batch_sel_*): right0 is member 0 of a batch whose member r holds the build of the
 * r-th selected stream, and stream s's target is read at member rank(s).  left0's batch still needs >= S members (a stream's source is
 * member s), right0's >= n_sel.  STALE-BUILD RULE: the mask the right batch was last built for must equal the set's current selection,
 * stream for stream; a batch built for another selection, or by an ordinary slam_pyr_update_batch_* since, gives SLAM_ERR_ARG (the message
 * names the stale build) and the lists are not touched.  Per selected stream the result is byte for byte that of slam_kpset_stereo_match
 * into a whole-batch build of the same frames; unselected streams come out as they went in.  With no selection set the call IS
 * slam_kpset_stereo_match (same kernels, same arguments; right0's batch then needs >= S members and no compact build of fewer streams). */
int slam_kpset_stereo_match_compact(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *left0, const slam_pyr *right0, const double *params,
                                    int prior, int pyramid_levels, int pyramid_levels_3d, int window, int iterations, double eig_thr, double eps,
                                    double max_distance, double epipolar_error, int n_bound);
/* remove the keypoints whose flag is set (flags_dev: S x cap bytes in HBM, slot order): map culling, outliers of the pose
 * estimators (estimator.jl:283-292, front_end.jl:174-219) */
int slam_kpset_remove(slam_ctx *ctx, slam_kpset *ks, const uint8_t *flags_dev);
/* extract_keypoints! (map_manager.jl:98-113) for every stream: detect() with the stream's own list as avoidance list; the
 * new keypoints are appended (is_3d = 0, fresh ids).  Needs cap >= max_points + grid_rows x grid_cols. */
int slam_kpset_detect(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *pyr0, int max_points, int radius, int grid_rows, int grid_cols,
                      int cell_size, double sigma_mask, double min_response);
/* extract_keypoints! WITH describe (map_manager.jl:98-113: keypoints = detect(...); descriptors, keypoints = describe(...);
 * add_keypoints_to_frame!) on the lists: detect, drop the candidates whose +-lim box (lim = (window + 1) / 2) leaves the image,
 * append the survivors (is_3d = 0, fresh consecutive ids), describe them.  desc_dev: S x dcap x (n_bits / 64) words in HBM; the j-th
 * keypoint appended to stream s by THIS call has id info_dev[2 s] + j and its descriptor at desc_dev[(s dcap + j) words ..];
 * info_dev[2 s + 1] = number appended (info_dev: S x 2 int64 in HBM).  Descriptors belong to the map point of that id
 * (map_manager.jl:116-131) and are not carried through compactions.  Enqueue-only, like slam_kpset_detect.
 * dcap >= grid_rows grid_cols ceil(max_points / (grid_rows grid_cols)); window as slam_describe_pyr.
 * An unselected stream s (slam_kpset_select): info_dev[2 s] = its id counter, info_dev[2 s + 1] = 0, its desc_dev rows are not written. */
int slam_kpset_detect_describe(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *pyr0, int max_points, int radius,
                               int grid_rows, int grid_cols, int cell_size, double sigma_mask, double min_response,
                               const int32_t *pattern, int n_bits, double sigma, int window,
                               uint64_t *desc_dev, int64_t *info_dev, int dcap);
/* triangulate_stereo! (mapper.jl:142-183) for every 2-D keypoint with a stereo match: success -> map point Twc[s] X and
 * is_3d = 1, failure -> the stereo observation is dropped.  P1, P2, T21, cam1, cam2 as slam_triangulate; Twc: S x 16.
 * The left and right pixels are used as stored: this form is for RECTIFIED, zero-distortion pairs (KITTI, the reference's
 * stereo example), where kp.undistorted_pixel == kp.pixel (mapper.jl:162-163); for cameras with lens distortion use
 * slam_kpset_triangulate_lens below. */
int slam_kpset_triangulate(slam_ctx *ctx, slam_kpset *ks, const double *P1, const double *P2, const double *T21,
                           const double *cam1, const double *cam2, const double *Twc, double max_error, double min_depth, int n_bound);
/* The same for a rig with lenses (dist1, dist2: k1 k2 p1 p2 of camera 1 / camera 2): the left pixel goes through
 * undistort_point(cam1, dist1, .), the stored stereo pixel through undistort_point(cam2, dist2, .), and the DLT and both reprojection
 * gates work on the undistorted pair (kp.undistorted_pixel / kp.right_undistorted_pixel, mapper.jl:162-177, frame.jl:272-281).  The
 * lists keep the raw pixels.  Selection, enqueue-only contract and every other argument as slam_kpset_triangulate; a camera whose four
 * coefficients are zero has its pixel used as stored, so with both zero the lists come out byte for byte as from that call. */
int slam_kpset_triangulate_lens(slam_ctx *ctx, slam_kpset *ks, const double *P1, const double *P2, const double *T21,
                                const double *cam1, const double *cam2, const double *dist1 /* 4 */, const double *dist2 /* 4 */,
                                const double *Twc, double max_error, double min_depth, int n_bound);

/* compute_pose! (front_end.jl:132-219) for every stream, on the set: the is_3d keypoints in list order (:139-160; undistorted
 * pixel and normalised bearing from params[s][16..23] = fx fy cx cy k1 k2 p1 p2) -> P3P RANSAC (threshold = max_reprojection_error,
 * `iters` triples per stream from a counter-based generator seeded with `seed`: three distinct indices,
 * splitmix64(seed ^ s << 48 ^ iteration << 16 ^ attempt) mod n, restated in keypoint_set.py) -> its outliers leave the list
 * (:187-189) -> pnp_bundle_adjustment of the inliers from the P3P pose (:203-206) -> its outliers leave the list (:213-215).
 * status[s] = 1: poses_cw[16 s ..] is the refined world -> camera transform (column-major 4 x 4); 0: one of the reference's
 * reset exits (fewer than 5 3-D keypoints :133, fewer than 5 P3P inliers :179, refinement left fewer than 5 inliers or a larger
 * error :207; in the last case the P3P outliers are already gone, as in the reference), pose = identity.  n_inliers (P3P) and
 * counts (list lengths after the removals) may be NULL.  Synchronous: the call is the step's one device -> host copy. */
int slam_kpset_compute_pose(slam_ctx *ctx, slam_kpset *ks, const double *params, double threshold, int iters, uint64_t seed,
                            int pnp_iters_fast, int pnp_iterations, double depth_eps, double repr_eps,
                            double *poses_cw, int32_t *status, int32_t *n_inliers, int32_t *counts);

/* create_keyframe! (map_manager.jl:60-96) for the lists: the current frame becomes the previous key-frame of every keypoint it
 * holds (call it after slam_kpset_detect: the key-frame contains the new keypoints).  The observation travels with the keypoint
 * through every compaction; keypoints detected later have none until the next call. */
int slam_kpset_keyframe(slam_ctx *ctx, slam_kpset *ks);
/* triangulate_temporal! (mapper.jl:185-262) for every 2-D keypoint whose first observer -- the key-frame that detected it; the set
 * keeps that observation and the key-frame's id (a per-stream counter advanced by slam_kpset_keyframe) beside the keypoint -- is an
 * earlier key-frame than the frame's (kf_cur[s]) and still in the table (>= kf_lo[s]).  tab: S x nkf x 64 doubles, entry
 * [s][kf % nkf] = { P2 = K * rel_pose_inv, rel_pose_inv, rel_pose = observer.cw * frame.wc, observer.wc }, column-major 4 x 4 each
 * (what mapper.jl:226-231 computes once per observer).  Success: map point = observer.wc * X, is_3d = 1; a gate fails with the
 * rotation-compensated parallax above min_parallax: the observation is removed (:244-258); otherwise the point is accepted. */
int slam_kpset_triangulate_temporal(slam_ctx *ctx, slam_kpset *ks, const double *params, const double *tab, int nkf,
                                    const int32_t *kf_cur, const int32_t *kf_lo, double max_error, double min_depth, double min_parallax,
                                    int n_bound);
/* the first observations of stream s's list, host <-> device (restoring state, tests): first_yx n x 2, first_kf n ids, and the
 * stream's key-frame counter */
int slam_kpset_upload_first(slam_ctx *ctx, slam_kpset *ks, int s, const double *first_yx, const int32_t *first_kf, int n, int kf_count);
int slam_kpset_download_first(slam_ctx *ctx, slam_kpset *ks, int s, double *first_yx, int32_t *first_kf, int cap_out, int *n_out, int *kf_count);
/* the key-frame observations of stream s's list, host <-> device (restoring state, tests): kyx n x 2 (y, x), has_kf n flags */
int slam_kpset_upload_keyframe(slam_ctx *ctx, slam_kpset *ks, int s, const double *kyx, const uint8_t *has_kf, int n);
int slam_kpset_download_keyframe(slam_ctx *ctx, slam_kpset *ks, int s, double *kyx, uint8_t *has_kf, int cap_out, int *n_out);
/* the stereo observations of stream s's list, host -> device (restoring state, tests; slam_kpset_download reads them back):
 * stereo_yx n x 2 (y, x) in the right image, has_stereo n flags */
int slam_kpset_upload_stereo(slam_ctx *ctx, slam_kpset *ks, int s, const double *stereo_yx, const uint8_t *has_stereo, int n);
/* compute_pose_5pt! (front_end.jl:242-332, run every frame at :105) for every stream, on the set: the keypoints the previous
 * key-frame also observes -> undistorted pixels and normalised coordinates of both views (:263-272), the rotation-compensated
 * average parallax (:277-281; params[s][0..8] = R_compensation, column-major; [16..23] camera and distortion) -> five-point
 * RANSAC (`iters` 5-tuples per stream from the generator of slam_kpset_compute_pose) -> its outliers leave the list (:310-318).
 * status[s] = 1: P[12 s ..] is [R | t] (column-major 3 x 4, key-frame -> frame, |t| = 1) of the best essential matrix; 0: one
 * of the `nothing` exits (fewer than 8 keypoints :243 / in the key-frame :283, parallax below min_parallax :290, fewer than 5
 * inliers :305), nothing removed.  The composition with the motion-model scale (:320-330) is the caller's.  n_inliers, parallax
 * (the average) and counts (list lengths after the removals) may be NULL.  Synchronous -- unless P and status are both NULL:
 * then the call only enqueues (the epipolar filter acts on the lists; compute_pose! right behind it brings the step's copy). */
int slam_kpset_compute_pose_5pt(slam_ctx *ctx, slam_kpset *ks, const double *params, double min_parallax, double max_repr_error,
                                int iters, uint64_t seed, double *P, int32_t *status, int32_t *n_inliers, double *parallax,
                                int32_t *counts);

/* What the front-end's key-frame tests read of a frame -- check_new_kf_required (front_end.jl:361-393, run at the end of every
 * track_mono!, :117) and check_ready_for_init! (:343-354) -- reduced from the lists, one workgroup per stream, SLAM_KF_STATS doubles
 * per stream (counts are held as doubles: one array, one copy):
 *   [0] list length   [1] nb_3d_kpts   [2] nb_stereo_kpts   [3] keypoints the previous key-frame observes
 *   [4] nb_occupied_cells (frame.jl:321-337): distinct cells (round(y) / cell_size + 1, round(x) / cell_size + 1) -- round to nearest even,
 *       truncating division (SLAM.jl:30,42-45) -- in the grid of ceil(height / cell_size) x ceil(width / cell_size) cells (frame.jl:130-132).
 *       A keypoint whose cell lies outside that grid (NaN and +-inf included) is NOT counted; the reference would throw at grid[kpi].
 *   [5] n_parallax   [6] mean parallax   [7] median parallax -- compute_parallax (front_end.jl:412-452) over the keypoints the previous
 *       key-frame observes (flags bit 1 = only_2d: the 2-D ones among them): |upx - undistort(key-frame pixel)| with upx = undistort(pixel),
 *       or, flags bit 0 = compensate_rotation, upx = project(camera, R_compensation * backproject(undistort(pixel))) -- then the mean is
 *       the average parallax of slam_kpset_compute_pose_5pt.  The median is Julia's: the middle order statistic, lo / 2 + hi / 2 of the
 *       two middle ones for an even number, NaN if any term is NaN -- exact for any list length (a radix select, no sort).  Both are
 *       0.0 when n_parallax == 0 (:444).
 * params: S x 32 as for slam_kpset_compute_pose_5pt ([0..8] R_compensation = Rcw(key-frame) Rwc(frame), dense column-major 3 x 3;
 * [16..23] fx fy cx cy k1 k2 p1 p2).  check_new_kf_required calls with flags = 1, check_ready_for_init! with flags = 2.
 * cell_size, height, width > 0; at most 131072 cells.  The lists are only read.
 * stats == NULL: the call only enqueues; the results go to stats_dev (caller-owned HBM, S x SLAM_KF_STATS doubles) or, stats_dev == NULL,
 * to a buffer of the set.  stats != NULL: the call ends with the one device -> host copy of S x SLAM_KF_STATS doubles and a wait for ctx's
 * stream; [0] is the list length, so a loop that calls this need not call slam_kpset_counts as well. */
#define SLAM_KF_STATS 8
int slam_kpset_frame_stats(slam_ctx *ctx, slam_kpset *ks, const double *params, int flags, int cell_size, int height, int width,
                           double *stats_dev, double *stats);
/* check_new_kf_required (front_end.jl:361-393) line for line, per stream, on host arrays (no context, no device): stats = the S x
 * SLAM_KF_STATS array of slam_kpset_frame_stats with flags = 1; frames_delta[s] = frame id - key-frame id; prev_kf_nb_3d[s] = the
 * key-frame's own nb_3d_kpts (the mapper and the estimator change it after creation: the host owns it); has_prev_kf[s] = 0: the key-frame
 * is not in the map (:363).  Comparisons are the reference's, in doubles, against its own products (nb < 0.33 * max_nb_keypoints ...).  required[s] = 1: insert a
 * key-frame.  rule (nullable) names the exit: 0 no previous key-frame -> 0 (:363); 1 few occupied cells -> 1 (:367-370); 2 fewer than
 * 20 3-D keypoints and frames_delta >= 2 -> 1 (:371-373); 3 enough 3-D keypoints -> 0 (:374-377); 4 the parallax rule cx && (c0 || c1 ||
 * c2) (:385-392; a NaN median makes cx false). */
int slam_keyframe_required(int S, const double *stats, const int32_t *frames_delta, const int32_t *prev_kf_nb_3d,
                           const uint8_t *has_prev_kf, int max_nb_keypoints, double initial_parallax, int local_ba_on,
                           uint8_t *required, uint8_t *rule);

/* ---- the key-frame map of the lists: gather and apply local-BA windows --------------------------------------------------------------------
 * What local_bundle_adjustment! reads and writes of the map manager (_get_ba_parameters src/estimator.jl:143-266, _update_ba_parameters!
 * :268-306; update_frame_covisibility! map_manager.jl:302-340, remove_mappoint_obs! :224-, remove_mappoint! :139-168, is_bad!
 * map_point.jl:155-161) for S lock-stepped streams whose keypoints live in a slam_kpset: a per-stream map in HBM, filled from the lists,
 * that emits LocalBACache arrays (estimator.jl:16-40) in slam_local_ba_batch's layout and takes the solution back.  One allocation:
 *   ring    R key-frames per stream, 2 <= R <= 64: key-frame k in slot k % R with get_cw_ba (frame.jl:432-437; 6 doubles), the list's ids
 *           (ascending), the undistorted pixels (y, x) and a live flag per observation (a removed observation is a tombstone).  Reusing a
 *           slot first forgets the old key-frame as remove_keyframe! does (map_manager.jl:184-209): its points lose that observer.
 *   table   mcap points per stream: point `id` in entry id % mcap with xyz, a 64-bit observer mask (bit k % R) and the flags is_3d,
 *           observed, ba, gone.  A newer id that lands on an occupied entry replaces it; the old point is gone, its observations are
 *           skipped like a missing map point.
 * `observed` is what the last slam_kfmap_add_keyframe saw (cleared by slam_kfmap_ba_update for what it removes from the frame); it is NOT
 * refreshed every frame as the reference's is_observed is.  Orders the reference takes from Dicts and Sets (a key-frame's 3-D keypoints, a
 * point's observers) are ascending by id; the covisibility walk is newest first over the <= 5 newest covisible key-frames and the dense
 * 1-based ids are numbered in first-encounter order, as in _get_ba_parameters.
 * Ordering across contexts: as for slam_kpset_select -- the map calls run in their ctx's stream order; a host that drives one map (or the
 * map and its set) from several contexts orders the calls against each other and against the list seams with events. */
typedef struct slam_kfmap slam_kfmap;
int slam_kfmap_create(slam_ctx *ctx, int S, int cap, int R, int mcap, slam_kfmap **out);   /* cap >= the set's cap */
int slam_kfmap_destroy(slam_kfmap *km);
/* Record the key-frame slam_kpset_keyframe has just made (call it right after): stream s records key-frame kfcount[s] - 1 from its list
 * (id, pixel, is_3d, map point; a 3-D keypoint's position replaces the point's unless a bundle adjustment has set it).  params: S x 32 as
 * for the seams above -- [0..15] Tcw, whose RotZYX angles and translation become the key-frame's theta; [16..23] fx fy cx cy k1 k2 p1 p2:
 * the stored pixel is undistort_point (camera.jl:98-125) of the list's, or the pixel itself when k1 = k2 = p1 = p2 = 0.  An id the frame
 * has lost (gone) is not recorded.  A KEY-FRAME SEAM: acts on the set's selected streams; the selection is remembered as the map's own (it
 * names the streams slam_kfmap_ba_gather acts on).  Enqueue-only. */
int slam_kfmap_add_keyframe(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, const double *params /* S x 32 */);
/* The windows of the newest key-frames of the streams the last slam_kfmap_add_keyframe acted on, back to back in window order, as
 * slam_local_ba_batch takes them.  The caller owns every array; cap_* are their total capacities (windows; poses: theta_const,
 * poses_remap; points: points_remap; observations: pixels_yx x 2, pose_ids, point_ids, obs_*; theta holds 6 cap_poses + 3 cap_points
 * doubles).  status[s] (S entries): 0 window produced; 1 none (fewer than min_cov_score[s] 3-D keypoints, estimator.jl:321, or no
 * observation: the first key-frame); 2 the window does not fit what is left of the capacities -- nothing of it is written, later windows
 * are unaffected, the stream has no pending window (the is_bad! demotions its gather made stay: any later gather makes them again); 3 not selected.  The bookkeeping arrays (poses_remap, points_remap: key-frame / keypoint id of a dense id; obs_kf,
 * obs_kp, obs_in_covmap per observation) may be NULL.  The map keeps every produced window's bookkeeping, its `bad` set included, as the
 * stream's pending window.  Synchronous: the estimator step's one copy of results (after one small copy of the window sizes). */
typedef struct slam_kfmap_windows {
    int32_t cap_windows, cap_poses, cap_points, cap_obs;
    int32_t *status, *win_stream, *Pn, *Mn, *On;
    double *theta;
    uint8_t *theta_const;
    double *pixels_yx;
    int64_t *pose_ids, *point_ids;
    int64_t *poses_remap, *points_remap, *obs_kf, *obs_kp;
    uint8_t *obs_in_covmap;
} slam_kfmap_windows;
int slam_kfmap_ba_gather(slam_ctx *ctx, slam_kfmap *km, const int32_t *min_cov_score /* S */, const slam_kfmap_windows *out, int32_t *n_windows);
/* _update_ba_parameters! for the pending windows of the listed streams: theta and outliers as slam_local_ba_batch left them (windows back
 * to back, in win_stream's order).  Refined poses and positions go into the map, an outlier observation inside the covisibility map is
 * removed, is_bad! is evaluated after all removals and removes the points it condemns.  Everything goes by key-frame and keypoint id: key-frames
 * added since the gather do not matter, one the ring has forgotten or slam_kfmap_filter has removed meanwhile is skipped.  ks != NULL: the live lists follow -- a 3-D keypoint
 * whose point was kept takes the refined position; an outlier observation of the window's own key-frame (remove_obs_from_current_frame!) and
 * an observed point that was removed leave the list (slam_kpset_remove's compaction); nothing else in the lists changes.  A stream without a
 * pending window is an argument error and nothing is enqueued for any stream; a window is consumed by its update.  Enqueue-only. */
int slam_kfmap_ba_update(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks /* nullable */, int n_windows, const int32_t *win_stream,
                         const double *theta, const uint8_t *outliers);
/* The estimator step on the map in ONE call, the windows never leaving HBM: for the streams the last slam_kfmap_add_keyframe acted on, what
 * slam_kfmap_ba_gather -> slam_local_ba_batch -> slam_kfmap_ba_update(ks) do -- the gather's plan kernel and its headers back (the first wait), the
 * gather's emit kernel into a device block of the map's own (no copy to the host), slam_local_ba_batch_dev on those arrays (camera cams[4 s ..] for
 * stream s), and the update's kernels (with ks: its list kernel and the compaction) on the same arrays.  Windows that batch does not take
 * (SLAM_BA_DEV_INELIGIBLE: e.g. one free pose among several, more than five free poses) take the host route INSIDE the call: their arrays come down,
 * slam_local_ba_batch solves them, theta and the flags go back up, and the one update launch applies them with the others.  status (S): 0 solved and
 * applied, 1 no window (the gather's rule), 3 not selected, SLAM_ERR_NUMERIC (the map is untouched for that stream, as when a host caller skips the
 * update; its window stays pending), SLAM_ERR_ARG.  stats (S x 8, nullable): slam_local_ba_batch's rows, zeros where nothing was solved.  A stream
 * that goes through has no pending window afterwards.  Synchronous up to the update, which is enqueued. */
int slam_kfmap_local_ba(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks /* nullable */, const int32_t *min_cov_score /* S */, const double *cams /* S x 4 */,
                        int iters_fast, int iterations, double repr_eps, int32_t *status /* S */, double *stats /* S x 8, nullable */);
/* P, M, O of the window every stream had in the last slam_kfmap_local_ba (S x 3 ints; zeros: none).  Host bookkeeping, no device work. */
int slam_kfmap_last_windows(slam_kfmap *km, int32_t *pmo);
/* map_filtering! (estimator.jl:358-406) for the streams the last slam_kfmap_add_keyframe acted on: key-frames that share too many well-observed
 * points with the rest of the ring are removed.  Per stream s, with cur = its newest key-frame:
 *   gates        nothing happens when filtering_ratio[s] >= 1 or cur < first_kfid (the reference's literal is 20; a parameter here);
 *   candidates   the covisibility map of cur as the gather forms it -- every other key-frame of the ring that shares at least one live point with
 *                cur (2-D points count) -- walked ASCENDING by key-frame id (the reference walks a Dict).  `kfid == 0 && break` is kept literally:
 *                while key-frame 0 is covisible with cur nothing is filtered.  An id >= cur is passed over.
 *   per candidate   n_total = its live observations whose point is 3-D (an observation without a point is skipped and left as it is); n_good = those
 *                with more than four observers, counted after the removals this call has already made.  n_total < min_cov_score[s] / 2 (integer
 *                division) removes the key-frame; else n_good / n_total > filtering_ratio[s], one division in doubles, removes it (0 / 0 is
 *                NaN: kept).
 * Deviations: n_total stands for kf.nb_3d_kpts as well (the map keeps is_3d per point, no counter per frame); `new_kf_available && break` has no
 * counterpart (lock-stepped streams never race); has_keyframe / remove_covisible_kf! have none (covisibility is derived from the observer masks).
 * A removal is remove_keyframe! (below).  Legal between a gather and its update: the update skips the removed key-frame (pose not copied, its
 * outlier observations not applied).  filtering_ratio[s] must be finite or >= 1, min_cov_score[s] >= 0, first_kfid >= 0, for EVERY stream: on an
 * error nothing is enqueued for any stream.  removed (nullable, S words): bit k % R set for every key-frame this call removed (its id is the one
 * in (cur - R, cur) with that residue; 0 for a stream the call did not act on); non-NULL makes the call synchronous (one 8 S byte copy), NULL
 * leaves it enqueue-only. */
int slam_kfmap_filter(slam_ctx *ctx, slam_kfmap *km, const double *filtering_ratio /* S */, const int32_t *min_cov_score /* S */,
                      int first_kfid, uint64_t *removed);
/* remove_keyframe! (map_manager.jl:184-209) of one key-frame of stream s: every point it observes loses that observer, the slot becomes empty
 * (later downloads answer "not in the ring", the next key-frame with that residue is recorded into an empty slot).  Nothing else changes: no
 * is_bad! evaluation (the reference makes none here; the next gather demotes what became bad), the live lists are untouched, and
 * remove_covisible_kf! has no counterpart.  Not in the ring: no-op; the newest key-frame: argument error.  The check reads the stream's newest id
 * (one 4-byte copy, one wait); the removal itself is enqueued. */
int slam_kfmap_remove_keyframe(slam_ctx *ctx, slam_kfmap *km, int s, int kfid);
/* newest[s] = the id of stream s's newest key-frame, -1 where there is none yet (what turns a bit of `removed` into an id).  Synchronous. */
int slam_kfmap_newest(slam_ctx *ctx, slam_kfmap *km, int32_t *newest /* S */);
/* read-backs (tests, checkpoints).  download_keyframe: *n_out = -1 when key-frame kfid is not in the ring.  download_points: the valid
 * entries in id order; flags bit 0 is_3d, 1 observed, 2 ba, 3 gone; point k's observer key-frame ids, ascending, are
 * obs_kf[obs_off[k] .. obs_off[k + 1]) (obs_off: cap_out + 1 entries).  slam_kfmap_reset empties stream s's map (enqueue-only). */
int slam_kfmap_download_keyframe(slam_ctx *ctx, slam_kfmap *km, int s, int kfid, double *theta, int64_t *ids, double *upx_yx, uint8_t *live,
                                 int cap_out, int *n_out);
int slam_kfmap_download_points(slam_ctx *ctx, slam_kfmap *km, int s, int64_t *ids, double *xyz, uint8_t *flags, int32_t *obs_off,
                               int32_t *obs_kf, int cap_out, int cap_obs, int *n_out);
int slam_kfmap_reset(slam_ctx *ctx, slam_kfmap *km, int s);
/* Descriptors in the map, opt-in (nothing changes for a map that never enables them): one n_bits = 256 row (4 words, the only width the
 * local-map match handles) and a "has descriptor" byte per table entry, 33 mcap bytes per stream in an allocation of their own.  The row of
 * point `id` lives at entry id % mcap under the table's ownership rule; a point replaced by a larger id loses its descriptor with its entry.
 * ONE descriptor per point is the whole of keyframes_descriptors here: map_manager.jl:116-131 describes only the keypoints a key-frame has just
 * extracted; further rows would come from merges, and slam_kfmap_merge keeps one row per point.  Enabling twice is a no-op. */
int slam_kfmap_enable_descriptors(slam_ctx *ctx, slam_kfmap *km, int n_bits);
/* Right after slam_kfmap_add_keyframe, with the arrays slam_kpset_detect_describe has just filled (desc_dev: S x dcap x 4 words, info_dev:
 * S x 2 int64, both in HBM): row j of stream s goes to the entry of id info_dev[2 s] + j where that entry carries the id.  Acts on the streams
 * the last slam_kfmap_add_keyframe acted on.  Enqueue-only. */
int slam_kfmap_add_descriptors(slam_ctx *ctx, slam_kfmap *km, const uint64_t *desc_dev, const int64_t *info_dev, int dcap);
/* update_frame_covisibility! + match_local_map! (map_manager.jl:302-355, mapper.jl:265-383) on the map, for the streams the last
 * slam_kfmap_add_keyframe acted on: the local map of each stream's newest key-frame `cur` is staged in HBM in slam_local_map_match_batch's packed
 * layout and matched by the same kernel; nothing returns to the host between staging and match, the call ends in one copy of the results.
 *   covisible key-frames   every other key-frame of the ring that shares a live point with cur (the gather's and the filter's covisibility);
 *   local map      the points that are 3-D, not removed, have a descriptor, have a live observation in a covisible key-frame and are NOT observed by
 *                  cur, each once, ASCENDING by id (the reference iterates a Set); among equal distances the larger local-map index wins;
 *   keypoints      cur's live observations whose point has a descriptor, in list order (ascending id); a keypoint's observers are its point's
 *                  observer key-frames with the pixel found there, a missing or removed observation skipped (mapper.jl:429-434);
 *   frame          Tcw from cur's theta; nb_3d_kpts = cur's live 3-D points (below 30 the projection distance doubles, mapper.jl:332).
 * cam [S x 10] = fx fy cx cy k1 k2 p1 p2 height width, cell_size, max_projection_distance, max_descriptor_distance [S] as for
 * slam_local_map_match_batch.  max_local bounds a stream's local map (the reference's 10 max_nb_keypoints).  status[s]: 0 matched; 1 nothing to
 * match (not acted on, no covisible key-frame, an empty local map or keypoint list); 2 the local map exceeds max_local -- nothing is matched for
 * that stream, the others are unaffected.  Result: the reference's prev_new_map (mapper.jl:370-382) as pairs (keypoint id, local-map point id),
 * ascending by keypoint id, the streams back to back in stream order (n_pairs[s] each), with the winning descriptor distance; more than
 * cap_pairs pairs in all is a capacity error.  The call changes NOTHING in the map: slam_kfmap_merge applies the pairs.
 * Deviations: the slabs hold undistorted pixels while find_best_match uses kp.pixel, so without the raw-pixel store
 * (slam_kfmap_enable_pixels, below) non-zero k1, k2, p1, p2 of any stream is an argument error (as is a map without descriptors), nothing is
 * launched; with the store the match reads the raw pixels and takes any lens; frame.local_map_ids is kept between key-frames only after
 * slam_kfmap_enable_local_map_history (below); no remove_mappoint_obs! clean-ups; a
 * keypoint outside the cell grid is in no cell.  Memory: a staging allocation with fixed per-stream strides, about cap (100 + 20 R) +
 * max_local (100 + 4 R) + 4 mcap bytes per stream, made by the first call.  Synchronous. */
int slam_kfmap_local_map_match(slam_ctx *ctx, slam_kfmap *km, const double *cam /* S x 10 */, const int32_t *cell_size,
                               const double *max_projection_distance, const double *max_descriptor_distance, int max_local,
                               int32_t *status /* S */, int32_t *n_pairs /* S */, int64_t *pairs /* cap_pairs x 2: keypoint id, local-map id */,
                               double *dist, int cap_pairs);
/* Raw pixels in the map, opt-in (a map that never makes this call launches the same kernels and gets the results it always got): kp.pixel (y, x) of every observation
 * beside the undistorted pixel, 16 R cap bytes per stream in an allocation of their own; a second call is a no-op.  Call it before the first
 * slam_kfmap_add_keyframe: an observation recorded earlier gets its undistorted pixel as its raw one.  From then on slam_kfmap_add_keyframe files
 * the list's pixel as it is beside undistort_point of it, slam_kfmap_merge moves it with the renamed observation, and
 * slam_kfmap_local_map_match stages keypoint and observer pixels -- hence the cell grid (add_keypoint_to_grid!, frame.jl:576-599) -- from the raw
 * pixels, as find_best_match does (mapper.jl:405-442), and accepts non-zero k1, k2, p1, p2.  The gather, the update, the filter and
 * slam_kfmap_triangulate_temporal keep reading the undistorted pixels. */
int slam_kfmap_enable_pixels(slam_ctx *ctx, slam_kfmap *km);
/* The raw pixels of key-frame kfid of stream s, in the order of slam_kfmap_download_keyframe's ids: *n_out = -1 when the key-frame is not in the
 * ring; more than cap_out: a capacity error.  An argument error without the store.  Synchronous. */
int slam_kfmap_download_pixels(slam_ctx *ctx, slam_kfmap *km, int s, int kfid, double *px_yx, int cap_out, int *n_out);
/* The local-map history: frame.local_map_ids of every key-frame of the ring, kept in HBM between key-frames.  Opt-in, ONE allocation of about
 * R mcap / 8 + 8 mcap bytes per stream (a bitset over the table's entries per ring slot, the key-frame each set belongs to, a copy of the table's
 * tags as of the stream's last match); a second call is a no-op.  From then on slam_kfmap_local_map_match, for the newest key-frame K of every
 * stream it acts on: (0) drops from the stream's stored sets every id whose table entry another id has taken; (1) forms C, the local map of K's
 * covisibility pass (what the call yields without history; empty without a covisible key-frame); (2) map_manager.jl:350-354: with P the set stored
 * for K (empty unless the match already ran for K), L = C if |C| > 0.5 |P|, else P + C; (3) mapper.jl:274-286: if a key-frame is covisible and
 * |L| < max_local, L takes in the set stored for the covisible key-frame of the smallest id, if one was stored for it; (4) stores L as K's set,
 * whatever the status; (5) stages the ids of L that pass the match's gates now (alive, 3-D, described, not observed by K), ascending: more than
 * max_local is status 2, none status 1.  A stored set holds ids that passed the gates when they were stored (the reference stores raw ids and gates
 * at match time).  Sets grow along the chain: max_local >= mcap rules status 2 out.  slam_kfmap_merge leaves the sets alone; slam_kfmap_reset clears
 * the stream's.  A map that never makes this call behaves exactly as before. */
int slam_kfmap_enable_local_map_history(slam_ctx *ctx, slam_kfmap *km);
/* The set stored for key-frame kfid of stream s, ascending (n_ids of them).  kfid not in the ring, or no set stored for it (its match was
 * skipped): an argument error; more than cap_ids: a capacity error (n_ids is set).  Synchronous. */
int slam_kfmap_download_local_map_ids(slam_ctx *ctx, slam_kfmap *km, int s, int kfid, int64_t *ids, int cap_ids, int32_t *n_ids);
/* merge_matches -> merge_mappoints -> update_keypoint! (mapper.jl:296-310, map_manager.jl:378-427, frame.jl:290-307) on the map: the pairs
 * (prev_id, new_id) = (keypoint of the newest key-frame, local-map point) of a local-map match are applied in HBM, with no host round trip between
 * match and merge.  n_pairs == NULL takes the result block of the last slam_kfmap_local_map_match where it lies in HBM (a stream whose status
 * was not 0 has no pairs; a block is consumed once); otherwise n_pairs[s] pairs per stream, the streams back to back in `pairs`, are uploaded
 * through the map's pinned block.  The call acts only on the streams that have pairs.  Per stream and pair:
 *   validity    skipped, nothing changed, unless both ids own their table entries (not removed), prev_id != new_id and the new point is 3-D;
 *   observers   in every key-frame of prev's observers whose slab holds a live observation of prev_id and none of new_id, that observation's
 *               id becomes new_id (pixel and live byte kept) and the new point gains the observer; a slab that holds both is left as it is
 *               (has_new: the prev observation stays, an orphan);
 *   order       every touched slab holds unique ascending ids again: the renamed record moves to its place, a tombstone whose id equals an
 *               arriving new_id is dropped, other tombstones stay; a slab never grows;
 *   points      prev's entry is removed as by pop!(map_points, prev_id) -- NOT remove_mappoint!: observations that were not renamed stay in their
 *               slabs; the new point is `observed` if the newest key-frame's slab was renamed to it; its position and `ba` are untouched;
 *   live list   (ks != NULL) a list that carries prev_id and not new_id: the slot takes new_id, is_3d = 1 and the new point's position in the map,
 *               every other field of the record travels with it, the list is re-ordered so that ids ascend, its count is unchanged;
 *   ks == NULL  prev's entry is also marked `gone`: later lists that still carry prev_id are not recorded as a fresh point.
 * The pairs of a stream must be one-to-one (no prev id twice, no new id twice, no id on both sides of two pairs): the merges then commute.  A
 * stream that has pairs and a pending local-BA window (the reference merges under optimization_lock), host pairs that are not one-to-one,
 * more than cap pairs for a stream, and n_pairs == NULL on a map without descriptors or without a match are argument errors: nothing is
 * enqueued for any stream.  Device pairs that are not one-to-one are reported in the status word, that stream unchanged.
 * merged (nullable) [S x 4]: pairs applied, pairs skipped, observations renamed in key-frames, status (0; 1 not one-to-one); zeros for a
 * stream without pairs.  merged == NULL: enqueue-only; else one copy and one wait more.
 * Deviations: add_covisibility! has no counterpart (covisibility is derived from the observer masks); the map keeps ONE descriptor row per
 * point, so the new point keeps its own and prev's row goes with prev (the reference appends prev's rows to keyframes_descriptors and
 * mappoint_min_distance takes the minimum over all of them); the `gone` mark of ks == NULL.  Memory: a scratch allocation made by the first
 * call that has pairs -- per slab and per list the rename list and the rebuild's plan (28 bytes a record), a scratch slab per (stream, slot)
 * (25 bytes a record), a scratch record array per list (103 bytes a record): about (53 R + 132) cap bytes per stream. */
int slam_kfmap_merge(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks /* nullable */, const int32_t *n_pairs /* S, or NULL */,
                     const int64_t *pairs /* x 2, streams back to back, or NULL */, int32_t *merged /* nullable, S x 4 */);
/* Descriptor rows: a point keeps one row per key-frame, the reference's keyframes_descriptors (map_point.jl:15).  Opt-in, after
 * slam_kfmap_enable_descriptors, ONE allocation of about 36 max_rows mcap bytes per stream: per table entry D = max_rows (2 .. 8) keys (key-frame id
 * + 1, 0 = empty slot) and D rows of 4 words, and a dropped-rows counter per stream.  A second call with the same D is a no-op, another D an argument
 * error.  A map that never makes this call behaves, allocates and launches exactly as before.  From then on:
 *   add_descriptors   the row also goes into the point's rows under the key of the stream's newest key-frame (add_mappoint!'s current_keyframe_id);
 *   observations      wherever a live point loses an observer -- a ring slot reused, slam_kfmap_filter, slam_kfmap_remove_keyframe, an outlier
 *                     observation of slam_kfmap_ba_update, an observer whose pixel is gone at slam_kfmap_ba_gather -- the row keyed by that
 *                     key-frame goes (remove_kf_observation!, map_point.jl:88-122); with the last valid observer every row goes and the point is no
 *                     longer described ("mp.descriptor is empty": the local map and the keypoint list pass it over);
 *   owners            an entry that takes a new owner loses its rows; slam_kfmap_reset clears the stream's rows and its counter;
 *   merge             the new point takes prev's rows by key; on an equal key its own row stays (add_descriptor!, map_point.jl:124-131,
 *                     map_manager.jl:410-412); prev's rows go with prev;
 *   match             every row of a local-map point and of a keypoint is staged, ascending by key: the distance of a pair is the minimum over ALL
 *                     pairs of rows (mappoint_min_distance, map_point.jl:165-174).  A described point without a row is staged with an empty row
 *                     range and is never chosen.  The staging allocation's descriptor regions hold D rows per record.
 * Deviations: a point keeps at most D rows -- where a row arrives at a full point the D rows with the LARGEST keys stay, whatever the order of
 * arrival, and the stream's counter counts the rows that went; the reference's most representative `descriptor` is read by nothing but its
 * emptiness test and is not modelled (the single row of slam_kfmap_enable_descriptors stays what add_descriptors wrote and is not staged); a
 * reused ring slot counts as remove_keyframe!. */
int slam_kfmap_enable_descriptor_rows(slam_ctx *ctx, slam_kfmap *km, int max_rows);
/* The rows of stream s's points: the owned points that have not been removed, ascending by id (the set slam_kfmap_download_points lists;
 * n_points of them).  Point k: ids[k], described[k] (the "has descriptor" byte), its rows rows[4 j .. 4 j + 4) with keys[j] = the key-frame id,
 * j in row_off[k] .. row_off[k + 1), ascending by key (row_off: cap_points + 1 entries).  dropped: the rows the bound D has dropped on this
 * stream since its creation or reset.  Every array is nullable.  More than cap_points points, or (keys or rows given) more than cap_rows rows: a
 * capacity error (n_points is set); a map without rows: an argument error.  Synchronous. */
int slam_kfmap_download_descriptor_rows(slam_ctx *ctx, slam_kfmap *km, int s, int64_t *ids, uint8_t *described, int32_t *row_off, int32_t *keys,
                                        uint64_t *rows, int cap_points, int cap_rows, int32_t *n_points, int32_t *dropped);
/* triangulate_temporal! (mapper.jl:185-262) from the map's own key-frames, for the streams the last slam_kfmap_add_keyframe acted on (call it after
 * that seam: the reference runs it on the map's copy of the new key-frame).  Every input is in HBM: the slabs' undistorted pixels, the key-frames'
 * theta AS THE LAST BUNDLE ADJUSTMENT LEFT IT, the observer masks, the table's flags; cams[4 s ..] = fx fy cx cy of stream s.  With k the newest
 * key-frame of a stream, every live observation of its slab:
 *   1  is skipped if its point is missing (the entry carries another id), removed, or 3-D already (get_2d_keypoints, :208-211);
 *   2  is skipped if its point has fewer than two observers (:215) or if the FIRST observer -- the smallest key-frame id among the point's
 *      observers as they are now, after every removal, ring reuse and outlier tombstone -- is k itself (:217);
 *   3  is skipped if the first observer's slab does not hold the id alive (:234-235);
 *   4  else the pair (first observer's stored pixel, k's stored pixel) is triangulated exactly as slam_kpset_triangulate_temporal does it (the DLT,
 *      both depth gates, both reprojection gates; a failed gate counts only when the rotation-compensated parallax exceeds min_parallax), with
 *      rel_pose = observer.cw * frame.wc from the two thetas and the closed-form rigid inverse;
 *   accepted (update_mappoint!): the point's position becomes observer.wc * X and it becomes 3-D (`ba` is not set); ks != NULL: the list slot that
 *      carries the id now (found by binary search: a merge may have moved it; an id the list no longer holds is no error) takes xyz and is_3d = 1;
 *   rejected (remove_mappoint_obs!(map, id, k)): k's observation becomes a tombstone, the point loses observer k, with descriptor rows the row keyed
 *      k goes.  THE LIVE LIST KEEPS THE KEYPOINT, as the reference's current frame does -- unlike slam_kpset_triangulate_temporal, which compacts it away.
 * Deviations: the list keeps a rejected keypoint; no remove_mappoint_obs! clean-up for a missing point (rule 1), as elsewhere in the map; the first
 * observer is the smallest id (the reference's observers are an ordered set, of which this is the first).  ks == NULL: the lists are the host's
 * business (their is_3d and xyz do not follow).  An unselected stream's map and list are untouched.  counts (nullable) [S x 4]: candidates after
 * rule 1, triangulated, observations removed, skipped by rules 2-3; zeros for a stream the call did not act on.  counts == NULL: enqueue-only; else
 * one copy of S x 4 ints and one wait.  Legal between a gather and its update: the pending window is untouched. */
int slam_kfmap_triangulate_temporal(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks /* nullable */, const double *cams /* S x 4: fx fy cx cy */,
                                    double max_error, double min_depth, double min_parallax, int32_t *counts /* S x 4, nullable */);

/* ---- one live stream, one call per frame (round 6) -----------------------------------------------------------------------------------
 * What run!() does per frame (src/front_end.jl:58-113: preprocess! :454-470 = copy!(previous_pyramid, current_pyramid) + update!,
 * klt_tracking! -> optical_flow_matching! map_manager.jl:451-564; at a key-frame create_keyframe! -> extract_keypoints!
 * map_manager.jl:98-113 and the mapper's right pyramid + stereo matching + triangulate_stereo! mapper.jl:51-66, :142-183) as ONE entry:
 * the frame's bytes are copied to HBM, the single-image build graph, the 3-D / 2-D matching passes, the removal of lost keypoints and
 * (key-frame) detection, right build, stereo match and triangulation are ENQUEUED back to back -- no host code between them -- and the call
 * returns with the one number a front-end needs per frame, the length of the keypoint list.  The lists live in HBM (a slam_kpset with one
 * stream); three left pyramids rotate (copy! = a handle rotation).
 *   lookahead = 0: step(frame t) returns frame t's list: latency = build + match.
 *   lookahead = 1: step(frame t + 1) starts that frame's build on the build stream and returns frame t's list (whose build ran during the
 *                  call before): one frame of latency buys the overlap of build and matching -- a recorded sequence, or a camera whose
 *                  next frame has arrived while the current one is processed (the "next frame only" figure of bench.py).
 * config: plain scalars mirroring Params (params.jl:58-82) and the Extractor (extractor.jl:7-22).  Per-call: params / stereo_params =
 * 32 doubles each as for slam_kpset_flow_match / _stereo_match (prior as there); tri = P1 (16), P2 (16), T21 (16), cam1 (4), cam2 (4),
 * Twc (16) as for slam_kpset_triangulate (read at key-frames with a right image); cull_flags_dev (nullable): cap bytes in HBM, 1 = remove
 * before detection (map culling).  right_u8 != NULL marks the fed frame as a key-frame.  frame_out: index (0-based, feed order) of the frame
 * whose list length count_out reports, -1 while the pipeline fills (first call with lookahead = 1); slam_frontend_flush processes the
 * frame still in flight.  The per-frame arguments describe the frame that is PROCESSED by the call. */
typedef struct slam_frontend slam_frontend;
typedef struct slam_frontend_config {
    int32_t H, W, pyramid_levels, pyramid_levels_3d, window, iterations;
    int32_t max_points, radius, grid_rows, grid_cols, cell_size, cap;
    int32_t pyr_mode;            /* 1: bit-exact update!, 3: tolerance mode */
    int32_t lookahead;           /* 0 / 1 */
    int32_t right_target_only;   /* build the right pyramid with SLAM_PYR_TARGET_ONLY */
    int32_t reserved;
    double eig_thr, eps, max_distance, sigma_mask, min_response, epipolar_error, max_error, min_depth, pyr_sigma;
} slam_frontend_config;
int slam_frontend_create(int device, const slam_frontend_config *cfg, slam_frontend **out);
int slam_frontend_destroy(slam_frontend *fe);
int slam_frontend_step(slam_frontend *fe, const uint8_t *left_u8, const uint8_t *right_u8, const double *params, int prior,
                       const double *stereo_params, int stereo_prior, const double *tri, const uint8_t *cull_flags_dev,
                       int32_t *frame_out, int32_t *count_out);
int slam_frontend_flush(slam_frontend *fe, const double *params, int prior, const double *stereo_params, int stereo_prior,
                        const double *tri, const uint8_t *cull_flags_dev, int32_t *frame_out, int32_t *count_out);
/* the stream's keypoint set (slam_kpset_download ...) and its tracking context (owned by the front-end) */
slam_kpset *slam_frontend_keypoints(slam_frontend *fe);
slam_ctx   *slam_frontend_ctx(slam_frontend *fe);
const char *slam_frontend_last_error(slam_frontend *fe);

/* ---- bundle adjustment ------------------------------------------------------ */
/* Array-level body of triangulate_stereo! (parallax == NULL: every gate applies, src/mapper.jl:142-183) and
 * triangulate_temporal! (a gate removes the observation only when parallax[i] > min_parallax, :185-262), for n
 * keypoints in one launch: DLT triangulation from the two undistorted pixels (RecoverPose.triangulate, :162,242),
 * division by the 4th component, depth gates in both cameras (min_depth = 0.1), reprojection gates against
 * max_error in both images.  P1, P2 (projection matrices), T21 (camera 1 -> camera 2: right_camera.Ti0 or
 * inv(rel_pose)): 4x4 column-major as Julia SMatrix{4,4}; cam = (fx, fy, cx, cy); pixels (y, x).
 * out_xyz[3 i..]: the point in camera-1 coordinates (the caller applies project_camera_to_world);
 * status[i] = 1: update the map point, 0: remove the keypoint / observation. */
int slam_triangulate(slam_ctx *ctx, const double *P1, const double *P2, const double *T21,
                     const double *cam1, const double *cam2,
                     const double *px1_yx, const double *px2_yx, int n,
                     double max_error, double min_depth,
                     const double *parallax, double min_parallax,
                     double *out_xyz, uint8_t *status);

/* Array-level body of the mapper's local-map re-matching -- do_local_map_matching + find_best_match + mappoint_min_distance
 * (src/mapper.jl:318-462, src/map_point.jl:165-174), the consumer of slam_describe's descriptors (map_manager.jl:108-112).  The hash-map work
 * around it (union! of local-map ids :274-286, merge_mappoints :296-310, the remove_mappoint_obs! clean-ups :412, :429-434) stays with the caller.
 * All arrays are host arrays; the batch form (S lock-stepped streams, no reference counterpart) concatenates every array over the streams:
 * stream s owns the keypoints [kp_offsets[s], kp_offsets[s+1]), the key-frame rows [kf_offsets[s], ..) and the local-map points
 * [mp_offsets[s], ..) (S + 1 entries each, first 0), the CSR offset arrays run over the concatenated keypoints / points, and key-frame rows in
 * the observer lists are local to their stream.  slam_local_map_match is the batch of one stream with N keypoints, K key-frames, M points.
 *   Tcw [S x 16]            frame.cw, 4x4 column-major (frame.jl:458-462)
 *   cam [S x 10]            fx, fy, cx, cy, k1, k2, p1, p2, height, width of the Camera frames and key-frames share (camera.jl:79-125)
 *   cell_size [S]           frame.cell_size (SLAM.jl:42-45; the grid is ceil(height / cell_size) x ceil(width / cell_size))
 *   nb_3d_kpts [S]          frame.nb_3d_kpts: below 30 the projection distance is doubled (mapper.jl:332)
 *   max_projection_distance, max_descriptor_distance [S]   the keyword arguments (mapper.jl:290-291, :320)
 *   kp_yx [N x 2]           kp.pixel of the frame's keypoints, 1-based (y, x), in the caller's list order (mapper.jl:407); the candidates of a
 *                           cell are met in this order (the reference iterates a Set there, frame.jl:588), and it decides ties
 *   kp_desc_off [N + 1], kp_desc [. x 4]   values(keyframes_descriptors) of each keypoint's map point (map_point.jl:168), one row of
 *                           slam_describe's out_bits (4 x uint64) per descriptor; a keypoint given none is skipped (mapper.jl:406, :411-415)
 *   kp_obs_off [N + 1], kp_obs_kf [.], kp_obs_yx [. x 2]   get_observers(mp) as rows of the key-frame table and observer_kp.pixel in that
 *                           key-frame (mapper.jl:419, :427-438)
 *   kf_Tcw [K x 16]         observer_kf.cw of every key-frame the observer lists name (mapper.jl:436-437)
 *   mp_xyz [M x 3]          get_position(mp) of the local map in the caller's iteration order of frame.local_map_ids, without the entries
 *                           mapper.jl:338-341 skips
 *   mp_desc_off [M + 1], mp_desc [. x 4]   values(target_mp.keyframes_descriptors) (map_point.jl:168)
 *   mp_obs_off [M + 1], mp_obs_kf [.]      get_observers(target_mp) (mapper.jl:397)
 * Outputs:
 *   match [N]       the local-map index prev_new_map maps keypoint j to, or -1 (mapper.jl:370-382)
 *   best_kp [M]     find_best_match's best_id as a keypoint index of the stream, or -1 (mapper.jl:461)
 *   best_dist [M]   its best_distance (256 max_descriptor_distance when nothing was taken); -1 where find_best_match was not called
 *   proj_yx [M x 2] the projection (mapper.jl:351), NaN where a gate of :346-352 dropped the point
 * Semantics kept: gates in the reference's order (z < 0.1, |z / norm| < cos(atan(max(0.5 H / fy, 0.5 W / fx))), project_undistort, in_image);
 * cell = round-to-even(p) / cell_size + 1, cells outside the grid skipped one by one (frame.jl:584-586); cells r outer / c inner; both selections
 * compare with <=, so among equal distances the LAST candidate wins (:445, :375); a keypoint without listed observers has the mean 0/0 = NaN and
 * passes (:441-442); distance = min popcount(d1 xor d2) over all descriptor pairs as a double, start value 256 max_descriptor_distance (:401).
 * A stream with N = 0 or M = 0 returns -1 everywhere (NaN in proj_yx) and launches nothing.  Decreasing offsets, an observer row outside its
 * stream's key-frame table, a keypoint outside the grid or a null array are argument errors: nothing is copied or launched.
 * Per stream the call moves about M (24 + 32 D + 4 O) + N (16 + 32 D + 20 O) + 4 (cells + N) bytes (D descriptors, O observers per point): under
 * 2 MB at M = 10 000, N = 1 000 -- bound by latency and issue, not by bandwidth. */
typedef struct slam_local_map_args {
    const double *Tcw, *cam;
    const int32_t *cell_size, *nb_3d_kpts;
    const double *max_projection_distance, *max_descriptor_distance;
    const double *kp_yx;
    const int32_t *kp_desc_off;
    const uint64_t *kp_desc;
    const int32_t *kp_obs_off, *kp_obs_kf;
    const double *kp_obs_yx;
    const double *kf_Tcw;
    const double *mp_xyz;
    const int32_t *mp_desc_off;
    const uint64_t *mp_desc;
    const int32_t *mp_obs_off, *mp_obs_kf;
    int32_t *match, *best_kp;
    double *best_dist, *proj_yx;
} slam_local_map_args;
int slam_local_map_match(slam_ctx *ctx, const slam_local_map_args *args, int N, int K, int M);
int slam_local_map_match_batch(slam_ctx *ctx, int S, const int32_t *kp_offsets, const int32_t *kf_offsets, const int32_t *mp_offsets,
                               const slam_local_map_args *args);

/* p3p_ransac(points, pixels, pdn, K; threshold) of compute_pose! (src/front_end.jl:164-167; result consumed at
 * :174-186: n_inliers, (KP, inliers, error)).  pts3d n x 3 map points, px_xy n x 2 undistorted pixels in (x, y)
 * order (front_end.jl:150-151), pdn n x 3 bearing vectors normalize(kp.position) (:149), K 3x3 column-major.
 * `samples`: iters x 3 point indices, 0-BASED, drawn by the caller (the reference's RNG stream cannot be
 * reproduced outside Julia; same convention as the BRIEF pattern) -- every triple is solved (Grunert P3P, up to
 * 4 poses) and scored on the GPU, one workgroup per triple; triples with a repeated or out-of-range index are
 * skipped.  Winner: most inliers (depth > 0 and reprojection error < threshold), ties to the lower iteration.
 * KP = K [R | t] (3x4 column-major; the reference recovers the pose as iK * KP, :182), Rt = [R | t] itself (may be
 * NULL), inliers n bytes, *error = sum of the inliers' reprojection errors (may be NULL), *best_iter (may be NULL).
 * *n_inliers = 0 (and zeros elsewhere) when no triple gave a pose -- the reference's `res === nothing` branch. */
int slam_p3p_ransac(slam_ctx *ctx, const double *pts3d, const double *px_xy, const double *pdn, int n,
                    const double *K, double threshold, const int32_t *samples, int iters,
                    double *KP, double *Rt, uint8_t *inliers, int *n_inliers, double *error, int *best_iter);

/* five_point_ransac(previous_points, current_points, previous_pd, current_pd, K, K, cache; max_repr_error) of
 * compute_pose_5pt! (src/front_end.jl:305-308; result consumed at :305-331: n_inliers, (_, P, inliers, _)).
 * px1/px2: n x 2 undistorted pixels (x, y) of the previous key-frame / the current frame (:271-272), pd1/pd2:
 * n x 2 normalised coordinates position[[1, 2]] (:273-274), K1/K2 3x3 column-major.  `samples`: iters x 5 point
 * indices, 0-BASED, drawn by the caller; every 5-tuple is solved (Nister's five-point algorithm, <= 10 essential
 * matrices; pose of each by Horn's closed form + cheirality on the five points) and scored on the GPU: a
 * correspondence is an inlier iff its DLT triangulation lies in front of both cameras and both reprojection
 * errors are < max_repr_error.  Winner: most inliers, ties to the earlier tuple.
 * E: 3x3 column-major (may be NULL), P = [R | t] 3x4 column-major, previous -> current, |t| = 1 (the caller
 * rescales t, front_end.jl:321-329), inliers n bytes, *error = sum of both errors over the inliers (may be
 * NULL), *best_iter (may be NULL).  *n_inliers = 0 when no tuple gave a pose. */
int slam_five_point_ransac(slam_ctx *ctx, const double *px1_xy, const double *px2_xy, const double *pd1_xy,
                           const double *pd2_xy, int n, const double *K1, const double *K2, double max_repr_error,
                           const int32_t *samples, int iters, double *E, double *P, uint8_t *inliers,
                           int *n_inliers, double *error, int *best_iter);

/* The pose seams for S lock-stepped streams (no reference counterpart, like the other *_batch entry points): S
 * independent problems in one set of launches, results identical to S single calls.  Problem z owns the elements
 * [offsets[z], offsets[z+1]) of the concatenated point arrays (offsets[0] = 0; offsets has S + 1 entries; empty
 * problems are allowed and report n_inliers = 0); per-problem matrices are stored back to back (K: S x 9, KP / Rt /
 * P: S x 12, E: S x 9, poses: S x 16, cams: S x 4 as fx, fy, cx, cy); samples are S x iters x 3 (x 5), indices
 * local to their problem. */
int slam_p3p_ransac_batch(slam_ctx *ctx, int S, const int32_t *offsets, const double *pts3d, const double *px_xy,
                          const double *pdn, const double *K, double threshold, const int32_t *samples, int iters,
                          double *KP, double *Rt, uint8_t *inliers, int *n_inliers, double *error, int *best_iter);
int slam_five_point_ransac_batch(slam_ctx *ctx, int S, const int32_t *offsets, const double *px1_xy, const double *px2_xy,
                                 const double *pd1_xy, const double *pd2_xy, const double *K1, const double *K2,
                                 double max_repr_error, const int32_t *samples, int iters, double *E, double *P,
                                 uint8_t *inliers, int *n_inliers, double *error, int *best_iter);
/* slam_pnp_ba for S poses, one workgroup per problem */
int slam_pnp_ba_batch(slam_ctx *ctx, int S, const int32_t *offsets, const double *cams, const double *poses_cw,
                      const double *pixels_yx, const double *points_xyz, int iters_fast, int iterations,
                      double depth_eps, double repr_eps, double *out_poses, double *err_init, double *err_final,
                      uint8_t *outliers, int *n_outliers);

/* bundle_adjustment!(cache::LocalBACache, camera; iterations, repr_eps) --
 * src/bundle_adjustment.jl:1-111 on the flat arrays of src/estimator.jl:16-40:
 * theta = [6P (RotZYX t1,t2,t3, tx,ty,tz) ; 3M], pixels (y,x) 2 x O, 1-based ids.
 * Two passes: iters_fast LM iterations on all observations, outlier flagging
 * (depth < 1e-6 or squared pixel error > repr_eps), then `iterations` LM
 * iterations with outliers zeroed.  The LM outer loop is LeastSquaresOptim's;
 * the step is the exact one from the Schur-complement reduced camera system.
 * stats (may be NULL, 8 doubles): ssr_init, ssr_pass1, ssr_final, iters_pass1,
 * iters_pass2, n_outliers, device_ms, 0. */
int slam_local_ba(slam_ctx *ctx, double fx, double fy, double cx, double cy,
                  int P, int M, int O,
                  double *theta, const uint8_t *theta_const, const double *pixels_yx,
                  const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                  int iters_fast, int iterations, double repr_eps, double *stats);

/* bundle_adjustment! for S windows in one set of launches (no reference counterpart, like the other *_batch entry points): the
 * caller is the estimator task of S lock-stepped SlamManagers -- every key-frame of every manager owes one local_bundle_adjustment!
 * (src/estimator.jl:78-99, :317-347; src/bundle_adjustment.jl:35-54).  Window z has Pn[z] poses, Mn[z] points, On[z] observations and
 * camera cams[4 z ..] = fx, fy, cx, cy; the arrays of the windows are stored back to back in window order: theta (6 Pn[z] + 3 Mn[z]
 * doubles each, in / out), theta_const (Pn[z] bytes), pixels_yx (2 On[z] doubles), pose_ids / point_ids (On[z], 1-based, local to the
 * window), outliers (On[z] bytes, out), stats (8 doubles per window as slam_local_ba's, may be NULL).  Each window runs its own
 * device-side Levenberg-Marquardt state (a converged window idles) and its results equal slam_local_ba's on its arrays TO ROUNDING
 * (theta <= 1e-6 relative, costs 1e-8; the batch kernels sum a window's points in a different order and solve the reduced system with
 * another elimination, so the outlier flag of an observation whose squared residual lies within rounding of repr_eps may differ
 * between the two entry points -- none does in the test suite's windows); windows the
 * banded group kernels do not cover (no banded pose order, a point with > 448 observations, no observations) are solved one by one
 * after the batch.  status (S ints, may be NULL): per-window code -- 0, SLAM_ERR_NUMERIC (reduced system not positive definite: that
 * window's theta / outliers are left unchanged) or SLAM_ERR_ARG; with status the call returns SLAM_OK unless the batch itself failed,
 * without it the first window error is returned.  stats[6] of every window is the device time of the WHOLE batch (one set of
 * launches).  Host set-up runs on a parked pool of min(max(hardware threads / 4, 4), 32) threads (SLAMHIP_BA_THREADS overrides).
 * Windows of <= 5 consecutive free poses are solved by one launch with one or two workgroups each; the two-workgroup form waits
 * for its partner with a bound and, should the partner not show up (compute units held by other processes), the call is solved
 * again with one workgroup per window -- a slow call, never a hung queue. */
int slam_local_ba_batch(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                        double *theta, const uint8_t *theta_const, const double *pixels_yx,
                        const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                        int iters_fast, int iterations, double repr_eps, double *stats, int32_t *status);

/* slam_local_ba_batch on windows that are RESIDENT IN HBM: the arguments are slam_local_ba_batch's, except that theta (in / out), theta_const,
 * pixels_yx, pose_ids, point_ids and outliers (out) are DEVICE pointers, the windows back to back exactly as the host form takes them; cams, Pn, Mn,
 * On, stats and status stay host arrays.  Nothing of a window crosses the bus: a probe kernel reports a few ints per window (free poses, the largest
 * per-point observation count, the observations of free poses, the two checks below), a stager kernel writes each window's solver arrays in place in
 * the batch arena, the solve is slam_local_ba_batch's one-workgroup kernel (two workgroups per window where the device has room, with the same bounded
 * wait and the same second attempt on one workgroup -- which stages the windows again, the solver having moved the parameters it was given), and a
 * results kernel writes theta (the caller's pose order) and the outlier flags back; only the LM states come back to the host, for stats and status.
 * Contract: a window's observations are grouped by map point in ascending point id (what slam_kfmap_ba_gather's emit kernel writes); a window that
 * breaks the rule, names an id out of range or has a map point observed twice by one free pose gets SLAM_ERR_ARG in status, found on the device.
 * Scope: the windows the one-workgroup kernel takes under the rule slam_local_ba_batch applies -- 2 .. 5 free poses once the poses are relabelled so
 * that the free ones are consecutive (constant poses first, then the free ones, each in the caller's order; one free pose among several is not such a
 * window, nor is a window of one pose), <= 128 poses, 1 .. 40000 observations, <= 168 observations of one point.  Any other window gets
 * SLAM_BA_DEV_INELIGIBLE.  A window with a code other than 0 keeps its arrays bit for bit (SLAM_ERR_NUMERIC included) and the rest of the batch is
 * solved.  Results equal slam_local_ba_batch's on the same arrays to rounding (theta <= 1e-6 relative, costs 1e-8: the map points are summed in the
 * caller's order here, in the planner's there).  With status the call returns SLAM_OK unless the batch itself failed; without it the first window
 * code is an error of the call.  The device arrays are read and written on the context's stream; the call returns after the results kernel has run. */
int slam_local_ba_batch_dev(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                            double *theta, const uint8_t *theta_const, const double *pixels_yx,
                            const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                            int iters_fast, int iterations, double repr_eps, double *stats, int32_t *status);

/* slam_local_ba_batch (the host-array form) in two halves (round 6): _begin hands everything -- structure analysis, staging, upload, solve, download, scatter into the
 * caller's arrays -- to a thread of the library's own and returns at once; _end waits for it and returns the call's code (message:
 * slam_last_error).  The estimator task (src/estimator.jl:78-99) prepares the next key-frame's windows while this one's are planned and
 * solved, without a host thread of its own.  Between the two calls the context belongs to the job -- no other call on it; one job per
 * context, several contexts for several batches in flight -- and every array passed to _begin stays valid and untouched (theta, outliers,
 * stats and status are written by the job).  slam_ctx_destroy waits for a job still in flight. */
int slam_local_ba_batch_begin(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                              double *theta, const uint8_t *theta_const, const double *pixels_yx,
                              const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                              int iters_fast, int iterations, double repr_eps, double *stats, int32_t *status);
int slam_local_ba_batch_end(slam_ctx *ctx);

/* pnp_bundle_adjustment(camera, pose, pixels, points; iterations, depth_eps,
 * repr_eps) -- src/bundle_adjustment.jl:113-171.  pose_cw/out_pose: 4x4
 * column-major.  out_pose = identity when fewer than 5 inliers remain (:157-161). */
int slam_pnp_ba(slam_ctx *ctx, double fx, double fy, double cx, double cy,
                const double pose_cw[16], const double *pixels_yx, const double *points_xyz, int n,
                int iters_fast, int iterations, double depth_eps, double repr_eps,
                double out_pose[16], double *err_init, double *err_final,
                uint8_t *outliers, int *n_outliers);

/* Point-sharded BA for multi-GPU windows: each rank owns the
 * observations of a subset of map points; per LM iteration it produces its
 * contribution [S (6P x 6P col-major) ; rhs (6P) ; diag(Jp'Jp) (6P) ; ssr ; pad]
 * into a caller-provided DEVICE buffer of slam_ba_reduce_len(P) doubles, which
 * the host all-reduces (RCCL via torch.distributed) before slam_ba_solve.
 * theta holds ALL poses (replicated) and this shard's points. */
int    slam_ba_create(slam_ctx *ctx, double fx, double fy, double cx, double cy,
                      int P, int M_local, int O_local,
                      const double *theta, const uint8_t *theta_const, const double *pixels_yx,
                      const int64_t *pose_ids, const int64_t *point_ids_local, slam_ba **out);
int    slam_ba_destroy(slam_ba *ba);
int64_t slam_ba_reduce_len(int P);
/* linearise at the current theta and write the local contribution.  A shard keeps ONE reduce buffer for its lifetime: from the second
 * build on only the blocks inside the band of the reduced system (and rhs / diag / ssr) are rewritten -- the rest of the buffer was
 * zeroed by the first build and must not be written by anyone else (an in-place all-reduce keeps zeros zero). */
int    slam_ba_build(slam_ctx *ctx, slam_ba *ba, int ignore_outliers, double inv_delta, double *reduce_dev);
/* solve the (all-reduced) system, back-substitute local points, evaluate the
 * trial step: writes [trial_ssr_local, predicted_ssr_local, max|dx| local, 0]
 * to trial_dev (4 doubles, device) */
int    slam_ba_solve(slam_ctx *ctx, slam_ba *ba, const double *reduce_dev, double inv_delta, double *trial_dev);
/* accept (1) or reject (0) the trial step */
int    slam_ba_commit(slam_ctx *ctx, slam_ba *ba, int accept);
/* flag outliers at the current theta; returns local count through n_out */
int    slam_ba_flag_outliers(slam_ctx *ctx, slam_ba *ba, double repr_eps, double depth_eps, int *n_out);
/* read back theta (6P + 3 M_local) and the outlier flags (O_local) */
int    slam_ba_download(slam_ctx *ctx, slam_ba *ba, double *theta, uint8_t *outliers);
/* The pose order slam_local_ba solves in (host work only, no device call; ctx-free).  The reduced camera system of a window of
 * consecutive key-frames is block-banded in the caller's order (S_pq = 0 for |p - q| > hb) and takes the single-launch banded
 * solver when hb <= 20.  A window that is not -- loop closures: the first and the last key-frames share map points
 * (src/map_manager.jl:300-449 re-associates old map points), so the covisibility chain is a ring -- is solved on relabelled poses when
 * a fold of the ring or a Cuthill-McKee order of the free poses' covisibility graph brings hb <= 20 (constant poses first); theta
 * comes back in the caller's order.  order_out (P entries, may be NULL): the caller's 0-based pose at the solver's position k;
 * hb_out (may be NULL): the half-bandwidth in that order.  Returns 1 if the window is reordered, 0 if the caller's order is kept,
 * < 0 on bad arguments.  (SLAMHIP_BA_NO_REORDER=1 in the environment keeps the caller's order: measurement knob.) */
int    slam_ba_plan_order(int P, int M, int O, const uint8_t *theta_const, const int64_t *pose_ids, const int64_t *point_ids,
                          int32_t *order_out, int *hb_out);
/* Block half-bandwidth of the shard's reduced system (S_pq = 0 for |p - q| > hb).  The all-reduced system has the maximum
 * over the ranks: the driver sets that on every rank before the first solve (single-launch banded solver). */
int    slam_ba_halfband(const slam_ba *ba);
int    slam_ba_set_halfband(slam_ba *ba, int hb);

/* Device-paced LM pass of the sharded path.  Every call below returns after ENQUEUEING on ctx's stream; the accept / reject
 * decision of LeastSquaresOptim's outer loop (bundle_adjustment.jl:35-54) is taken on the device from the
 * gathered trial costs, identically on every rank, so a pass contains no host synchronisation.  Protocol per pass:
 *     slam_ba_lm_begin(ignore, red);  slam_comm_allreduce_sum(red);  slam_ba_lm_start(red, first_pass);
 *     for it = 1 .. iters:
 *         if (it > 1) { slam_ba_lm_build(ignore, red);  slam_comm_allreduce_sum(red); }
 *         slam_ba_lm_solve(red, ignore, trial);  slam_comm_allgather(trial -> gathered, 4);
 *         slam_ba_lm_step(gathered, nranks, it);
 *     slam_ba_lm_state(out8);                       -- the only synchronising call
 * Once the device-side state says "converged" the remaining iterations are no-ops (every kernel early-outs). */
int    slam_ba_lm_begin(slam_ctx *ctx, slam_ba *ba, int ignore_outliers, double *reduce_dev);
int    slam_ba_lm_start(slam_ctx *ctx, slam_ba *ba, const double *reduce_dev, int first_pass);
int    slam_ba_lm_build(slam_ctx *ctx, slam_ba *ba, int ignore_outliers, double *reduce_dev);
int    slam_ba_lm_solve(slam_ctx *ctx, slam_ba *ba, const double *reduce_dev, int ignore_outliers, double *trial_dev);
int    slam_ba_lm_step(slam_ctx *ctx, slam_ba *ba, const double *gathered_dev, int nranks, int iter_tag);
/* synchronises; out8 = {ssr, iterations, converged, delta, chol_fail, ssr at the start of the first pass, trial ssr, max|dx|} */
int    slam_ba_lm_state(slam_ctx *ctx, slam_ba *ba, double *out8);

/* ---- RCCL collectives for the sharded BA ("ncclAllReduce(sum, f64) of [S ; g ; cost] over xGMI") -----------
 * One communicator per process / GPU.  Rank 0 obtains a 128-byte id (slam_comm_unique_id) and hands it to the other
 * ranks through the host's own channel (the Julia side: MPI.jl / Distributed / a file); every rank then calls
 * slam_comm_create.  The collectives are enqueued on ctx's stream (device-ordered with the slam_ba_lm_* calls) and
 * return immediately.  librccl is bound at run time: a process that never creates a communicator does not load it. */
typedef struct slam_comm slam_comm;
int    slam_comm_unique_id(void *id128);
int    slam_comm_create(slam_ctx *ctx, int nranks, int rank, const void *id128, slam_comm **out);
int    slam_comm_destroy(slam_comm *comm);
int    slam_comm_size(const slam_comm *comm);
int    slam_comm_rank(const slam_comm *comm);
/* in-place sum of buf_dev[0 .. count) (Float64) over all ranks */
int    slam_comm_allreduce_sum(slam_ctx *ctx, slam_comm *comm, double *buf_dev, int64_t count);
/* recv_dev[r * count .. (r + 1) * count) = rank r's send_dev[0 .. count) */
int    slam_comm_allgather(slam_ctx *ctx, slam_comm *comm, const double *send_dev, double *recv_dev, int64_t count);

#ifdef __cplusplus
}
#endif
#endif
