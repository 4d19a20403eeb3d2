// kpset.hip -- device-resident keypoint lists for S lock-stepped streams.
//
// In the reference the keypoints of a frame live in a Dict (src/frame.jl) and optical_flow_matching!
// (src/map_manager.jl:451-564) copies them into arrays, tracks, and applies updates / removals one by one; the
// round-1 batch seams kept that list on the HOST and crossed PCIe with it at every call.  Here the list stays in HBM:
// tracking (slam_kpset_flow_match), the removal of lost keypoints, map culling (slam_kpset_remove), the avoidance list
// and the merge of fresh keypoints in key-frame detection (slam_kpset_detect), stereo matching
// (slam_kpset_stereo_match) and triangulation (slam_kpset_triangulate) all read and write the same device arrays; the
// host sees one small copy of the per-stream counts per step (slam_kpset_counts).  Compaction is stable (a stream's
// keypoints keep their order) and is done with wave ballots + prefix counts, one workgroup per stream.
#include "kpset.hpp"
#include <algorithm>
#include "geom_device.hpp"
#include "work_order.hpp"
#include "kf_host.hpp"
#include <cmath>
#include <type_traits>

// The work list (k_kpset_worklist, kpset_kernels.inc): live slots of the streams back to back, each segment in the order of work_order.hpp.
// SLAMHIP_WORK_BAND, read once per process: the band width in pixels, 0 = slot order (the lists as they are); default WORK_BAND_PX.
// KPSET_SORT_LDS_BYTES is the sort's LDS budget (what a workgroup gets without asking for more): a set whose capacity, padded to a
// power of two, does not fit keeps slot order -- slam_kpset_create decides that once (sort_pad).
#define WORK_BAND_PX 16
#define KPSET_SORT_LDS_BYTES 65536
static int work_band() { static const int band = [] { const char *v = getenv("SLAMHIP_WORK_BAND"); const int b = v ? atoi(v) : WORK_BAND_PX; return b < 0 ? 0 : b; }(); return band; }
struct WorkOrder { int H, W, band, pad; };       // band 0: slot order; pad: power of two >= cap whose words fit KPSET_SORT_LDS_BYTES
// SLAMHIP_NO_MATCH_REC=1, read once per process: the matches build no work records and run their record-less prologue (the A/B of round 22)
bool kpset_match_records() { static const bool on = [] { const char *v = getenv("SLAMHIP_NO_MATCH_REC"); return !(v && atoi(v) != 0); }(); return on; }
// the work record of entry idx (work_order.hpp: work_rec_slot) of a list of ceil(ntot / 8) = per entries per XCD: slot q of stream s, target member zt
__device__ __forceinline__ void kp_write_rec(const KpWorkRecs &R, const double *yx, int H, int W, int idx, int per, int q, int s, int zt)
{
    const int at = work_rec_slot(idx, per, R.stride);
    if (at >= WORK_XCDS * R.stride) return;                      // (cannot happen while count <= cap: ntot <= S cap, so per <= stride; it guards the region)
    KpWorkRec r;
    r.py = yx[2 * (size_t)q]; r.px = yx[2 * (size_t)q + 1];
    const bool is3 = R.is3d[q] != 0;
    // the prior is formed for every keypoint and kept for the 3-D ones: under `if (is3)` the loads of the map point and of the parameter slot would wait
    // for the flag -- one more dependent round trip per entry (a 2-D keypoint's xyz holds whatever the slot held: read, computed with, dropped)
    double pry, prx;
    kp_match_prior(R.prior, R.xyz + 3 * (size_t)q, R.par + KP_PAR * (size_t)s, r.py, r.px, pry, prx);
    r.pry = is3 ? pry : r.py; r.prx = is3 ? prx : r.px;
    r.q = q; r.s = s; r.flags = (is3 ? KPREC_3D : 0) | (kp_in_image(r.pry, r.prx, H, W) ? KPREC_INSIDE : 0); r.zt = zt;
    R.rec[at] = r;
}
// k_kpset_worklist, k_kpset_compact and k_kpset_keyframe, plain and selected (slam_kpset_select): kpset_kernels.inc, included once per form
#define SEL_NAME(k) k
#define SEL_ARG
#define SEL_STREAM(b) b
#define SEL_STREAMS(S) S
#define SEL_SELF(s) s
#include "kpset_kernels.inc"
#undef SEL_NAME
#undef SEL_ARG
#undef SEL_STREAM
#undef SEL_STREAMS
#undef SEL_SELF
#define SEL_NAME(k) k##_sel
#define SEL_ARG , const int *sel
#define SEL_STREAM(b) sel[b]
#define SEL_STREAMS(S) (int)gridDim.x
#define SEL_SELF(s) (int)blockIdx.x
#include "kpset_kernels.inc"
#undef SEL_NAME
#undef SEL_ARG
#undef SEL_STREAM
#undef SEL_STREAMS
#undef SEL_SELF

// H x W: the image the positions live in (the match that follows reads its planes); H <= 0: slot order -- the triangulation
// kernels read a few bytes per keypoint and gain nothing from an order
// selected: the caller is one of the six key-frame seams, which honour the set's selection (it has returned already when no stream is selected)
// match: the caller is a match with this prior and these staged parameters -- the entries' work records are written too (unless SLAMHIP_NO_MATCH_REC)
int kpset_build_worklist(slam_ctx *ctx, slam_kpset *ks, int H, int W, bool selected, const KpMatchPrior *match)
{
    WorkOrder O;
    O.H = H; O.W = W; O.pad = ks->sort_pad; O.band = H > 0 && W > 0 && ks->sort_pad > 0 ? work_band() : 0;
    const size_t lds = O.band > 0 ? (size_t)ks->sort_pad * 8 : 0;
    KpWorkRecs R = {nullptr, 0, 0, nullptr, nullptr, nullptr, 0};
    if (match && kpset_match_records()) R = {ks->rec, ks->rec_stride, match->prior, match->par, ks->v.xyz, ks->v.is3d, match->compact ? 1 : 0};
    if (selected && ks->n_sel != KPSEL_ALL)
        hipLaunchKernelGGL(k_kpset_worklist_sel, dim3(ks->n_sel), dim3(256), lds, ctx->stream, (const int *)ks->v.count, ks->S, ks->v.cap, ks->work, ks->ntot, (const double *)ks->v.yx, O, R,
                           (const int *)ks->sel_idx);
    else
        hipLaunchKernelGGL(k_kpset_worklist, dim3(ks->S), dim3(256), lds, ctx->stream, (const int *)ks->v.count, ks->S, ks->v.cap, ks->work, ks->ntot, (const double *)ks->v.yx, O, R);
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

int kpset_stage_params(slam_ctx *ctx, slam_kpset *ks, const double *host, size_t n, const double **dev_out)
{
    const size_t slot_d = (size_t)ks->S * KP_PAR;
    ARG_TRY(ctx, n <= slot_d);
    const int sl = ks->par_slot; ks->par_slot = (sl + 1) & 7;
    HIP_TRY(ctx, hipEventSynchronize(ks->par_ev[sl]));           // the copy that last used this slot (8 calls ago) has long completed
    double *h = ks->par_host + (size_t)sl * slot_d, *dv = ks->par + (size_t)sl * slot_d;
    memcpy(h, host, n * 8);
    HIP_TRY(ctx, hipMemcpyAsync(dv, h, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ks->par_ev[sl], ctx->stream));
    *dev_out = dv;
    return SLAM_OK;
}

int kpset_compact(slam_ctx *ctx, slam_kpset *ks, int mode, const uint8_t *flags_dev, bool selected)
{
    if (selected && ks->n_sel != KPSEL_ALL)
        hipLaunchKernelGGL(k_kpset_compact_sel, dim3(ks->n_sel), dim3(256), 0, ctx->stream, ks->v, mode, flags_dev, (const int *)ks->sel_idx);
    else
        hipLaunchKernelGGL(k_kpset_compact, dim3(ks->S), dim3(256), 0, ctx->stream, ks->v, mode, flags_dev);
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

// Array-level body of triangulate_stereo! (src/mapper.jl:142-183) on the set: every 2-D keypoint with a stereo match is
// triangulated (the DLT of slam_triangulate, same gates); success -> map point Twc[s] * X, is3d = 1; failure -> the stereo
// observation is dropped (remove_stereo_keypoint!).
struct KTriArgs {
    TwoViewMats M;
    const double *Twc;                 // [S][16] column-major camera-1 -> world, device
    double max_error, min_depth;
};
// the two lenses of slam_kpset_triangulate_lens: k1 k2 p1 p2 of camera 1 and of camera 2 (the intrinsics are M.cam1 / M.cam2)
struct KTriLens { double dist1[4], dist2[4]; };
// LENS: the left pixel and the stored stereo pixel are undistorted first, each through its own camera (kp.undistorted_pixel /
// kp.right_undistorted_pixel, mapper.jl:162-177); the DLT and the gates then see the undistorted pair.  <false> never touches Z.
template <bool LENS>
__device__ __forceinline__ void k_kpset_triangulate_slot(const KpsetView &K, const KTriArgs &T, const KTriLens *Z, const int *work, int i)
{
    const size_t q = (size_t)work[i];
    if (!K.stereo[q] || K.is3d[q]) return;
    const int s = (int)(q / K.cap);
    double x1 = K.yx[2 * q + 1], y1 = K.yx[2 * q], x2 = K.syx[2 * q + 1], y2 = K.syx[2 * q];
    if constexpr (LENS) {                                        // (a camera whose four coefficients are zero: the pixel as it is, a copy -- k_kfm_record's rule)
        if (Z->dist1[0] != 0.0 || Z->dist1[1] != 0.0 || Z->dist1[2] != 0.0 || Z->dist1[3] != 0.0) undistort_px(T.M.cam1, Z->dist1, y1, x1, y1, x1);
        if (Z->dist2[0] != 0.0 || Z->dist2[1] != 0.0 || Z->dist2[2] != 0.0 || Z->dist2[3] != 0.0) undistort_px(T.M.cam2, Z->dist2, y2, x2, y2, x2);
    }
    double L[4];
    dlt_two_view(x1, y1, x2, y2, T.M.P1, T.M.P2, L);
    const bool ok = two_view_gates(L, T.M.T21, T.M.cam1, T.M.cam2, x1, y1, x2, y2, T.max_error, T.min_depth, true);
    if (ok) {
        const double *W = T.Twc + 16 * (size_t)s;                // project_camera_to_world (frame.jl): Twc * X
        for (int r = 0; r < 3; r++) K.xyz[3 * q + r] = ((W[r] * L[0] + W[r + 4] * L[1]) + W[r + 8] * L[2]) + W[r + 12] * L[3];
        K.is3d[q] = 1;
    } else K.stereo[q] = 0;
}
// (the grid is sized from the host's bound of the list lengths, which is only a hint: the loop covers every live slot whatever it was)
// One work-list entry per thread and iteration; k_kpset_triangulate_slot reads and writes slot q = work[i] alone (xyz, is3d, stereo
// of q), so any permutation of a stream's segment gives the same lists.
__global__ __launch_bounds__(64) void k_kpset_triangulate(KpsetView K, KTriArgs T, const int *work, const int *ntot)
{
    const int n = ntot[0];
    for (int i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) k_kpset_triangulate_slot<false>(K, T, nullptr, work, i);
}
// the same with a lens on either camera (slam_kpset_triangulate_lens)
__global__ __launch_bounds__(64) void k_kpset_triangulate_lens(KpsetView K, KTriArgs T, KTriLens Z, const int *work, const int *ntot)
{
    const int n = ntot[0];
    for (int i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) k_kpset_triangulate_slot<true>(K, T, &Z, work, i);
}

// Array-level body of triangulate_temporal! (src/mapper.jl:185-262) on the set: every 2-D keypoint whose first observer (the
// key-frame that detected it, observers[1] of its map point) is an earlier key-frame is triangulated from that observation and the
// current one.  The caller supplies, per stream and observer key-frame (slot kf % nkf of `tab`, 64 doubles), what mapper.jl:226-231
// computes once per observer: P2 = K * rel_pose_inv, rel_pose_inv, rel_pose = observer.cw * frame.wc, and observer.wc -- all
// column-major 4 x 4 -- so their arithmetic stays the host's (Manifolds' inv(SE3, .)).  Gates as slam_triangulate's temporal mode:
// a failed gate removes the observation only when the rotation-compensated parallax exceeds min_parallax (20 px), otherwise the
// point is accepted as it is (:244-258).
struct KTempArgs {
    const double *par;        // S x KP_PAR (kpset.hpp)
    const double *tab;        // S x nkf x 64
    const int *kf_cur, *kf_lo; int nkf;
    double max_error, min_depth, min_parallax;
    uint8_t *flags;
};
__device__ __forceinline__ void k_kpset_tri_temporal_slot(const KpsetView &K, const KTempArgs &T, const int *work, int i)
{
    const size_t q = (size_t)work[i];
    if (K.is3d[q] || !K.haskf[q]) return;                        // get_2d_keypoints; keypoints no key-frame has observed yet
    const int s = (int)(q / K.cap), kf = K.fkf[q];
    if (kf == T.kf_cur[s] || kf < T.kf_lo[s]) return;            // :216 the frame itself is the first observer; observer no longer in the table
    const double *par = T.par + KP_PAR * (size_t)s, *cam = par + KP_PAR_CAM, *dist = par + KP_PAR_DIST;
    const double *E = T.tab + ((size_t)s * T.nkf + (kf % T.nkf)) * 64;
    double y1, x1, y2, x2, W[3];
    undistort_px(cam, dist, K.fyx[2 * q], K.fyx[2 * q + 1], y1, x1);  // obup
    undistort_px(cam, dist, K.yx[2 * q], K.yx[2 * q + 1], y2, x2);    // kpup
    if (temporal_pair(cam, E, y1, x1, y2, x2, T.max_error, T.min_depth, T.min_parallax, W)) {     // the parallax, the DLT, the gates (geom_device.hpp)
        for (int r = 0; r < 3; r++) K.xyz[3 * q + r] = W[r];     // project_camera_to_world(observer_kf, .)
        K.is3d[q] = 1;
    } else T.flags[q] = 1;                                        // remove_mappoint_obs!(map_manager, id, frame.kfid)
}
// (the grid is sized from the host's bound of the list lengths, which is only a hint: the loop covers every live slot whatever it was)
// One work-list entry per thread and iteration; k_kpset_tri_temporal_slot writes xyz, is3d and flags of slot q = work[i] alone: the
// order of the work list does not matter here either.
__global__ __launch_bounds__(64) void k_kpset_tri_temporal(KpsetView K, KTempArgs T, const int *work, const int *ntot)
{
    const int n = ntot[0];
    for (int i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) k_kpset_tri_temporal_slot(K, T, work, i);
}

// What check_new_kf_required / check_ready_for_init! (src/front_end.jl:343-393) read of a frame, reduced from the lists: the counts
// (nb_3d_kpts, nb_stereo_kpts, keypoints the previous key-frame observes), nb_occupied_cells (frame.jl:321-337) and compute_parallax
// (front_end.jl:412-452) as mean AND median.  One 256-thread workgroup per stream (stream = blockIdx.x); the lists are only read.
//   cells     a bitmap in LDS over the gr x gc grid (dynamic LDS, one bit per cell), cell = rint(p) / cell_size with the truncating
//             division of SLAM.jl:42-45 (so rint(p) in (-cell_size, 0) is cell 0, as there); a keypoint off the grid -- NaN and
//             +-inf included -- sets no bit (the reference's grid[kpi] would throw)
//   terms     the parallax of every keypoint with haskf (and !is3d under only_2d), compacted in list order (ordered_slot) into LDS
//             while there are at most KF_TERMS_LDS of them, else into the stream's row of A.terms; compensated, the term is the one
//             k_kfive_gather (fivepoint.hip) sums -- same expressions, same order -- so the mean here is the parallax that call returns
//   mean      per lane, butterfly, four waves: k_kfive_gather's order
//   median    Julia's: NaN if any term is NaN, else the middle order statistic(s) by a radix select over the terms' bit patterns
//             (non-negative doubles order as unsigned integers): 8 passes of a 256-bin histogram, most significant byte first
#define KF_TERMS_LDS 4096
static_assert(KF_STATS == SLAM_KF_STATS, "kf_host.hpp and slamhip.h disagree on the record length");
#define KF_BITMAP_LDS_BYTES 16384     /* with the 32 KiB of terms and the histogram: inside the 64 KiB a workgroup gets without asking */
struct KfStatsArgs {
    const double *yx, *kyx; const uint8_t *is3d, *stereo, *haskf; const int *count; int cap;
    const double *par;                 // S x KP_PAR (kpset.hpp), R_compensation in [0..8]
    int flags, cell, gr, gc, words;    // flags: bit 0 compensate_rotation, bit 1 only_2d; words: 32-bit words of the cell bitmap
    unsigned long long *terms;         // S x cap, or nullptr when cap <= KF_TERMS_LDS
    double *out;                       // S x SLAM_KF_STATS
};
// sum of four ints over the 256 threads (s_c: 16 ints); every thread gets the totals
__device__ __forceinline__ void kf_block_sum4(int *v, int *s_c)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 4; k++) v[k] += __shfl_xor(v[k], o, 64);
    __syncthreads();                                             // the previous use of s_c is over
    if (lane == 0) for (int k = 0; k < 4; k++) s_c[4 * wv + k] = v[k];
    __syncthreads();
    for (int k = 0; k < 4; k++) v[k] = (s_c[k] + s_c[4 + k]) + (s_c[8 + k] + s_c[12 + k]);
}
// the element of rank `rank` (0-based, ascending) among T[0 .. m), 0 <= rank < m; k_eq: its rank among the elements equal to it,
// mult: how many of those there are.  s_hist: 256 words, s_w: 4, s_sel: 3.
__device__ __forceinline__ unsigned long long kf_radix_select(const unsigned long long *T, int m, int rank, unsigned *s_hist, int *s_w, int *s_sel,
                                                              int &k_eq, int &mult)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long prefix = 0;
    int k = rank;
    for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);      // the bytes already decided
        s_hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const unsigned long long v = T[i];
            if ((v & himask) == prefix) atomicAdd(&s_hist[(unsigned)(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        const int h = (int)s_hist[tid];
        int incl = h;                                            // inclusive scan of the 256 bins: shuffles inside a wave, one LDS hop across
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        for (int w = 0; w < wv; w++) incl += s_w[w];
        if (incl - h <= k && k < incl) { s_sel[0] = tid; s_sel[1] = k - (incl - h); s_sel[2] = h; }    // one bin holds rank k (k < the bins' total)
        __syncthreads();
        prefix |= (unsigned long long)(unsigned)s_sel[0] << shift; k = s_sel[1]; mult = s_sel[2];
    }
    k_eq = k;
    return prefix;
}
// Julia's median of T[0 .. m), m >= 1, no NaN among the terms: the lower middle by kf_radix_select; for even m the upper middle is the
// same value when its multiplicity reaches past the lower's rank, else the smallest term above it.  Every thread returns the result.
__device__ __forceinline__ double kf_median(const unsigned long long *T, int m, unsigned *s_hist, int *s_w, int *s_sel, unsigned long long *s_min)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int k_eq = 0, mult = 0;
    const unsigned long long lo = kf_radix_select(T, m, (m - 1) >> 1, s_hist, s_w, s_sel, k_eq, mult);
    if (m & 1) return __longlong_as_double((long long)lo);
    unsigned long long hi = lo;
    if (k_eq + 1 >= mult) {                                      // (uniform: k_eq and mult come from LDS)
        unsigned long long mn = ~0ull;
        for (int i = tid; i < m; i += 256) { const unsigned long long v = T[i]; if (v > lo && v < mn) mn = v; }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned ol = __shfl_xor((unsigned)mn, o, 64), oh = __shfl_xor((unsigned)(mn >> 32), o, 64);
            const unsigned long long other = ((unsigned long long)oh << 32) | ol;
            mn = other < mn ? other : mn;
        }
        if (lane == 0) s_min[wv] = mn;
        __syncthreads();
        const unsigned long long a = s_min[0] < s_min[1] ? s_min[0] : s_min[1], c = s_min[2] < s_min[3] ? s_min[2] : s_min[3];
        hi = a < c ? a : c;
    }
    return __longlong_as_double((long long)lo) / 2.0 + __longlong_as_double((long long)hi) / 2.0;      // middle(lo, hi)
}
__global__ __launch_bounds__(256) void k_kpset_frame_stats(KfStatsArgs A)
{
    extern __shared__ unsigned s_bits[];
    __shared__ unsigned long long s_term[KF_TERMS_LDS], s_min[4];
    __shared__ unsigned s_hist[256];
    __shared__ int s_w[4], s_base, s_sel[3], s_c[16];
    __shared__ double s_par[4];
    const int z = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = min(max(A.count[z], 0), A.cap);
    const size_t b = (size_t)z * A.cap;
    const double *par = A.par + KP_PAR * (size_t)z;
    double cam[4], dist[4];
    load_cam(par, cam, dist);
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const bool comp = (A.flags & 1) != 0, only2d = (A.flags & 2) != 0;
    for (int w = tid; w < A.words; w += 256) s_bits[w] = 0;
    if (tid == 0) s_base = 0;
    // pass 1, the flags alone: the counts, and with them where the terms go
    int c[4] = {0, 0, 0, 0};                                     // is3d, stereo, haskf, terms
    for (int j = tid; j < n; j += 256) {
        const bool f3 = A.is3d[b + j] != 0, fk = A.haskf[b + j] != 0;
        c[0] += f3; c[1] += A.stereo[b + j] != 0; c[2] += fk; c[3] += fk && !(only2d && f3);
    }
    kf_block_sum4(c, s_c);                                       // (its barriers also publish the cleared bitmap and s_base)
    const int m = c[3];
    const bool in_lds = m <= KF_TERMS_LDS;
    unsigned long long *gterm = A.terms ? A.terms + b : nullptr; // (dereferenced only when !in_lds: then cap > KF_TERMS_LDS and A.terms is allocated)
    // pass 2: cells and parallax terms
    const double ylim = (double)A.gr * (double)A.cell, xlim = (double)A.gc * (double)A.cell, low = -(double)A.cell;
    double psum = 0.0;
    int isnan_any = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int j = c0 + tid;
        bool take = false;
        double y = 0.0, x = 0.0;
        if (j < n) {
            y = A.yx[2 * (b + j)]; x = A.yx[2 * (b + j) + 1];
            const double ry = rint(y), rx = rint(x);
            if (ry > low && ry < ylim && rx > low && rx < xlim) {            // (false for NaN)
                const int cell = ((int)ry / A.cell) * A.gc + (int)rx / A.cell;
                atomicOr(&s_bits[cell >> 5], 1u << (cell & 31));
            }
            take = A.haskf[b + j] != 0 && !(only2d && A.is3d[b + j] != 0);
        }
        const int pos = ordered_slot(take, s_w, &s_base);
        if (take) {
            const size_t q = b + j;
            double uy, ux, vy, vx, qy, qx, t;
            undistort_px(cam, dist, y, x, uy, ux);
            undistort_px(cam, dist, A.kyx[2 * q], A.kyx[2 * q + 1], vy, vx);
            if (comp) {
                // project(camera, R_compensation * position) - previous undistorted pixel: the term k_kfive_gather (fivepoint.hip) sums
                rotate_project<3>(par, cam, (ux - cx) / fx, (uy - cy) / fy, qy, qx);
                const double dy = qy - vy, dx = qx - vx;
                t = sqrt(dy * dy + dx * dx);
            } else {
                const double dy = uy - vy, dx = ux - vx;
                t = sqrt(dy * dy + dx * dx);
            }
            psum += t;
            isnan_any |= t != t;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(t);
            if (in_lds) s_term[pos] = bits; else gterm[pos] = bits;          // pos < m: <= KF_TERMS_LDS in LDS, <= n <= cap in the stream's row
        }
    }
    for (int o = 32; o > 0; o >>= 1) psum += __shfl_xor(psum, o, 64);
    if (lane == 0) s_par[wv] = psum;
    __threadfence_block();
    const int has_nan = __syncthreads_or(isnan_any);             // terms, bitmap and s_par complete
    int occ[4] = {0, 0, 0, 0};
    for (int w = tid; w < A.words; w += 256) occ[0] += __popc(s_bits[w]);
    kf_block_sum4(occ, s_c);
    double median = 0.0;                                         // :444 without a term
    if (m > 0) {
        if (has_nan) median = __longlong_as_double(0x7FF8000000000000ll);
        else median = in_lds ? kf_median(s_term, m, s_hist, s_w, s_sel, s_min) : kf_median(gterm, m, s_hist, s_w, s_sel, s_min);
    }
    if (tid == 0) {
        double *o = A.out + SLAM_KF_STATS * (size_t)z;
        o[KF_N] = (double)n; o[KF_N3D] = (double)c[0]; o[KF_NSTEREO] = (double)c[1]; o[KF_NHASKF] = (double)c[2]; o[KF_CELLS] = (double)occ[0]; o[KF_NPAR] = (double)m;
        o[KF_MEAN] = m > 0 ? ((s_par[0] + s_par[1]) + (s_par[2] + s_par[3])) / (double)m : 0.0;
        o[KF_MEDIAN] = median;
    }
}

// Every region of the set's one allocation, each named once with its size: called without a block for the total, then with the block
// to bind the pointers.  The order is the allocation's.
static size_t kpset_regions(slam_kpset *ks, char *base)
{
    Layout Lo;
    KpsetView &v = ks->v;
    const size_t S = (size_t)ks->S, n = S * v.cap;
    Lo.bind(v.yx, n * 16, base); Lo.bind(v.oyx, n * 16, base); Lo.bind(v.syx, n * 16, base); Lo.bind(v.xyz, n * 24, base); Lo.bind(v.id, n * 8, base);
    Lo.bind(v.is3d, n, base); Lo.bind(v.stereo, n, base); Lo.bind(v.st, n, base); Lo.bind(v.count, S * 4, base); Lo.bind(ks->work, n * 4, base); Lo.bind(ks->ntot, 64, base);
    Lo.bind(ks->next_id, S * 8, base); Lo.bind(ks->par, 8 * S * KP_PAR * 8, base); Lo.bind(v.kyx, n * 16, base); Lo.bind(v.haskf, n, base); Lo.bind(v.fyx, n * 16, base);
    Lo.bind(v.fkf, n * 4, base); Lo.bind(v.kfcount, S * 4, base);
    Lo.bind(ks->sel_idx, S * 8 + S, base);                               // the selection as one block (one staged copy): S indices, S ranks, the S mask bytes
    if (base) { ks->sel_rank = ks->sel_idx + S; ks->sel_mask = (uint8_t *)(ks->sel_idx + 2 * S); }
    ks->rec_stride = work_rec_stride((long long)n);
    Lo.bind(ks->rec, (size_t)WORK_XCDS * ks->rec_stride * sizeof(KpWorkRec), base);      // the work records of a match (regions start 256-byte aligned)
    return Lo.size();
}

// One body of the three uploads and the three downloads: n keypoints of stream s between each listed array (bytes per keypoint) and
// its host array, skipped where that is null; n == 0 enqueues nothing; `wait`: the seam's wait after the copies.
struct KpField { void *dev; size_t bytes; const void *host; };
static int kpset_copy(slam_ctx *ctx, const slam_kpset *ks, int s, int n, hipMemcpyKind kind, bool wait, std::initializer_list<KpField> fields)
{
    if (n <= 0) return SLAM_OK;
    for (const KpField &f : fields) {
        if (!f.host) continue;
        void *d = (char *)f.dev + (size_t)s * ks->v.cap * f.bytes, *h = const_cast<void *>(f.host);
        HIP_TRY(ctx, hipMemcpyAsync(kind == hipMemcpyHostToDevice ? d : h, kind == hipMemcpyHostToDevice ? h : d, (size_t)n * f.bytes, kind, ctx->stream));
    }
    if (wait) HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    return SLAM_OK;
}
// What every download does first: read count[s] (and kfcount[s] `with_kf`), one wait, *n_out (and *kf_count, where given), the capacity refusal in `who`'s name
static int kpset_download_begin(slam_ctx *ctx, slam_kpset *ks, int s, const char *who, int cap_out, int *n_out, bool with_kf, int *kf_count)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int n = 0, kc = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, ks->v.count + s, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (with_kf) HIP_TRY(ctx, hipMemcpyAsync(&kc, ks->v.kfcount + s, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    *n_out = n; if (kf_count) *kf_count = kc;
    if (n > cap_out) return slam_fail(ctx, SLAM_ERR_CAPACITY, "%s: %d keypoints but cap = %d", who, n, cap_out);
    return SLAM_OK;
}

int kpset_read_back(slam_ctx *ctx, char *h, std::initializer_list<KpReadBack> parts)
{
    for (const KpReadBack &p : parts) HIP_TRY(ctx, hipMemcpyAsync(h + p.at, p.dev, p.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    for (const KpReadBack &p : parts) if (p.out) memcpy(p.out, h + p.at, p.bytes);
    return SLAM_OK;
}

extern "C" {

int slam_kpset_destroy(slam_kpset *ks);

int slam_kpset_create(slam_ctx *ctx, int S, int cap, slam_kpset **out)
{
    ARG_TRY(ctx, ctx != nullptr && out != nullptr && S >= 1 && S <= 128 && cap >= 1 && (size_t)S * cap < (1u << 30));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    slam_kpset *ks = new slam_kpset();
    ks->device = ctx->device; ks->S = S; ks->v.cap = cap;
    const size_t bytes = kpset_regions(ks, nullptr);
    { size_t pad = 1; while (pad < (size_t)cap) pad <<= 1; ks->sort_pad = work_band() > 0 && pad * 8 <= KPSET_SORT_LDS_BYTES ? (int)pad : 0; }
    hipError_t e = hipMalloc((void **)&ks->base, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(ks->base, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = slam_stream_wait(ctx->stream);
    if (e != hipSuccess) { if (ks->base) (void)hipFree(ks->base); delete ks; return slam_fail(ctx, SLAM_ERR_HIP, "slam_kpset_create: %s", hipGetErrorString(e)); }
    kpset_regions(ks, ks->base);
    e = hipHostMalloc((void **)&ks->par_host, (size_t)8 * S * KP_PAR * 8);
    for (int i = 0; i < 8 && e == hipSuccess; i++) { e = hipEventCreateWithFlags(&ks->par_ev[i], hipEventDisableTiming); if (e == hipSuccess) e = hipEventRecord(ks->par_ev[i], ctx->stream); }
    if (e != hipSuccess) { slam_kpset_destroy(ks); return slam_fail(ctx, SLAM_ERR_HIP, "slam_kpset_create: %s", hipGetErrorString(e)); }
    *out = ks;
    return SLAM_OK;
}

int slam_kpset_destroy(slam_kpset *ks)
{
    if (!ks) return SLAM_OK;
    (void)hipSetDevice(ks->device);
    (void)hipDeviceSynchronize();
    if (ks->base) (void)hipFree(ks->base);
    if (ks->par_host) (void)hipHostFree(ks->par_host);
    if (ks->kf_stats) (void)hipFree(ks->kf_stats);
    if (ks->kf_terms) (void)hipFree(ks->kf_terms);
    for (int i = 0; i < 8; i++) if (ks->par_ev[i]) (void)hipEventDestroy(ks->par_ev[i]);
    if (ks->sel_pin) (void)hipHostFree(ks->sel_pin);
    for (int i = 0; i < 8; i++) if (ks->sel_ev[i]) (void)hipEventDestroy(ks->sel_ev[i]);
    delete ks;
    return SLAM_OK;
}

// Test-only (not part of include/slamhip.h): build the work list for an H x W image (H <= 0: slot order) and copy it out --
// work_out S x cap ints (the first *ntot_out are the list), band_out the band width in use (0: slot order for this set).
int slamhip_test_kpset_worklist(slam_ctx *ctx, slam_kpset *ks, int H, int W, int *work_out, int *ntot_out, int *band_out)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && work_out != nullptr && ntot_out != nullptr && band_out != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = kpset_build_worklist(ctx, ks, H, W);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(work_out, ks->work, (size_t)ks->S * ks->v.cap * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ntot_out, ks->ntot, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    *band_out = H > 0 && W > 0 && ks->sort_pad > 0 ? work_band() : 0;
    return SLAM_OK;
}

int slam_kpset_streams(const slam_kpset *ks) { return ks ? ks->S : SLAM_ERR_ARG; }
int slam_kpset_capacity(const slam_kpset *ks) { return ks ? ks->v.cap : SLAM_ERR_ARG; }

// The streams the six key-frame seams act on (kpset_select.hpp makes the table; kpset.hpp says who reads it).  Enqueue-only: the table and
// the normalised mask go through the next slot of a pinned ring (the caller's array is free on return; the wait is for the copy that used
// the slot 8 calls ago) into the set's one device block, in ctx's stream order -- behind every seam enqueued before, ahead of every one after.
int slam_kpset_select(slam_ctx *ctx, slam_kpset *ks, const uint8_t *selected)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr);
    const int S = ks->S;
    int32_t idx[128], rank[128]; uint8_t norm[128];
    const int n_sel = kpset_select_plan(S, selected, idx, norm);
    kpset_select_rank(S, idx, n_sel, rank);
    if (n_sel != KPSEL_ALL) {                                    // (no selection needs no table: the unselected kernel forms read none)
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const size_t bytes = (size_t)S * 9;
        if (!ks->sel_pin) {
            HIP_TRY(ctx, hipHostMalloc((void **)&ks->sel_pin, 8 * bytes));
            for (int i = 0; i < 8; i++) if (!ks->sel_ev[i]) HIP_TRY(ctx, hipEventCreateWithFlags(&ks->sel_ev[i], hipEventDisableTiming));
        }
        const int sl = ks->sel_slot; ks->sel_slot = (sl + 1) & 7;
        HIP_TRY(ctx, hipEventSynchronize(ks->sel_ev[sl]));       // (an event never recorded is complete)
        char *h = ks->sel_pin + (size_t)sl * bytes;
        memcpy(h, idx, (size_t)S * 4); memcpy(h + (size_t)S * 4, rank, (size_t)S * 4); memcpy(h + (size_t)S * 8, norm, (size_t)S);
        HIP_TRY(ctx, hipMemcpyAsync(ks->sel_idx, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ks->sel_ev[sl], ctx->stream));
    }
    memcpy(ks->sel_host, norm, (size_t)S);
    ks->n_sel = n_sel;
    return SLAM_OK;
}
int slam_kpset_selection(const slam_kpset *ks, uint8_t *selected_out)
{
    if (!ks || !selected_out) return SLAM_ERR_ARG;
    for (int s = 0; s < ks->S; s++) selected_out[s] = ks->n_sel == KPSEL_ALL ? 1 : ks->sel_host[s];
    return SLAM_OK;
}

// replace stream s's list (initialisation, tests); ids == NULL: 0 .. n-1, the stream's id counter moves past them
int slam_kpset_upload(slam_ctx *ctx, slam_kpset *ks, int s, const double *yx, const uint8_t *is3d, const double *xyz, const int64_t *ids, int n)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n >= 0 && n <= ks->v.cap && (n == 0 || (yx != nullptr && is3d != nullptr)));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KpsetView &v = ks->v;
    const size_t b = (size_t)s * v.cap;
    std::vector<int64_t> idv((size_t)n);
    int64_t mx = -1;
    for (int i = 0; i < n; i++) { idv[i] = ids ? ids[i] : i; mx = idv[i] > mx ? idv[i] : mx; }
    const int64_t next = mx + 1;
    int rc = kpset_copy(ctx, ks, s, n, hipMemcpyHostToDevice, false, {{v.yx, 16, yx}, {v.is3d, 1, is3d}, {v.xyz, 24, xyz}});
    if (rc) return rc;
    if (n > 0 && !xyz) HIP_TRY(ctx, hipMemsetAsync(v.xyz + 3 * b, 0, (size_t)n * 24, ctx->stream));
    rc = kpset_copy(ctx, ks, s, n, hipMemcpyHostToDevice, false, {{v.id, 8, idv.data()}});
    if (rc) return rc;
    if (n > 0) {
        HIP_TRY(ctx, hipMemsetAsync(v.stereo + b, 0, (size_t)n, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(v.haskf + b, 0, (size_t)n, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(v.count + s, &n, 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ks->next_id + s, &next, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    return SLAM_OK;
}

// read stream s's list back (every output may be NULL); cap_out = capacity of the caller's arrays in keypoints
int slam_kpset_download(slam_ctx *ctx, slam_kpset *ks, int s, double *yx, uint8_t *is3d, double *xyz, int64_t *ids,
                        double *stereo_yx, uint8_t *has_stereo, int cap_out, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n_out != nullptr);
    const int rc = kpset_download_begin(ctx, ks, s, "slam_kpset_download", cap_out, n_out, false, nullptr);
    if (rc) return rc;
    const KpsetView &v = ks->v;
    return kpset_copy(ctx, ks, s, *n_out, hipMemcpyDeviceToHost, true,
                      {{v.yx, 16, yx}, {v.is3d, 1, is3d}, {v.xyz, 24, xyz}, {v.id, 8, ids}, {v.syx, 16, stereo_yx}, {v.stereo, 1, has_stereo}});
}

// create_keyframe! for the lists: k_kpset_keyframe (kpset_kernels.inc), then the streams' key-frame counters
__global__ void k_kpset_kf_advance(int *kfcount, int S) { const int s = blockIdx.x * 64 + threadIdx.x; if (s < S) kfcount[s] += 1; }   // (one 64-thread block until round 5: streams 64.. never advanced)
// only the selected streams' key-frame counters advance: an unselected stream's next key-frame keeps the id it would have had
__global__ void k_kpset_kf_advance_sel(int *kfcount, const int *sel, int n_sel) { const int i = blockIdx.x * 64 + threadIdx.x; if (i < n_sel) kfcount[sel[i]] += 1; }
int slam_kpset_keyframe(slam_ctx *ctx, slam_kpset *ks)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (kpset_none_selected(ks)) return SLAM_OK;
    if (const int *sel = kpset_sel_table(ks)) {
        hipLaunchKernelGGL(k_kpset_keyframe_sel, dim3((ks->v.cap + 255) / 256, ks->n_sel), dim3(256), 0, ctx->stream, ks->v, sel);
        hipLaunchKernelGGL(k_kpset_kf_advance_sel, dim3((ks->n_sel + 63) / 64), dim3(64), 0, ctx->stream, ks->v.kfcount, sel, ks->n_sel);
    } else {
        hipLaunchKernelGGL(k_kpset_keyframe, dim3((ks->v.cap + 255) / 256, ks->S), dim3(256), 0, ctx->stream, ks->v);
        hipLaunchKernelGGL(k_kpset_kf_advance, dim3((ks->S + 63) / 64), dim3(64), 0, ctx->stream, ks->v.kfcount, ks->S);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}
// the key-frame observations of stream s's list, host <-> device (restoring state, tests): kyx n x 2 (y, x), has_kf n flags
int slam_kpset_upload_first(slam_ctx *ctx, slam_kpset *ks, int s, const double *first_yx, const int32_t *first_kf, int n, int kf_count)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n >= 0 && n <= ks->v.cap && (n == 0 || (first_yx != nullptr && first_kf != nullptr)));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = kpset_copy(ctx, ks, s, n, hipMemcpyHostToDevice, false, {{ks->v.fyx, 16, first_yx}, {ks->v.fkf, 4, first_kf}});
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ks->v.kfcount + s, &kf_count, 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    return SLAM_OK;
}
int slam_kpset_download_first(slam_ctx *ctx, slam_kpset *ks, int s, double *first_yx, int32_t *first_kf, int cap_out, int *n_out, int *kf_count)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n_out != nullptr);
    const int rc = kpset_download_begin(ctx, ks, s, "slam_kpset_download_first", cap_out, n_out, true, kf_count);
    if (rc) return rc;
    return kpset_copy(ctx, ks, s, *n_out, hipMemcpyDeviceToHost, true, {{ks->v.fyx, 16, first_yx}, {ks->v.fkf, 4, first_kf}});
}
int slam_kpset_upload_keyframe(slam_ctx *ctx, slam_kpset *ks, int s, const double *kyx, const uint8_t *has_kf, int n)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n >= 0 && n <= ks->v.cap && (n == 0 || (kyx != nullptr && has_kf != nullptr)));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return kpset_copy(ctx, ks, s, n, hipMemcpyHostToDevice, true, {{ks->v.kyx, 16, kyx}, {ks->v.haskf, 1, has_kf}});
}
// the stereo observations of stream s's list, host -> device (restoring state, tests): stereo_yx n x 2 (y, x), has_stereo n flags
int slam_kpset_upload_stereo(slam_ctx *ctx, slam_kpset *ks, int s, const double *stereo_yx, const uint8_t *has_stereo, int n)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n >= 0 && n <= ks->v.cap && (n == 0 || (stereo_yx != nullptr && has_stereo != nullptr)));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return kpset_copy(ctx, ks, s, n, hipMemcpyHostToDevice, true, {{ks->v.syx, 16, stereo_yx}, {ks->v.stereo, 1, has_stereo}});
}
int slam_kpset_download_keyframe(slam_ctx *ctx, slam_kpset *ks, int s, double *kyx, uint8_t *has_kf, int cap_out, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && s >= 0 && s < ks->S && n_out != nullptr);
    const int rc = kpset_download_begin(ctx, ks, s, "slam_kpset_download_keyframe", cap_out, n_out, false, nullptr);
    if (rc) return rc;
    return kpset_copy(ctx, ks, s, *n_out, hipMemcpyDeviceToHost, true, {{ks->v.kyx, 16, kyx}, {ks->v.haskf, 1, has_kf}});
}

// the one small device -> host copy of a step: the S list lengths (synchronises ctx's stream)
int slam_kpset_counts(slam_ctx *ctx, slam_kpset *ks, int32_t *counts)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && counts != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    char *h;
    int rc = slam_pinned(ctx, std::max<size_t>(256, (size_t)ks->S * 4), (void **)&h);
    if (rc) return rc;
    return kpset_read_back(ctx, h, {{0, ks->v.count, (size_t)ks->S * 4, counts}});
}

// remove the keypoints whose flag is set (flags_dev: S x cap bytes in HBM, slot order): map culling, outliers of the pose
// estimators, ... -- stable compaction on the device, returns after enqueueing
int slam_kpset_remove(slam_ctx *ctx, slam_kpset *ks, const uint8_t *flags_dev)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && flags_dev != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return kpset_compact(ctx, ks, 1, flags_dev);
}

// the one body of slam_kpset_triangulate and slam_kpset_triangulate_lens: lens == nullptr launches k_kpset_triangulate, else k_kpset_triangulate_lens
static int kpset_triangulate(slam_ctx *ctx, slam_kpset *ks, const double *P1, const double *P2, const double *T21, const double *cam1, const double *cam2,
                             const KTriLens *lens, const double *Twc, double max_error, double min_depth, int n_bound)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    KTriArgs T;
    T.M.fill(P1, P2, T21, cam1, cam2);
    T.max_error = max_error; T.min_depth = min_depth;
    if (kpset_none_selected(ks)) return SLAM_OK;
    int rc = kpset_stage_params(ctx, ks, Twc, (size_t)ks->S * 16, &T.Twc);      // (an unselected stream's row is staged and never read: no slot of it is in the work list)
    if (rc) return rc;
    rc = kpset_build_worklist(ctx, ks, 0, 0, true);
    if (rc) return rc;
    const int nb = kpset_sel_grid_bound(ks, n_bound);
    if (lens) hipLaunchKernelGGL(k_kpset_triangulate_lens, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, ks->v, T, *lens, (const int *)ks->work, (const int *)ks->ntot);
    else hipLaunchKernelGGL(k_kpset_triangulate, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, ks->v, T, (const int *)ks->work, (const int *)ks->ntot);
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}
int slam_kpset_triangulate(slam_ctx *ctx, slam_kpset *ks, const double *P1, const double *P2, const double *T21,
                           const double *cam1, const double *cam2, const double *Twc, double max_error, double min_depth, int n_bound)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && P1 && P2 && T21 && cam1 && cam2 && Twc);
    return kpset_triangulate(ctx, ks, P1, P2, T21, cam1, cam2, nullptr, Twc, max_error, min_depth, n_bound);
}
// triangulate_stereo! for a rig with lenses: the left pixel through undistort_px(cam1, dist1, .), the stored stereo pixel through
// undistort_px(cam2, dist2, .), then the DLT and both reprojection gates on the undistorted pair (mapper.jl:162-177)
int slam_kpset_triangulate_lens(slam_ctx *ctx, slam_kpset *ks, const double *P1, const double *P2, const double *T21,
                                const double *cam1, const double *cam2, const double *dist1, const double *dist2, const double *Twc,
                                double max_error, double min_depth, int n_bound)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && P1 && P2 && T21 && cam1 && cam2 && dist1 && dist2 && Twc);
    KTriLens Z;
    memcpy(Z.dist1, dist1, sizeof Z.dist1); memcpy(Z.dist2, dist2, sizeof Z.dist2);
    return kpset_triangulate(ctx, ks, P1, P2, T21, cam1, cam2, &Z, Twc, max_error, min_depth, n_bound);
}

int slam_kpset_triangulate_temporal(slam_ctx *ctx, slam_kpset *ks, const double *params, const double *tab, int nkf,
                                    const int32_t *kf_cur, const int32_t *kf_lo, double max_error, double min_depth, double min_parallax,
                                    int n_bound)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && params && tab && kf_cur && kf_lo && nkf >= 1);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (kpset_none_selected(ks)) return SLAM_OK;
    const int S = ks->S;
    const size_t nc = (size_t)S * ks->v.cap;
    Layout D;                          // the staged inputs (same offsets in the pinned block), then the removal flags
    const auto o_tab = D.take<double>((size_t)S * nkf * 64); const auto o_cur = D.take<int>(S), o_lo = D.take<int>(S); const size_t in_b = D.size(); const auto o_fl = D.take<uint8_t>(nc);
    char *scr, *h;
    int rc = slam_scratch2(ctx, D.size(), (void **)&scr);
    if (rc) return rc;
    rc = slam_pinned(ctx, in_b, (void **)&h);
    if (rc) return rc;
    memcpy(o_tab.at(h), tab, o_tab.bytes()); memcpy(o_cur.at(h), kf_cur, o_cur.bytes()); memcpy(o_lo.at(h), kf_lo, o_lo.bytes());
    HIP_TRY(ctx, hipMemcpyAsync(scr, h, in_b, hipMemcpyHostToDevice, ctx->stream));
    KTempArgs T;
    rc = kpset_stage_params(ctx, ks, params, (size_t)S * KP_PAR, &T.par);
    if (rc) return rc;
    T.tab = o_tab.at(scr); T.kf_cur = o_cur.at(scr); T.kf_lo = o_lo.at(scr); T.nkf = nkf;
    T.max_error = max_error; T.min_depth = min_depth; T.min_parallax = min_parallax;
    T.flags = o_fl.at(scr);
    HIP_TRY(ctx, hipMemsetAsync(T.flags, 0, nc, ctx->stream));
    rc = kpset_build_worklist(ctx, ks, 0, 0, true);
    if (rc) return rc;
    const int nb = kpset_sel_grid_bound(ks, n_bound);
    hipLaunchKernelGGL(k_kpset_tri_temporal, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, ks->v, T, (const int *)ks->work, (const int *)ks->ntot);
    HIP_TRY(ctx, hipGetLastError());
    rc = kpset_compact(ctx, ks, 1, T.flags, true);
    if (rc) return rc;
    // the pinned table is read by the copy above: it must be gone from the host block before the next call reuses it
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    return SLAM_OK;
}

// the per-frame statistics of every stream's list (k_kpset_frame_stats); stats == NULL: enqueue only
int slam_kpset_frame_stats(slam_ctx *ctx, slam_kpset *ks, const double *params, int flags, int cell_size, int height, int width,
                           double *stats_dev, double *stats)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && params != nullptr && cell_size > 0 && height > 0 && width > 0 && (flags & ~3) == 0);
    const int S = ks->S;
    KfStatsArgs A;
    A.gr = (int)(((long long)height + cell_size - 1) / cell_size); A.gc = (int)(((long long)width + cell_size - 1) / cell_size);
    const long long cells = (long long)A.gr * A.gc;
    if (cells > 8ll * KF_BITMAP_LDS_BYTES)
        return slam_fail(ctx, SLAM_ERR_ARG, "slam_kpset_frame_stats: %d x %d cells, the kernel's bitmap holds %d", A.gr, A.gc, 8 * KF_BITMAP_LDS_BYTES);
    A.words = (int)((cells + 31) / 32);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ks->kf_stats) HIP_TRY(ctx, hipMalloc((void **)&ks->kf_stats, (size_t)S * SLAM_KF_STATS * 8));
    if (ks->v.cap > KF_TERMS_LDS && !ks->kf_terms) HIP_TRY(ctx, hipMalloc((void **)&ks->kf_terms, (size_t)S * ks->v.cap * 8));
    int rc = kpset_stage_params(ctx, ks, params, (size_t)S * KP_PAR, &A.par);
    if (rc) return rc;
    A.yx = ks->v.yx; A.kyx = ks->v.kyx; A.is3d = ks->v.is3d; A.stereo = ks->v.stereo; A.haskf = ks->v.haskf; A.count = ks->v.count; A.cap = ks->v.cap;
    A.flags = flags; A.cell = cell_size; A.terms = ks->kf_terms; A.out = stats_dev ? stats_dev : ks->kf_stats;
    { ProfScope span(ctx, "kpset_frame_stats");
      hipLaunchKernelGGL(k_kpset_frame_stats, dim3(S), dim3(256), (size_t)A.words * 4, ctx->stream, A); }
    HIP_TRY(ctx, hipGetLastError());
    if (!stats) return SLAM_OK;
    char *h;
    rc = slam_pinned(ctx, std::max<size_t>(256, (size_t)S * SLAM_KF_STATS * 8), (void **)&h);
    if (rc) return rc;
    return kpset_read_back(ctx, h, {{0, A.out, (size_t)S * SLAM_KF_STATS * 8, stats}});
}

// check_new_kf_required for S streams on those statistics (kf_host.hpp): host arithmetic only, no context
int slam_keyframe_required(int S, const double *stats, const int32_t *frames_delta, const int32_t *prev_kf_nb_3d, const uint8_t *has_prev_kf,
                           int max_nb_keypoints, double initial_parallax, int local_ba_on, uint8_t *required, uint8_t *rule)
{
    if (!kf_required(S, stats, frames_delta, prev_kf_nb_3d, has_prev_kf, max_nb_keypoints, initial_parallax, local_ba_on, required, rule))
        return slam_fail(nullptr, SLAM_ERR_ARG, "slam_keyframe_required: S < 1 or a null array");
    return SLAM_OK;
}

}  // extern "C"
