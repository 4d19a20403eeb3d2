// ba_host.hpp -- the host-only half of the local BA set-up (no HIP call, no device needed): structure analysis of a window (pose order, point groups,
// pair lists), the layout of its three arena regions and the staging of its uploads.  Included at the end of ba_device.hpp (it uses slam_ba / BADev).
// Also here: BAKnobs (the planner reads switches too) and the small host helpers slam_local_ba and slam_local_ba_batch share (batch_in, lm_stats, ba_unpermute).
// Definitions: ba_host.hip.  reference: the arrays are those of src/estimator.jl:143-266 (_get_ba_parameters); the planner has no counterpart there.
#pragma once
#include "ba_dev_plan.hpp"
inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
size_t band_lds_bytes(int n, int Ps, int hb);
bool ba_pose_order(int P, int M, int O, const uint8_t *theta_const, const int64_t *pose_ids, const int64_t *point_ids, std::vector<int> &order);
// ---- set-up of one window, in two host-only halves so that a batch of windows can be prepared by several threads:
//   ba_plan   the structure of the problem (map points sorted by first free observer, observation order, point groups or pair lists,
//             pose order) and the layout of its device memory in three regions -- uploaded arrays, zero-initialised state, work arrays;
//   ba_emit   binds the device pointers to the three region bases (ba_bind) and writes the uploaded region into a host staging block (ba_stage).
// slam_local_ba_batch_dev, whose windows lie in HBM, has neither half's analysis: it lays a window out from sizes alone (ba_layout, the tail of ba_plan),
// binds the pointers (ba_bind) and leaves the uploaded region to a device kernel.  What both forms decide alike is ba_dev_plan.hpp's.
// slam_ba_create / slam_local_ba give one window its own arena (the three regions back to back); slam_local_ba_batch lays the
// regions of all windows out region-major (one H2D copy, one memset for the whole batch).  Neither half makes a HIP call.
// fn(0 .. count-1) on the library's parked worker pool, the caller taking part (ba_batch.hip).  A batch prepares one window per task; ONE large window
// (slam_local_ba, BAPlan::nthreads > 1) splits its own passes over the observations instead.  Never called from inside a task of the pool.
void ba_parallel_for(int count, const std::function<void(int)> &fn);
int ba_pool_threads();
// Every SLAMHIP_* switch of the local BA, read once per process at the first ba_knobs() (names, defaults and meanings: scripts/README.md).  getenv occurs
// nowhere else in the local BA; a test that sets a switch does so for a child process.
struct BAKnobs {
    static long long num(const char *v, long long dflt) { return v ? atoll(v) : dflt; }
    // the planner (ba_plan, ba_plan_order)
    bool no_reorder = getenv("SLAMHIP_BA_NO_REORDER") != nullptr;   // (measurement knob) the caller's pose order even where another one is banded
    bool no_groups = getenv("SLAMHIP_NO_GROUPS") != nullptr;        // pair lists instead of point groups
    bool no_dense = getenv("SLAMHIP_NO_DENSE") != nullptr;          // no one-workgroup dense solve (pair lists + tiled Cholesky for windows no order makes banded)
    bool no_bw = getenv("SLAMHIP_NO_BA_WINDOW") != nullptr;         // the launch-per-phase kernels take the small windows of a batch (asked by ba_plan AND by batch_route)
    bool window_sorted = getenv("SLAMHIP_BA_WINDOW_SORTED") != nullptr; // (knob) k_ba_window's map points stay in the order by first free observer
    int sg_points = (int)num(getenv("SLAMHIP_SG_POINTS"), 0);   // <n> (measurement knob): points per group, 0 = ba_plan's own choice
    int threads = (int)num(getenv("SLAMHIP_BA_THREADS"), 0);   // <n>: threads of the worker pool, 0 = hardware threads / 4 between 4 and 32
    // the solve of one window (solve_route)
    bool no_band = getenv("SLAMHIP_NO_BAND") != nullptr;            // the tiled Cholesky instead of the banded solve -- consulted by the single-window path only (see solve_route)
    bool no_twist = getenv("SLAMHIP_NO_TWIST") != nullptr;          // one-sided banded factorisation
    int twist_min = (int)num(getenv("SLAMHIP_TWIST_MIN"), 0);   // <n> (measurement knob): twisted from n free poses, 0 = the measured threshold
    int twist_shift = (int)num(getenv("SLAMHIP_TWIST_SHIFT"), 0);   // <n> (measurement knob): side 0 takes 2 x shift columns more than side 1; +1 paid while the hand-over cost 13 k cycles, with 7 k an even split is 1 % ahead
    bool twist_spread = getenv("SLAMHIP_TWIST_SPREAD") != nullptr;  // (test knob) the two sides on different XCDs
    bool band_trace = getenv("SLAMHIP_BAND_TRACE") != nullptr;      // print k_band_solve's phase clocks (band_trace, ba_single.hip)
    // the batch (batch_route)
    int upload_parts = (int)num(getenv("SLAMHIP_BA_UPLOAD_PARTS"), 4);   // <n> (measurement knob): at most n parts of a large upload, default 4
    bool t512 = getenv("SLAMHIP_BA_BATCH_T512") != nullptr;         // 512-thread point groups even where 256 fit
    bool no_mfma = getenv("SLAMHIP_BA_NO_MFMA") != nullptr;         // the vector Schur build for every window (A/B timing, and the parity reference of the tests)
    bool one_stream = getenv("SLAMHIP_BA_ONE_STREAM") != nullptr;   // (measurement knob) both halves of a batch on one stream
    bool window_one = getenv("SLAMHIP_BA_WINDOW_ONE") != nullptr;   // k_ba_window always on one workgroup per window
    long long xlimit = num(getenv("SLAMHIP_BA_XWAIT_US"), 500000LL) * 100;   // <n> x 100: the bound of k_ba_window's wait for its partner workgroup (default 500 000 us; 0 in the tests = give up at once)
    bool host_times = getenv("SLAMHIP_BA_HOSTTIME") != nullptr;     // print the host-side time split of slam_local_ba / slam_local_ba_batch
};
inline const BAKnobs &ba_knobs() { static const BAKnobs kn; return kn; }
#define BA_PAR_MIN_OBS 32768        // observations per task; windows below 6 such tasks stay on the calling thread (measured: 100 k observations gain nothing from three tasks)
struct BAPlan {
    // inputs
    double fx = 0, fy = 0, cx = 0, cy = 0; int P = 0, M = 0, O = 0;
    const double *theta = nullptr; const uint8_t *theta_const_in = nullptr; const double *pixels_yx = nullptr;
    const int64_t *pose_ids = nullptr, *point_ids = nullptr;
    bool may_reorder = false, small_groups = false, order_only = false;      // order_only: ba_plan stops behind the pose order and the half-bandwidth (ba_plan_order)
    int nthreads = 1;            // > 1: this one window's passes over the observations run on the worker pool (results identical to the serial passes)
    bool window = false;         // result: the window fits k_ba_window (<= 5 consecutive free poses, ...): no point groups are built for it
    int nfree_obs = 0;           // result: observations of free poses
    // results
    slam_ba *ba = nullptr;
    int err = 0; char msg[160] = {0};
    std::vector<int> cnt, pfirst, new_of, pt_id, rank, start, fgrp;
    std::unique_ptr<int[]> ccnt; int nchunk = 1;   // nchunk > 1: observations of point j in chunk t of the caller's list, [t * M + j] (spans -> fill_obs: the stable order without a serial walk)
    int chunks() const { return nthreads > 1 && O >= 6 * BA_PAR_MIN_OBS ? std::min(nthreads, O / BA_PAR_MIN_OBS) : 1; }
    std::vector<uint8_t> const_perm;
    std::vector<int4> grp;
    std::vector<int2> pairs, blk_pq; std::vector<int> blk_start;
    std::vector<int> v_opose, v_opoint, v_opk; std::vector<double> v_pix; bool filled = false;
    const uint8_t *theta_const = nullptr;
    size_t npairs = 0; int nblk = 0, ngrp = 0, wstride = 0, hb = 0, sg_ob = SG_OB, sg_sb = SG_SB;
    int twice_pt = -1, twice_pose = -1;
    // layout: offsets inside the three regions
    size_t o_pose, o_pts, o_const, o_pix, o_opose, o_opoint, o_start, o_ptid, o_opk, o_ohp, o_pfs, o_fobs, o_grp, o_fgrp, o_pairs, o_bs, o_bpq, up_bytes = 0;
    int sg_hp = SG_OB;
    size_t o_st, o_cf, o_outl, o_bwx = 0, zero_bytes = 0;
    int ksplit = 0;
    size_t o_sc0, o_sc1, o_pose_t, o_pts_t, o_hasp, o_f, o_ft, o_Jp, o_Jl, o_Vinv, o_bl, o_T, o_W, o_red, o_Sw, o_dp, o_dl, o_li, o_lf, o_part, o_band, o_wpart, o_xchg, work_bytes = 0;
    ~BAPlan() { delete ba; }
    int lab(int64_t id) const { return new_of.empty() ? (int)id - 1 : new_of[id - 1]; }
    int fail(int code, const char *fmt, long long a = 0, long long b = 0, long long c = 0) { err = code; snprintf(msg, sizeof msg, fmt, a, b, c); return code; }
    // the per-observation arrays (sorted by point): ONE walk over the caller's observations -- the sorted position of observation i is the
    // next free one of its point.  The walk also finds a map point observed twice by one free pose: it has no place in a pose block.
    void fill_obs(int *opose, int *opoint, int *opk, double *pix, int *ohp = nullptr, int *pfs = nullptr, int *fobs = nullptr)
    {
        const int T = nchunk;
        if (T > 1) {
            // chunk t of the caller's list places its observations behind those of the chunks before it: ccnt becomes the first sorted position of
            // (chunk, point) -- the same positions the serial walk hands out
            int *cc = ccnt.get();
            const size_t Ms = (size_t)M;
            ba_parallel_for(T, [&](int c) {
                for (int j = (int)((long long)M * c / T), j1 = (int)((long long)M * (c + 1) / T); j < j1; j++) {
                    int run = start[rank[j]];
                    for (int t = 0; t < T; t++) { const int v = cc[t * Ms + j]; cc[t * Ms + j] = run; run += v; }
                }
            });
            ba_parallel_for(T, [&](int t) {
                int *fill = cc + t * Ms;
                for (int i = (int)((long long)O * t / T), i1 = (int)((long long)O * (t + 1) / T); i < i1; i++) {
                    const int j = (int)point_ids[i] - 1, s = fill[j]++;
                    ba->perm[s] = i;
                    opose[s] = lab(pose_ids[i]); opoint[s] = j; opk[s] = rank[j];
                    pix[s] = pixels_yx[2 * i]; pix[(size_t)O + s] = pixels_yx[2 * i + 1];
                }
            });
            ccnt.reset();
        } else {
            std::vector<int> fill(start.begin(), start.end() - 1);
            for (int i = 0; i < O; i++) {
                const int j = (int)point_ids[i] - 1, k = rank[j], s = fill[k]++;
                ba->perm[s] = i;
                opose[s] = lab(pose_ids[i]); opoint[s] = j; opk[s] = k;
                pix[s] = pixels_yx[2 * i]; pix[(size_t)O + s] = pixels_yx[2 * i + 1];
            }
        }
        // a map point observed twice by one free pose (seen[p]: the last point, by sorted position, free pose p observed): the first such point in sorted order
        std::vector<int> tw_pt(T, -1), tw_pose(T, -1);
        auto twice = [&](int c) {
            std::vector<int> seen((size_t)P, -1);
            for (int k = (int)((long long)M * c / T), k1 = (int)((long long)M * (c + 1) / T); k < k1 && tw_pt[c] < 0; k++)
                for (int a = start[k]; a < start[k + 1]; a++) {
                    const int p = opose[a];
                    if (theta_const[p]) continue;
                    if (seen[p] == k) { tw_pt[c] = pt_id[k]; tw_pose[c] = new_of.empty() ? p : ba->pose_order[p]; break; }
                    seen[p] = k;
                }
        };
        if (T > 1) ba_parallel_for(T, twice); else twice(0);
        for (int c = 0; c < T && twice_pt < 0; c++) if (tw_pt[c] >= 0) { twice_pt = tw_pt[c]; twice_pose = tw_pose[c]; }
        if (pfs) {                                              // running count of free-pose observations by sorted point
            int c = 0;
            for (int k = 0; k < M; k++) { pfs[k] = c; for (int a = start[k]; a < start[k + 1]; a++) if (!theta_const[opose[a]]) { if (fobs) fobs[c] = a; c++; } }
            pfs[M] = c;
        }
        if (ohp) {                                              // index of an observation among its group's observations of free poses
            const int NG = (int)grp.size();
            std::vector<int> mxs(T, 0);
            auto groups = [&](int c) {
                int mx = 0;
                for (int gi = (int)((long long)NG * c / T), g1 = (int)((long long)NG * (c + 1) / T); gi < g1; gi++) {
                    const int4 &G = grp[gi];
                    int n = 0;
                    for (int a = G.y; a < G.y + G.w; a++) ohp[a] = theta_const[opose[a]] ? -1 : n++;
                    mx = std::max(mx, n);
                }
                mxs[c] = mx;
            };
            if (T > 1) ba_parallel_for(T, groups); else groups(0);
            int mx = 0; for (int c = 0; c < T; c++) mx = std::max(mx, mxs[c]);
            if (small_groups) sg_hp = std::max(8, (mx + 1) & ~1);
        }
    }
};
int ba_plan(BAPlan &pl);
void ba_layout(BAPlan &pl);
void ba_bind(BAPlan &pl, char *Aup, char *Azero, char *Awork);
int ba_stage(BAPlan &pl, char *stage);
int ba_emit(BAPlan &pl, char *Aup, char *Azero, char *Awork, char *stage);      // ba_bind, then ba_stage
int ba_plan_order(int P, int M, int O, const uint8_t *theta_const, const int64_t *pose_ids, const int64_t *point_ids, int32_t *order_out, int *hb_out);
// S windows of a batch call: the prefix sums over the caller's concatenated arrays and one BAPlan's inputs per window (slam_local_ba_batch, slam_debug_ba_host_time)
struct BatchIn { std::vector<size_t> th_off, pc_off, ob_off; std::vector<BAPlan> pl; };
inline void batch_in(BatchIn &in, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On, const double *theta, const uint8_t *theta_const,
                     const double *pixels_yx, const int64_t *pose_ids, const int64_t *point_ids)
{
    in.th_off.assign(S + 1, 0); in.pc_off.assign(S + 1, 0); in.ob_off.assign(S + 1, 0); in.pl = std::vector<BAPlan>(S);
    for (int z = 0; z < S; z++) {
        BAPlan &q = in.pl[z];
        const size_t th = in.th_off[z], pc = in.pc_off[z], ob = in.ob_off[z];
        in.th_off[z + 1] = th + 6 * (size_t)Pn[z] + 3 * (size_t)Mn[z]; in.pc_off[z + 1] = pc + Pn[z]; in.ob_off[z + 1] = ob + On[z];
        q.fx = cams[4 * z]; q.fy = cams[4 * z + 1]; q.cx = cams[4 * z + 2]; q.cy = cams[4 * z + 3];
        q.P = Pn[z]; q.M = Mn[z]; q.O = On[z]; q.theta = theta + th; q.theta_const_in = theta_const + pc;
        q.pixels_yx = pixels_yx ? pixels_yx + 2 * ob : nullptr; q.pose_ids = pose_ids ? pose_ids + ob : nullptr; q.point_ids = point_ids ? point_ids + ob : nullptr;
        q.may_reorder = true; q.small_groups = true;
    }
}
// the eight values of `stats` (slam_local_ba and the batch)
inline void lm_stats(const LMState &h, float dev_ms, double *sv) { sv[0] = h.ssr_init; sv[1] = h.ssr_pass1; sv[2] = h.ssr_final; sv[3] = h.iters_pass1; sv[4] = h.iters_pass2; sv[5] = h.n_outliers; sv[6] = dev_ms; sv[7] = h.chol_fail; }
// results in the solver's pose order / sorted observation order -> the caller's arrays (either pair may be absent)
inline void ba_unpermute(const slam_ba *ba, const double *poses, double *theta, const uint8_t *outl, uint8_t *outliers)
{
    if (poses && ba->pose_order.empty()) memcpy(theta, poses, (size_t)ba->d.n * 8);
    else if (poses) for (int k = 0; k < ba->d.P; k++) memcpy(theta + 6 * ba->pose_order[k], poses + 6 * k, 48);
    if (outl) for (int s = 0; s < ba->d.O; s++) outliers[ba->perm[s]] = outl[s];
}
