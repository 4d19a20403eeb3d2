// ba_batch.hip -- bundle_adjustment! for S windows in one set of launches (slam_local_ba_batch, _begin / _end; _dev: the windows resident in HBM, with its probe / stager / results kernels): the window-indexed wrappers of the
// bodies of ba_device.hpp (table of BAWin read through the constant address space: ba_win), among them the matrix-core Schur build, and the host half of the call
// (worker pool, arena layout, retry of k_ba_window on one workgroup).  reference: src/estimator.jl:78-99, :317-347; src/bundle_adjustment.jl:1-111.
#include "ba_device.hpp"

__global__ __launch_bounds__(256) void k_linearize_b(const BAWin *tab, int ignore_outliers, int respect_done)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    if ((int)blockIdx.x >= w.nb_obs) return;
    linearize_body<false>(w.d, ignore_outliers, respect_done);
}
// start of a pass: ssr of the current residuals (k_control mode 0) + the reset of the LM state (k_lm_reset), one launch
__global__ __launch_bounds__(256) void k_pass_start_b(const BAWin *tab, int pass)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    control_body(w.d, 0, w.nb_obs, w.nb_pts, 0, nullptr);
    {   const ParamBufs pb = param_bufs(w.d);                 // the committed poses' sin / cos for the pass's first build (later ones: the accepted trial's, k_trial_poses_b)
        for (int q = threadIdx.x; q < w.d.P; q += 256) pose_sincos(pb.pose + 6 * q, pb.sc + 6 * q); }
    __syncthreads();
    if (threadIdx.x != 0) return;
    LMState *s = w.d.st;
    if (pass == 0) lm_first_pass(s);
    lm_trust_reset(s);
}
template <int TT> __global__ __launch_bounds__(TT) __attribute__((amdgpu_waves_per_eu(4))) void k_schur_groups_b(const BAWin *tab, int ignore_outliers)
{
    const BAWin w = ba_win(tab);
    if (w.pad || w.pad2) return;                             // the window is k_ba_window's / k_schur_groups_m's (pad2: the matrix-core build takes it)
    if ((int)blockIdx.x >= w.d.ngrp) return;
    schur_groups_body<TT>(w.d, 0.0, ignore_outliers, 1);
}
template <int TT> __global__ __launch_bounds__(TT) void k_schur_groups_m(const BAWin *tab, int ignore_outliers)
{
    const BAWin w = ba_win(tab);
    if (w.pad || !w.pad2) return;                            // the window is k_ba_window's / the vector build's
    if ((int)blockIdx.x >= w.d.ngrp) return;
    schur_groups_mfma_body<TT>(w.d, ignore_outliers);
}
__global__ __launch_bounds__(256) void k_schur_reduce_b(const BAWin *tab)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    if ((int)blockIdx.x >= w.n_red) return;
    schur_reduce_body(w.d, 1);
}
__global__ __launch_bounds__(BS_T) void k_band_solve_b(const BAWin *tab)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    band_solve_body(w.d, w.B, 1);
}
// the trial poses' sin / cos, once per window and iteration (one wave; behind k_band_solve_b, ahead of k_update_groups_b)
__global__ __launch_bounds__(64) void k_trial_poses_b(const BAWin *tab)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    const BADev &d = w.d;
    if (d.st->converged) return;
    const ParamBufs pb = param_bufs(d);
    for (int q = threadIdx.x; q < d.P; q += 64) {
        const double tp[3] = {pb.pose[6 * q] - d.dp[6 * q], pb.pose[6 * q + 1] - d.dp[6 * q + 1], pb.pose[6 * q + 2] - d.dp[6 * q + 2]};
        pose_sincos(tp, pb.sc_t + 6 * q);
    }
}
// dynamic LDS: [n] dp, [n] + [n] sin / cos of the trial / committed poses, [cap_ob x 3], [cap_sb x 6], [8] (ug_lds_bytes)
static size_t ug_lds_bytes(int n, int cap_ob, int cap_sb) { return ((size_t)3 * n + (size_t)cap_ob * 3 + (size_t)cap_sb * 6 + 8) * 8; }
template <int TT, bool RECOMP> __global__ __launch_bounds__(TT) void k_update_groups_b(const BAWin *tab, int ignore_outliers, int n_cap, int cap_ob, int cap_sb)
{
    extern __shared__ __attribute__((aligned(16))) double ug_lds[];
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    if ((int)blockIdx.x >= w.d.ngrp || (w.pad2 != 0) != RECOMP) return;      // (a window of the matrix-core build stores nothing of its evaluation: RECOMP forms it again; the others read it back)
    double *s_dp = ug_lds, *s_sct = s_dp + n_cap, *s_sc = s_sct + n_cap, *s_u = s_sc + n_cap, *s_dl = s_u + (size_t)cap_ob * 3, *s_red = s_dl + (size_t)cap_sb * 6;
    update_groups_body<TT, RECOMP>(w.d, ignore_outliers, 1, s_dp, s_u, s_dl, s_red, s_sct, true, s_sc);
}
__global__ __launch_bounds__(256) void k_control_b(const BAWin *tab)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    control_body(w.d, 1, w.d.ngrp, w.d.ngrp, 1 | 2, nullptr);
}
// end of pass 1: record it, flag the outliers at theta_1 (bundle_adjustment.jl:45); the count follows in k_outlier_count_b
__global__ __launch_bounds__(256) void k_outliers_b(const BAWin *tab, double repr_eps, double depth_eps)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    if ((int)blockIdx.x >= w.nb_obs) return;
    outliers_body(w.d, repr_eps, depth_eps);
}
__global__ __launch_bounds__(256) void k_outlier_count_b(const BAWin *tab)
{
    const BAWin w = ba_win(tab);
    if (w.pad) return;                                       // the window is k_ba_window's
    LMState *s = w.d.st;
    if (threadIdx.x == 0) lm_record_pass(s, 1);
    outlier_count_body(w.d, w.nb_obs);
}
// end of pass 2: record it and pack every window's result -- committed parameters (solver's pose order), LM state, outlier flags (sorted
// observation order) -- into one contiguous block for a single device -> host copy.  res: per window [LMState | theta 6P + 3M | outl O]
struct BARes { size_t off_state, off_theta, off_outl; };
__global__ __launch_bounds__(256) void k_results_b(const BAWin *tab, const BARes *rtab, char *res)
{
    const BAWin w = ba_win(tab);
    if (w.pad == 2) return;                                  // rejected at set-up (slam_local_ba_batch reports SLAM_ERR_ARG): nothing to pack
    const BADev &d = w.d;
    LMState *s = d.st;
    const BARes r = rtab[blockIdx.y];
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    const int cur = s->cur;
    const double *pose = cur ? d.pose_t : d.pose, *pts = cur ? d.pts_t : d.pts;
    double *th = (double *)(res + r.off_theta);
    for (int i = tid; i < d.n; i += nth) th[i] = pose[i];
    for (int i = tid; i < 3 * d.M; i += nth) th[d.n + i] = pts[i];
    uint8_t *ol = (uint8_t *)(res + r.off_outl);
    for (int i = tid; i < d.O; i += nth) ol[i] = d.outl[i];
    if (tid == 0) {
        LMState h = *s;
        lm_record_pass(&h, 2);
        *(LMState *)(res + r.off_state) = h;
    }
}

// ---- slam_local_ba_batch_dev: the windows are arrays in HBM (slam_local_ba_batch's layout, observations grouped by point in ascending point id); three
// small kernels take the place of the host's structure analysis, staging and result scatter for the windows k_ba_window solves.  One 256-thread
// workgroup per window each; the decisions they share with the host form are ba_dev_plan.hpp's.
struct BADevArgs { double *theta; const uint8_t *tc; const double *px; const int64_t *pi, *li; uint8_t *outl; };   // the caller's device arrays
struct BADevIn { long long th_off, pc_off, ob_off; int P, M, O, pad; };      // where a window's arrays start in them
struct BADevProbe { int nfree, cmax, nfree_obs, flags; };                    // flags: BAD_UNGROUPED | BAD_TWICE
#define BAD_UNGROUPED 1      // an id out of range, or the point ids do not ascend
#define BAD_TWICE 2          // a map point observed twice by one free pose
// first index of the ascending ids[0 .. n) whose id is not below `id`
__device__ __forceinline__ int bad_lower(const int64_t *ids, int n, int64_t id)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
    return lo;
}
// exclusive scan of v over the 256 threads of the workgroup (every thread calls it); *total = the workgroup's sum.  s_w: 4 ints of LDS
__device__ __forceinline__ int bad_scan256(int v, int *s_w, int *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) { const int o = __shfl_up(inc, dd); if (lane >= dd) inc += o; }
    __syncthreads();                                         // (the sums of the round before are read)
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < wv; q++) base += s_w[q];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return base + inc - v;
}
// Probe: what the host needs to decide a window's route and lay out its arena -- free poses, the largest per-point observation count, the observations of
// free poses -- and the two checks of the contract.  A window whose sizes alone rule k_ba_window out is not looked at (nfree = -1).
__global__ __launch_bounds__(256) void k_ba_dev_probe(const BADevIn *din, BADevArgs a, BADevProbe *out)
{
    __shared__ uint8_t s_tc[BAP_PMAX];
    __shared__ int s_nfree, s_cmax, s_nfo, s_flags, s_twice;      // (s_twice: a word of its own -- s_flags is read for a uniform branch while later waves may already be past it)
    const BADevIn w = din[blockIdx.x];
    const int tid = threadIdx.x, P = w.P, M = w.M, O = w.O;
    if (P > BAP_PMAX || O > BAP_OMAX || O <= 0 || M <= 0) { if (tid == 0) out[blockIdx.x] = BADevProbe{-1, 0, 0, 0}; return; }      // (uniform)
    if (tid == 0) { s_nfree = 0; s_cmax = 0; s_nfo = 0; s_flags = 0; s_twice = 0; }
    if (tid < P) s_tc[tid] = a.tc[w.pc_off + tid];
    __syncthreads();
    if (tid < P && !s_tc[tid]) atomicAdd(&s_nfree, 1);
    const int64_t *pi = a.pi + w.ob_off, *li = a.li + w.ob_off;
    int nfo = 0, bad = 0;
    for (int i = tid; i < O; i += 256) {
        const int64_t p = pi[i], j = li[i];
        if (p < 1 || p > P || j < 1 || j > M || (i > 0 && li[i - 1] > j)) bad = 1;
        else if (!s_tc[p - 1]) nfo++;
    }
    if (bad) atomicOr(&s_flags, BAD_UNGROUPED);
    if (nfo) atomicAdd(&s_nfo, nfo);
    __syncthreads();
    if (s_flags) { if (tid == 0) out[blockIdx.x] = BADevProbe{s_nfree, 0, 0, s_flags}; return; }      // (uniform; below, every id is in range and the ids ascend)
    int cmax = 0, twice = 0;
    for (int j = tid; j < M; j += 256) {
        const int s = bad_lower(li, O, j + 1), e = bad_lower(li, O, j + 2);
        cmax = max(cmax, e - s);
        unsigned long long seen[2] = {0, 0};                 // the free poses that observe point j (P <= 128)
        for (int o = s; o < e; o++) {
            const int p = (int)pi[o] - 1;
            if (s_tc[p]) continue;
            const unsigned long long bit = 1ull << (p & 63);
            if (seen[p >> 6] & bit) twice = 1;
            seen[p >> 6] |= bit;
        }
    }
    atomicMax(&s_cmax, cmax);
    if (twice) atomicOr(&s_twice, BAD_TWICE);
    __syncthreads();
    if (tid == 0) out[blockIdx.x] = BADevProbe{s_nfree, s_cmax, s_nfo, s_twice};
}
// Stager: a window's uploaded region, written in place in exactly the layout ba_stage writes for a `window` plan -- with the caller's point order kept
// (rank[j] = j, pt_id[k] = k; k_ba_window depends on no particular point order) and the poses relabelled by ba_label_free_last: the constant poses first,
// then the free ones, each in the caller's order.  The pointers are those of the window's table entry (ba_bind); the cost split goes into that entry.
__global__ __launch_bounds__(256) void k_ba_dev_stage(BAWin *tab, const BADevIn *din, BADevArgs a)
{
    __shared__ uint8_t s_tc[BAP_PMAX];
    __shared__ int s_lab[BAP_PMAX], s_w[4];
    const BADevIn w = din[blockIdx.x];
    const BADev d = tab[blockIdx.x].d;
    const int tid = threadIdx.x, P = w.P, M = w.M, O = w.O;
    double *pose = d.pose, *pts = d.pts, *pix = (double *)d.pix;
    uint8_t *pconst = (uint8_t *)d.pconst;
    int *opose = (int *)d.opose, *opoint = (int *)d.opoint, *opk = (int *)d.opk, *pt_start = (int *)d.pt_start, *pt_id = (int *)d.pt_id;
    int *pfs = (int *)d.pfs, *fobs = (int *)d.fobs, *fgrp = (int *)d.fgrp, *blk_start = (int *)d.blk_start;
    const double *th = a.theta + w.th_off, *px = a.px + 2 * w.ob_off;
    const int64_t *pi = a.pi + w.ob_off, *li = a.li + w.ob_off;
    if (tid < P) s_tc[tid] = a.tc[w.pc_off + tid];
    __syncthreads();
    if (tid < P) {
        const int lab = ba_label_free_last(s_tc, P, tid);
        s_lab[tid] = lab; pconst[lab] = s_tc[tid];
        for (int c = 0; c < 6; c++) pose[6 * lab + c] = th[6 * tid + c];
    }
    for (int t = tid; t <= P; t += 256) fgrp[t] = 0;
    for (int i = tid; i < 3 * M; i += 256) pts[i] = th[6 * P + i];
    for (int j = tid; j < M; j += 256) pt_id[j] = j;
    __syncthreads();
    for (int i = tid; i < O; i += 256) {
        const int j = (int)li[i] - 1;
        opose[i] = s_lab[pi[i] - 1]; opoint[i] = j; opk[i] = j;
        pix[i] = px[2 * (size_t)i]; pix[(size_t)O + i] = px[2 * (size_t)i + 1];
    }
    // the points in chunks of 256: a point's first observation (the ids ascend: a search), the running count of free-pose observations (a scan with carry)
    int carry = 0;
    for (int c0 = 0; c0 < M; c0 += 256) {
        const int j = c0 + tid;
        int s = 0, e = 0, nf = 0;
        if (j < M) {
            s = bad_lower(li, O, j + 1); e = bad_lower(li, O, j + 2);
            for (int o = s; o < e; o++) nf += s_tc[pi[o] - 1] ? 0 : 1;
        }
        int total;
        const int first = carry + bad_scan256(nf, s_w, &total);
        if (j < M) {
            pt_start[j] = s; pfs[j] = first;
            int r = first;
            for (int o = s; o < e; o++) if (!s_tc[pi[o] - 1]) fobs[r++] = o;
        }
        carry += total;
    }
    if (tid == 0) { pt_start[M] = O; pfs[M] = carry; blk_start[0] = 0; }
    // the cost split: the points before it are those for which ba_ksplit_before holds (each thread reads back what it wrote itself)
    int before = 0;
    const long long cost = ba_ksplit_total(O, carry);
    if (M > 1) for (int j = tid; j < M; j += 256) before += ba_ksplit_before(cost, pt_start[j], pfs[j]) ? 1 : 0;
    int kk;
    (void)bad_scan256(before, s_w, &kk);
    if (tid == 0) tab[blockIdx.x].ksplit = M > 1 ? ba_ksplit_clamp(kk, M) : ba_ksplit_obs(M, O, [&](int k) { return k == 0 ? 0 : O; });
}
// Results, behind k_results_b: a window's committed parameters from the solver's pose order to the caller's, its outlier flags (sorted observation order IS
// the caller's), into the caller's arrays -- where the factorisation held (chol_fail == 0), else the arrays stay as they are.  While the windows run on two
// workgroups each, one whose halves missed each other (chol_fail == 2) means the whole call is solved again FROM THE CALLER'S ARRAYS: nothing is written.
__global__ __launch_bounds__(256) void k_ba_dev_results(const BAWin *tab, const BARes *rtab, const char *res, const BADevIn *din, int nb, int two, BADevArgs a)
{
    __shared__ uint8_t s_tc[BAP_PMAX];
    __shared__ int s_missed;
    const int tid = threadIdx.x;
    if (tid == 0) s_missed = 0;
    __syncthreads();
    if (two) for (int q = tid; q < nb; q += 256) if (((const LMState *)(res + rtab[q].off_state))->chol_fail == 2) s_missed = 1;
    __syncthreads();
    if (s_missed) return;
    const BARes r = rtab[blockIdx.x];
    if (((const LMState *)(res + r.off_state))->chol_fail) return;
    const BADevIn w = din[blockIdx.x];
    const int P = w.P, M = w.M, O = w.O;
    if (tid < P) s_tc[tid] = a.tc[w.pc_off + tid];
    __syncthreads();
    const double *src = (const double *)(res + r.off_theta);
    double *th = a.theta + w.th_off;
    if (tid < P) {
        const int lab = ba_label_free_last(s_tc, P, tid);
        for (int c = 0; c < 6; c++) th[6 * tid + c] = src[6 * lab + c];
    }
    for (int i = tid; i < 3 * M; i += 256) th[6 * P + i] = src[6 * P + i];
    const uint8_t *ol = (const uint8_t *)(res + r.off_outl);
    for (int i = tid; i < O; i += 256) a.outl[w.ob_off + i] = ol[i];
}



// Worker threads for the host half of a batch (structure analysis, staging, result scatter of S windows): created once, parked on a
// condition variable between calls -- starting 15 threads per phase cost more than the work they did (128 windows: 2.3 ms of a 6.3 ms
// call).  Callers from several contexts take turns (run_mu).  Windows are handed out one at a time from an atomic counter.
namespace {
// A run hands out task indices from one atomic word tagged with the run's generation, so that a worker only ever executes a task with the function of
// the run the index belongs to; only as many workers are woken as there are tasks beside the caller's (a one-window set-up of four tasks does not
// wake and collect 31 threads), and a worker that wakes late finds nothing to claim and goes back to sleep.
struct BAPool {
    std::vector<std::thread> th;
    std::mutex mu, run_mu;
    std::condition_variable cv, cv_done;
    const std::function<void(int)> *fn = nullptr;
    int n = 0; unsigned gen = 0; bool stop = false;
    std::atomic<unsigned long long> next{0};      // generation << 32 | next task index
    std::atomic<int> done{0};
    // claims are one fetch_add each (no retry under contention).  A worker that read run g's function and then draws an index of a LATER run g' (it was
    // late: run g is over) owns that task of run g' -- which therefore cannot have completed -- and reads g's successor under the mutex before executing it.
    void take(const std::function<void(int)> *f, int count, unsigned g)
    {
        for (;;) {
            const unsigned long long cur = next.fetch_add(1, std::memory_order_acq_rel);
            if ((unsigned)(cur >> 32) != g) { std::lock_guard<std::mutex> lk(mu); f = fn; count = n; g = gen; if ((unsigned)(cur >> 32) != g) return; }
            if ((int)(unsigned)cur >= count) return;
            (*f)((int)(unsigned)cur);
            if (done.fetch_add(1, std::memory_order_acq_rel) + 1 == count) { std::lock_guard<std::mutex> lk(mu); cv_done.notify_one(); }
        }
    }
    explicit BAPool(int workers)
    {
        for (int t = 0; t < workers; t++)
            th.emplace_back([this] {
                unsigned seen = 0;
                for (;;) {
                    const std::function<void(int)> *f; int count;
                    { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return stop || gen != seen; }); if (stop) return; seen = gen; f = fn; count = n; }
                    take(f, count, seen);
                }
            });
    }
    ~BAPool() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (auto &x : th) x.join(); }
    void run(int count, const std::function<void(int)> &f)
    {
        std::lock_guard<std::mutex> turn(run_mu);
        if (th.empty() || count <= 1) { for (int z = 0; z < count; z++) f(z); return; }
        unsigned g;
        { std::lock_guard<std::mutex> lk(mu); fn = &f; n = count; g = ++gen; done.store(0, std::memory_order_relaxed); next.store((unsigned long long)g << 32, std::memory_order_release); }
        if (count - 1 >= (int)th.size()) cv.notify_all(); else for (int k = 0; k < count - 1; k++) cv.notify_one();
        take(&f, count, g);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return done.load(std::memory_order_acquire) >= count; });
    }
};
std::atomic<long> n_xretry{0};       // calls that were solved again on one workgroup per window (slam_debug_ba_xretries)
BAPool &ba_pool()
{
    const int hw = (int)std::thread::hardware_concurrency(), env_threads = ba_knobs().threads;
    static BAPool pool(std::max(0, (env_threads > 0 ? env_threads : std::min(std::max(hw / 4, 4), 32)) - 1));
    return pool;
}
}  // namespace
void ba_parallel_for(int count, const std::function<void(int)> &fn) { ba_pool().run(count, fn); }
int ba_pool_threads() { return (int)ba_pool().th.size() + 1; }

// ---- slam_local_ba_batch in steps over one plain state struct: batch_arena -> batch_stage -> batch_route -> batch_enqueue -> batch_scatter
namespace {
struct BatchCall {
    slam_ctx *ctx = nullptr; int S = 0, NB = 0;
    BatchIn in;                                    // prefix sums over the caller's arrays + the plans of all S windows
    std::vector<int> st_code, batch, single;      // [S] per-window code; the windows the batch kernels take (batch_takes); those solved one by one afterwards
    std::vector<SolveRoute> route;                // [S] the batch's solve route of a window
    // region-major arena: [window table | result table | list of k_ba_window's windows | uploads of every window][zero regions][work regions][results]
    std::vector<size_t> up, ze, wk, rs;           // [NB + 1] prefix sums of the four regions
    size_t tab_bytes = 0, rtab_bytes = 0, up_total = 0, zero_base = 0, work_base = 0, res_base = 0, total = 0;
    char *A = nullptr, *stage = nullptr, *res_host = nullptr; BAWin *tab_h = nullptr; BARes *rtab_h = nullptr;
    int n_early = 0; bool early_sent = false;     // windows whose staged bytes leave before the launch sequence: all but the last part of a large upload
    float dev_ms = 0;
    BAPlan &plan(int k) { return in.pl[batch[k]]; }
    size_t list_off() const { return tab_bytes + rtab_bytes - al((size_t)NB * 4); }      // (the list travels behind the result table in the same upload)
    const LMState &state(int k) const { return *(const LMState *)(res_host + (rtab_h[k].off_state - res_base)); }
};
// Every launch size of the batch, decided once from the staged table.
struct BatchRoute {
    // windows one workgroup can keep to itself (k_ba_window: <= 5 free poses, consecutive; BAWin::pad = 1); the others take the launch-per-phase kernels
    std::vector<int> small_list; int NS = 0; size_t lds_bw = 0;
    bool all_small = false;
    int gx_obs = 1, gx_grp = 1, gx_red = 1;        // grid x extents: the largest launch-per-phase window's
    // small groups everywhere (the reference's window shape: 16 points x 10 observers): 256-thread workgroups, two to three per compute unit
    int TT = SG_T; size_t lds_sg = 0, lds_band = 0;
    void (*build_vec)(const BAWin *, int) = nullptr; void (*update_vec)(const BAWin *, int, int, int, int) = nullptr;      // k_schur_groups_b / k_update_groups_b<., false> at TT threads
    int ug_n = 6, ug_ob = 8, ug_sb = 8; size_t lds_ug = 0;      // k_update_groups_b's LDS arrays at the batch's own sizes
    // the Schur products on the matrix cores (k_schur_groups_m, BAWin::pad2 = 1): 256-thread groups whose matrix Y (3 x points columns, 6 x window slots rows) fits
    // LDS beside two more workgroups.  Per window: one whose Y does not fit (a wide band with few observations per point) does not take the matrix cores from the
    // others.  The vector kernel's lds_sg and the cost-only linearisation are shared: the vector build stores its own evaluation, the matrix-core build none
    int n_mfma = 0, n_vec = 0; size_t lds_m = 0;
    // A batch of >= 32 windows runs its launch-per-phase kernels as TWO halves on two streams: while one half sits in its latency-bound kernels (k_band_solve_b:
    // one workgroup per window, k_trial_poses_b, k_control_b -- ~75 us of an iteration) the other half's builds fill the chip
    bool two_streams = false;
    // two workgroups per window (k_ba_window) only while BOTH halves of EVERY window are resident at once -- they wait for each other: one
    // workgroup per compute unit (136-148 KB of LDS), so 2 x NS workgroups must fit the device's compute units (hipDeviceProp_t, not a
    // constant), the stream must not be CU-masked (a mask says nothing about how many of an XCD's units are left, and the halves b / b + 8
    // need two on the SAME XCD) and the architecture must be the one the memory-side hand-over was validated on (ctx->xwg_ok).  Other
    // processes' kernels can still hold LDS the count knows nothing about: the kernel's wait is bounded (BAKnobs::xlimit) and a window whose halves
    // missed each other comes back with chol_fail = 2 -- the call is then solved again with one workgroup per window (batch_enqueue).
    int two = 0, two_grid = 0;
};

int batch_arena(BatchCall &c)
{
    const int NB = c.NB;
    c.up.resize(NB + 1); c.ze.resize(NB + 1); c.wk.resize(NB + 1); c.rs.resize(NB + 1);
    c.tab_bytes = al((size_t)NB * sizeof(BAWin)); c.rtab_bytes = al((size_t)NB * sizeof(BARes)) + al((size_t)NB * 4);   // (+ the list of k_ba_window's windows)
    c.up[0] = c.tab_bytes + c.rtab_bytes; c.ze[0] = 0; c.wk[0] = 0; c.rs[0] = 0;
    for (int k = 0; k < NB; k++) {
        const BAPlan &q = c.plan(k);
        c.up[k + 1] = c.up[k] + q.up_bytes; c.ze[k + 1] = c.ze[k] + q.zero_bytes; c.wk[k + 1] = c.wk[k] + q.work_bytes;
        c.rs[k + 1] = c.rs[k] + al(sizeof(LMState)) + al((6 * (size_t)q.P + 3 * (size_t)q.M) * 8 + 8) + al((size_t)q.O + 8);
    }
    c.up_total = c.up[NB]; c.zero_base = c.up_total; c.work_base = c.zero_base + c.ze[NB]; c.res_base = c.work_base + c.wk[NB]; c.total = c.res_base + c.rs[NB];
    if (const int rc = slam_scratch(c.ctx, c.total, (void **)&c.A)) return rc;
    if (const int rc = slam_pinned(c.ctx, c.up_total + c.rs[NB], (void **)&c.stage)) return rc;
    c.res_host = c.stage + c.up_total; c.tab_h = (BAWin *)c.stage; c.rtab_h = (BARes *)(c.stage + c.tab_bytes);
    return SLAM_OK;
}
// window k's entry of the window table, once its pointers are bound (ba_bind); ksplit: the plan's, by observation counts
void win_table(BatchCall &c, int k, char *zero)
{
    BAPlan &q = c.plan(k);
    BAWin &w = c.tab_h[k];
    slam_ba *b = q.ba; b->device = c.ctx->device; b->owns_arena = false; b->arena = c.A;
    w.d = b->d;
    w.B = band_args(b, c.route[c.batch[k]], b->reduce, 0.0); w.B.epoch = 1;
    w.nb_obs = b->nblocks_obs; w.nb_pts = b->nblocks_pts; w.n_red = (w.d.P * (w.d.whb + 1) * 36 + w.d.P * 12 + 255) / 256;
    w.ksplit = q.ksplit; w.bwx = q.window ? (double *)(zero + q.o_bwx) : nullptr;
}
// stage window k of the batch: its uploaded region, its table entries
void emit_window(BatchCall &c, int k)
{
    BAPlan &q = c.plan(k);
    BAWin &w = c.tab_h[k];
    memset(&w, 0, sizeof w);
    BARes &r = c.rtab_h[k];
    r.off_state = c.res_base + c.rs[k]; r.off_theta = r.off_state + al(sizeof(LMState)); r.off_outl = r.off_theta + al((6 * (size_t)q.P + 3 * (size_t)q.M) * 8 + 8);
    char *zero = c.A + c.zero_base + c.ze[k];
    // Kept exactly as found: a window whose set-up fails in ba_emit (q.err: a point observed twice by one pose) stays in the table with pad = 2 -- every batch kernel,
    // k_results_b included, returns at once for it, it is in no list of k_ba_window's and its (zeroed) table entry is never read for a launch size
    if (ba_emit(q, c.A + c.up[k], zero, c.A + c.work_base + c.wk[k], c.stage + c.up[k])) { w.pad = 2; return; }
    win_table(c, k, zero);
    if (q.window && q.M > 1) {
        // the split point of k_ba_window's two workgroups: an observation costs the evaluation phases ~24 cycles, an observation of a FREE
        // pose ~6.5 times that in the Schur phase (phase clocks, BW_TRACE) -- and those sit at one end of the sorted points: split by cost (ba_dev_plan.hpp)
        const int *pfs = (const int *)(c.stage + c.up[k] + q.o_pfs);
        w.ksplit = ba_ksplit_cost(q.M, q.O, [&](int kk) { return q.start[kk]; }, [&](int kk) { return pfs[kk]; });
    }
}
// a large upload travels in parts: the staged bytes of the first windows go out while the pool stages the next ones (128 x P20: 203 MB = 4 ms of PCIe
// beside 2.5 ms of staging); the tables and the last part follow with the launch sequence (batch_enqueue)
// (a part keeps every thread of the pool busy -- one window per task -- and a small upload is not worth the extra runs of the pool: measured, 128 reference-shaped
//  windows = 33 MB gained 0.2 ms per call and lost 25 % with two calls in flight; 32 x P100 in four parts of eight windows lost 4 ms)
int batch_stage(BatchCall &c, BAPool &pool, const int32_t *status)
{
    const int NB = c.NB, nthr = (int)pool.th.size() + 1;
    const int n_parts = c.up_total < ((size_t)64 << 20) ? 1 : std::max(1, std::min(ba_knobs().upload_parts, NB / std::max(nthr, 1)));
    c.n_early = n_parts > 1 ? NB - (NB + n_parts - 1) / n_parts : 0;
    const int early_step = n_parts > 1 ? std::max(1, (c.n_early + n_parts - 2) / (n_parts - 1)) : NB;
    c.early_sent = c.n_early > 0;
    for (int b0 = 0; c.n_early > 0 && b0 < NB;) {
        const int b1 = b0 < c.n_early ? std::min(c.n_early, b0 + early_step) : NB;
        pool.run(b1 - b0, [&](int zz) { emit_window(c, b0 + zz); });
        if (b1 <= c.n_early && c.early_sent) c.early_sent = hipMemcpyAsync(c.A + c.up[b0], c.stage + c.up[b0], c.up[b1] - c.up[b0], hipMemcpyHostToDevice, c.ctx->stream) == hipSuccess;
        b0 = b1;
    }
    // (kept as found: S pool tasks for NB <= S windows -- the pool wakes its workers by the task count)
    if (c.n_early == 0) pool.run(c.S, [&](int zz) { if (zz < NB) emit_window(c, zz); });
    for (int k = 0; k < NB; k++) {
        const BAPlan &q = c.plan(k);
        if (q.err) { c.st_code[c.batch[k]] = q.err; if (!status) return slam_fail(c.ctx, q.err, "slam_local_ba_batch: window %d: %s", c.batch[k], q.msg); }
    }
    return SLAM_OK;
}
// One pass over the staged table marks k_ba_window's windows (pad = 1) and takes the maxima of the others (pad == 0: neither k_ba_window's nor rejected at set-up);
// TT is a property of the whole batch, so what depends on it -- lds_sg and each window's pad2 -- follows in a second, short loop over the same windows.
BatchRoute batch_route(BatchCall &c)
{
    const BAKnobs &kn = ba_knobs();
    const int NB = c.NB;
    BatchRoute r;
    int max_ob = 0, max_hb = 0;
    for (int k = 0; k < NB; k++) {
        BAWin &w = c.tab_h[k];
        if (!kn.no_bw && !w.pad && c.plan(k).window) { r.small_list.push_back(k); r.lds_bw = std::max(r.lds_bw, bw_lds_bytes(c.plan(k).P)); w.pad = 1; }
        if (w.pad) continue;
        const BADev &d = w.d;
        r.gx_obs = std::max(r.gx_obs, w.nb_obs); r.gx_grp = std::max(r.gx_grp, d.ngrp); r.gx_red = std::max(r.gx_red, w.n_red);
        max_ob = std::max(max_ob, d.sg_ob); max_hb = std::max(max_hb, d.whb);
        r.lds_band = std::max(r.lds_band, (size_t)w.B.lds_bytes);
        r.ug_n = std::max(r.ug_n, d.n); r.ug_ob = std::max(r.ug_ob, d.sg_ob); r.ug_sb = std::max(r.ug_sb, d.sg_sb);
    }
    r.NS = (int)r.small_list.size(); r.all_small = r.NS == NB;
    std::copy(r.small_list.begin(), r.small_list.end(), (int *)(c.stage + c.list_off()));
    r.TT = (!kn.t512 && max_ob <= 256 && (max_hb + 1) * (max_hb + 2) / 2 <= 256) ? 256 : SG_T;
    r.build_vec = r.TT == 256 ? k_schur_groups_b<256> : k_schur_groups_b<SG_T>; r.update_vec = r.TT == 256 ? k_update_groups_b<256, false> : k_update_groups_b<SG_T, false>;
    r.lds_ug = ug_lds_bytes(r.ug_n, r.ug_ob, r.ug_sb);
    for (int k = 0; k < NB; k++) {
        BAWin &w = c.tab_h[k];
        if (w.pad) continue;
        const BADev &d = w.d;
        r.lds_sg = std::max(r.lds_sg, sg_lds_bytes(d.whb, d.P, d.sg_ob, d.sg_sb, r.TT, d.sg_hp));
        const size_t b = sgm_lds_bytes(d.whb, d.P, d.sg_ob, d.sg_sb, d.sg_hp);
        w.pad2 = !kn.no_mfma && r.TT == 256 && b <= 64 * 1024;
        if (w.pad2) { r.lds_m = std::max(r.lds_m, b); r.n_mfma++; } else r.n_vec++;
    }
    r.two_streams = !r.all_small && NB >= 32 && !kn.one_stream;
    r.two_grid = 16 * ((r.NS + 7) / 8);
    r.two = (!kn.window_one && c.ctx->xwg_ok && r.two_grid <= c.ctx->dev_cus) ? 1 : 0;
    return r;
}

// the launch-per-phase windows [n0, n0 + nb) on stream q: one pass (the group build and the group update: the matrix-core kernels for the windows with pad2, the
// route's vector kernels for the others), then both
void run_pass(const BatchRoute &r, hipStream_t q, const BAWin *tb, int nb, int ignore, int iters)
{
    hipLaunchKernelGGL(k_linearize_b, dim3(r.gx_obs, nb), dim3(256), 0, q, tb, ignore, 0);
    hipLaunchKernelGGL(k_pass_start_b, dim3(1, nb), dim3(256), 0, q, tb, ignore ? 1 : 0);
    for (int it = 1; it <= iters; it++) {
        if (r.n_mfma) hipLaunchKernelGGL(k_schur_groups_m<256>, dim3(r.gx_grp, nb), dim3(256), r.lds_m, q, tb, ignore);
        if (r.n_vec) hipLaunchKernelGGL(r.build_vec, dim3(r.gx_grp, nb), dim3(r.TT), r.lds_sg, q, tb, ignore);
        hipLaunchKernelGGL(k_schur_reduce_b, dim3(r.gx_red, nb), dim3(256), 0, q, tb);
        hipLaunchKernelGGL(k_band_solve_b, dim3(1, nb), dim3(BS_T), r.lds_band, q, tb);
        hipLaunchKernelGGL(k_trial_poses_b, dim3(1, nb), dim3(64), 0, q, tb);
        if (r.n_mfma) hipLaunchKernelGGL((k_update_groups_b<256, true>), dim3(r.gx_grp, nb), dim3(256), r.lds_ug, q, tb, ignore, r.ug_n, r.ug_ob, r.ug_sb);
        if (r.n_vec) hipLaunchKernelGGL(r.update_vec, dim3(r.gx_grp, nb), dim3(r.TT), r.lds_ug, q, tb, ignore, r.ug_n, r.ug_ob, r.ug_sb);
        hipLaunchKernelGGL(k_control_b, dim3(1, nb), dim3(256), 0, q, tb);
    }
}
void both_passes(const BatchRoute &r, hipStream_t q, const BAWin *tb, int nb, int iters_fast, int iterations, double repr_eps)
{
    run_pass(r, q, tb, nb, 0, iters_fast);
    hipLaunchKernelGGL(k_outliers_b, dim3(r.gx_obs, nb), dim3(256), 0, q, tb, repr_eps, 1e-6);
    hipLaunchKernelGGL(k_outlier_count_b, dim3(1, nb), dim3(256), 0, q, tb);
    run_pass(r, q, tb, nb, 1, iterations);
}
// k_ba_window over the route's list of windows, on one or two workgroups each (both forms of the batch launch it here); its LDS limit once per device
int window_attr(BatchCall &c, const BatchRoute &r)
{
    static std::atomic<bool> bw_attr[64];
    return r.NS > 0 ? LDS_ATTR_ONCE(c.ctx, bw_attr, k_ba_window, bw_lds_bytes(BW_PMAX)) : SLAM_OK;
}
void launch_window(BatchCall &c, const BatchRoute &r, int iters_fast, int iterations, double repr_eps)
{
    if (r.NS > 0) hipLaunchKernelGGL(k_ba_window, dim3(r.two ? r.two_grid : r.NS), dim3(BW_T), r.lds_bw, c.ctx->stream, (const BAWin *)c.A, (const int *)(c.A + c.list_off()), r.NS, r.two, iters_fast, iterations, repr_eps, 1e-6, ba_knobs().xlimit);
}
// upload, memset, k_ba_window, the one or two halves, k_results_b, download; a second attempt with one workgroup per window if two halves missed each other
int batch_enqueue(BatchCall &c, BatchRoute &r, int iters_fast, int iterations, double repr_eps)
{
    slam_ctx *ctx = c.ctx;
    const int NB = c.NB;
    char *A = c.A;
    hipStream_t st = ctx->stream;
    static std::atomic<bool> attr_set[7][64];
    const size_t sg_max = sg_lds_bytes(BS_MAXHB, SOLVE_MAX_N / 6);
    int rc = LDS_ATTR_ONCE(ctx, attr_set[0], k_schur_groups_b<SG_T>, sg_max);
    if (!rc) rc = LDS_ATTR_ONCE(ctx, attr_set[1], k_schur_groups_b<256>, sg_max);
    if (!rc) rc = LDS_ATTR_ONCE(ctx, attr_set[2], k_band_solve_b, 150 * 1024);
    if (!rc) rc = LDS_ATTR_ONCE(ctx, attr_set[3], k_schur_groups_m<256>, 64 * 1024);
    if (!rc) rc = LDS_ATTR_ONCE(ctx, attr_set[4], (k_update_groups_b<256, true>), 64 * 1024);
    if (!rc) rc = LDS_ATTR_ONCE(ctx, attr_set[5], (k_update_groups_b<256, false>), 64 * 1024);
    if (!rc) rc = LDS_ATTR_ONCE(ctx, attr_set[6], (k_update_groups_b<SG_T, false>), 64 * 1024);
    if (rc) return rc;
    const BAWin *tab = (const BAWin *)A; const BARes *rtab = (const BARes *)(A + c.tab_bytes);
    hipStream_t st2 = r.two_streams ? ctx_aux_stream(ctx) : nullptr;
    if ((rc = window_attr(c, r)) != SLAM_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    for (int attempt = 0; e == hipSuccess && attempt < 2; attempt++) {
        if (attempt == 0 && c.early_sent) {                    // (the first parts of the windows' bytes are on their way already)
            e = hipMemcpyAsync(A, c.stage, c.up[0], hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(A + c.up[c.n_early], c.stage + c.up[c.n_early], c.up_total - c.up[c.n_early], hipMemcpyHostToDevice, st);
        } else e = hipMemcpyAsync(A, c.stage, c.up_total, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(A + c.zero_base, 0, c.ze[NB], st);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e0, st);
        launch_window(c, r, iters_fast, iterations, repr_eps);
        if (!r.all_small && st2) {
            const int nA = NB / 2;
            (void)hipEventRecord(ctx->fork_ev, st); (void)hipStreamWaitEvent(st2, ctx->fork_ev, 0);
            both_passes(r, st2, tab + nA, NB - nA, iters_fast, iterations, repr_eps);
            both_passes(r, st, tab, nA, iters_fast, iterations, repr_eps);
            (void)hipEventRecord(ctx->join_ev, st2); (void)hipStreamWaitEvent(st, ctx->join_ev, 0);
        } else if (!r.all_small) both_passes(r, st, tab, NB, iters_fast, iterations, repr_eps);
        hipLaunchKernelGGL(k_results_b, dim3(8, NB), dim3(256), 0, st, tab, rtab, A);
        e = hipGetLastError();
        (void)hipEventRecord(e1, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c.res_host, A + c.res_base, c.rs[NB], hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = slam_stream_wait(st);
        if (e == hipSuccess) (void)hipEventElapsedTime(&c.dev_ms, e0, e1);
        if (e != hipSuccess || !r.two) break;
        bool missed = false;                                   // did the halves of some window miss each other?
        for (int k : r.small_list) if (c.state(k).chol_fail == 2) { missed = true; break; }
        if (!missed) break;
        r.two = 0; n_xretry.fetch_add(1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e == hipSuccess) return SLAM_OK;
    if (st2) (void)hipStreamSynchronize(st2);                  // (work may be in flight on the second stream: it reads the arena the next call reuses)
    return slam_fail(ctx, SLAM_ERR_HIP, "slam_local_ba_batch: %s", hipGetErrorString(e));
}
// results -> the caller's arrays (its pose order, its observation order); a failed factorisation leaves a window's arrays untouched
void batch_scatter(BatchCall &c, BAPool &pool, double *theta, uint8_t *outliers, double *stats)
{
    pool.run(c.S, [&](int k) {
        if (k >= c.NB) return;
        const int z = c.batch[k]; const BAPlan &q = c.plan(k);
        if (q.err) return;
        const BARes &r = c.rtab_h[k];
        const LMState &h = c.state(k);
        if (stats) lm_stats(h, c.dev_ms, stats + 8 * (size_t)z);
        if (h.chol_fail) { c.st_code[z] = SLAM_ERR_NUMERIC; return; }
        const double *th = (const double *)(c.res_host + (r.off_theta - c.res_base));
        double *dst = theta + c.in.th_off[z];
        ba_unpermute(q.ba, th, dst, (const uint8_t *)(c.res_host + (r.off_outl - c.res_base)), outliers + c.in.ob_off[z]);
        memcpy(dst + 6 * q.P, th + 6 * q.P, (size_t)3 * q.M * 8);
    });
}

// ---- slam_local_ba_batch_dev in steps over the same state: dev_probe -> dev_select -> dev_arena -> dev_tables -> dev_enqueue
struct DevCall {
    BatchCall c;
    BADevArgs a;
    std::vector<BADevIn> din;                     // [S] where window z's arrays start in the caller's device arrays
    std::vector<BADevProbe> pr;                   // [S] what the probe kernel found
    size_t din_off = 0;                           // the batch's windows' BADevIn records: behind the tables, in the same upload
    size_t probe_bytes = 0, state_bytes = 0;      // the call's two device -> host copies
    const BADevIn *din_dev() const { return (const BADevIn *)(c.A + din_off); }
};
// the probe kernel over all S windows and its one small copy back
int dev_probe(DevCall &dc, const int32_t *Pn, const int32_t *Mn, const int32_t *On)
{
    slam_ctx *ctx = dc.c.ctx; const int S = dc.c.S;
    dc.din.resize(S); dc.pr.resize(S);
    long long th = 0, pc = 0, ob = 0;
    for (int z = 0; z < S; z++) { dc.din[z] = {th, pc, ob, Pn[z], Mn[z], On[z], 0}; th += 6ll * Pn[z] + 3ll * Mn[z]; pc += Pn[z]; ob += On[z]; }
    const size_t in_b = al((size_t)S * sizeof(BADevIn)), out_b = (size_t)S * sizeof(BADevProbe);
    char *scr, *h;
    int rc = slam_scratch2(ctx, in_b + out_b, (void **)&scr);
    if (!rc) rc = slam_pinned(ctx, in_b + out_b, (void **)&h);
    if (rc) return rc;
    memcpy(h, dc.din.data(), (size_t)S * sizeof(BADevIn));
    HIP_TRY(ctx, hipMemcpyAsync(scr, h, in_b, hipMemcpyHostToDevice, ctx->stream));
    { ProfScope span(ctx, "ba_dev_probe");
      hipLaunchKernelGGL(k_ba_dev_probe, dim3(S), dim3(256), 0, ctx->stream, (const BADevIn *)scr, dc.a, (BADevProbe *)(scr + in_b)); }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h + in_b, scr + in_b, out_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    memcpy(dc.pr.data(), h + in_b, out_b);
    dc.probe_bytes = out_b;
    return SLAM_OK;
}
// Which windows k_ba_window takes -- ba_plan's own rule (ba_window_eligible) on what the probe found, with the poses relabelled so that the free ones are
// last -- and their plans, from sizes alone.  The others get their code: SLAM_ERR_ARG (the contract's two checks) or SLAM_BA_DEV_INELIGIBLE.
void dev_select(DevCall &dc, const double *cams)
{
    BatchCall &c = dc.c;
    const BAKnobs &kn = ba_knobs();
    c.in.pl = std::vector<BAPlan>(c.S); c.st_code.assign(c.S, SLAM_OK); c.route.resize(c.S);
    for (int z = 0; z < c.S; z++) {
        const BADevIn &w = dc.din[z]; const BADevProbe &p = dc.pr[z];
        BAPlan &q = c.in.pl[z];
        q.fx = cams[4 * z]; q.fy = cams[4 * z + 1]; q.cx = cams[4 * z + 2]; q.cy = cams[4 * z + 3]; q.P = w.P; q.M = w.M; q.O = w.O; q.small_groups = true;
        if (p.nfree < 0) { c.st_code[z] = SLAM_BA_DEV_INELIGIBLE; continue; }          // sizes alone: no observations, P > 128, O > 40000
        if (p.flags) { q.fail(SLAM_ERR_ARG, (p.flags & BAD_UNGROUPED) ? "slam_local_ba_batch_dev: an id out of range, or observations not grouped by ascending point id" : "slam_local_ba_batch_dev: a map point is observed twice by one free pose"); c.st_code[z] = SLAM_ERR_ARG; continue; }
        int p0, pspan;
        ba_free_span_relabelled(w.P, p.nfree, &p0, &pspan);
        // (free poses that are consecutive have half-bandwidth <= nfree - 1: the bound stands in for the value, which k_ba_window never reads)
        const int hb = std::max(p.nfree - 1, 0);
        const bool grouped = !kn.no_groups && hb <= BS_MAXHB && sg_fold_fits(hb);
        if (!ba_window_eligible(!kn.no_bw, grouped, p.nfree, pspan, w.P, w.O, p.cmax)) { c.st_code[z] = SLAM_BA_DEV_INELIGIBLE; continue; }
        slam_ba *ba = q.ba = new slam_ba();
        ba->hb = q.hb = hb; ba->p0 = p0; ba->pspan = pspan; ba->grouped = true;
        q.window = true; q.nfree_obs = p.nfree_obs; q.sg_ob = std::max(p.cmax, 1);
        ba_layout(q);
        c.route[z] = solve_route(ba, w.P, c.ctx, true);
        if (!batch_takes(ba, c.route[z])) { c.st_code[z] = SLAM_BA_DEV_INELIGIBLE; continue; }      // (one pose in all: the host form solves it outside the batch)
        c.batch.push_back(z);
    }
    c.NB = (int)c.batch.size();
}
// the arena of the host form with two differences: the windows' BADevIn records travel behind the tables, and the LM states of all windows stand together at
// the head of the result region -- they are all that comes back
int dev_arena(DevCall &dc)
{
    BatchCall &c = dc.c;
    const int NB = c.NB;
    c.up.resize(NB + 1); c.ze.resize(NB + 1); c.wk.resize(NB + 1); c.rs.resize(NB + 1);
    c.tab_bytes = al((size_t)NB * sizeof(BAWin)); c.rtab_bytes = al((size_t)NB * sizeof(BARes)) + al((size_t)NB * 4);
    dc.din_off = c.tab_bytes + c.rtab_bytes;
    c.up[0] = dc.din_off + al((size_t)NB * sizeof(BADevIn)); c.ze[0] = 0; c.wk[0] = 0;
    dc.state_bytes = (size_t)NB * al(sizeof(LMState)); c.rs[0] = dc.state_bytes;
    for (int k = 0; k < NB; k++) {
        const BAPlan &q = c.plan(k);
        c.up[k + 1] = c.up[k] + q.up_bytes; c.ze[k + 1] = c.ze[k] + q.zero_bytes; c.wk[k + 1] = c.wk[k] + q.work_bytes;
        c.rs[k + 1] = c.rs[k] + al((6 * (size_t)q.P + 3 * (size_t)q.M) * 8 + 8) + al((size_t)q.O + 8);
    }
    c.up_total = c.up[NB]; c.zero_base = c.up_total; c.work_base = c.zero_base + c.ze[NB]; c.res_base = c.work_base + c.wk[NB]; c.total = c.res_base + c.rs[NB];
    if (const int rc = slam_scratch(c.ctx, c.total, (void **)&c.A)) return rc;
    if (const int rc = slam_pinned(c.ctx, c.up[0] + dc.state_bytes, (void **)&c.stage)) return rc;
    c.res_host = c.stage + c.up[0]; c.tab_h = (BAWin *)c.stage; c.rtab_h = (BARes *)(c.stage + c.tab_bytes);
    return SLAM_OK;
}
// the tables, from sizes alone: pointers bound (ba_bind), nothing staged
void dev_tables(DevCall &dc)
{
    BatchCall &c = dc.c;
    for (int k = 0; k < c.NB; k++) {
        BAPlan &q = c.plan(k);
        BAWin &w = c.tab_h[k];
        memset(&w, 0, sizeof w);
        BARes &r = c.rtab_h[k];
        r.off_state = c.res_base + (size_t)k * al(sizeof(LMState)); r.off_theta = c.res_base + c.rs[k]; r.off_outl = r.off_theta + al((6 * (size_t)q.P + 3 * (size_t)q.M) * 8 + 8);
        char *zero = c.A + c.zero_base + c.ze[k];
        ba_bind(q, c.A + c.up[k], zero, c.A + c.work_base + c.wk[k]);
        win_table(c, k, zero);
        ((BADevIn *)(c.stage + dc.din_off))[k] = dc.din[c.batch[k]];
    }
}
// tables up, memset, the stager; `solve`: k_ba_window, k_results_b, the results kernel, the states back -- and all of it again, THE STAGER INCLUDED, on one
// workgroup per window if two halves missed each other: the solver advances d.pose / d.pts inside the region the stager wrote, and the caller's arrays are
// still the inputs (k_ba_dev_results wrote nothing)
int dev_enqueue(DevCall &dc, BatchRoute &r, bool solve, int iters_fast, int iterations, double repr_eps)
{
    BatchCall &c = dc.c;
    slam_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    char *A = c.A;
    const int NB = c.NB;
    if (const int rc = window_attr(c, r)) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    for (int attempt = 0; e == hipSuccess && attempt < 2; attempt++) {
        e = hipMemcpyAsync(A, c.stage, c.up[0], hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(A + c.zero_base, 0, c.ze[NB], st);
        if (e != hipSuccess) break;
        (void)hipEventRecord(e0, st);
        { ProfScope span(ctx, "ba_dev_stage");
          hipLaunchKernelGGL(k_ba_dev_stage, dim3(NB), dim3(256), 0, st, (BAWin *)A, dc.din_dev(), dc.a); }
        if (!solve) { e = hipGetLastError(); break; }
        launch_window(c, r, iters_fast, iterations, repr_eps);
        hipLaunchKernelGGL(k_results_b, dim3(8, NB), dim3(256), 0, st, (const BAWin *)A, (const BARes *)(A + c.tab_bytes), A);
        { ProfScope span(ctx, "ba_dev_results");
          hipLaunchKernelGGL(k_ba_dev_results, dim3(NB), dim3(256), 0, st, (const BAWin *)A, (const BARes *)(A + c.tab_bytes), (const char *)A, dc.din_dev(), NB, r.two, dc.a); }
        e = hipGetLastError();
        (void)hipEventRecord(e1, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c.res_host, A + c.res_base, dc.state_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = slam_stream_wait(st);
        if (e == hipSuccess) (void)hipEventElapsedTime(&c.dev_ms, e0, e1);
        if (e != hipSuccess || !r.two) break;
        bool missed = false;
        for (int k = 0; k < NB; k++) if (c.state(k).chol_fail == 2) { missed = true; break; }
        if (!missed) break;
        r.two = 0; n_xretry.fetch_add(1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e == hipSuccess) return SLAM_OK;
    return slam_fail(ctx, SLAM_ERR_HIP, "slam_local_ba_batch_dev: %s", hipGetErrorString(e));
}
int dev_begin(DevCall &dc, slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
              double *theta, const uint8_t *theta_const, const double *pixels_yx, const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers)
{
    ARG_TRY(ctx, ctx != nullptr && S >= 1 && S <= 65535 && cams != nullptr && Pn != nullptr && Mn != nullptr && On != nullptr);
    ARG_TRY(ctx, theta != nullptr && theta_const != nullptr && outliers != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    long long nO = 0;
    for (int z = 0; z < S; z++) { ARG_TRY(ctx, Pn[z] > 0 && Mn[z] >= 0 && On[z] >= 0); nO += On[z]; }
    ARG_TRY(ctx, nO == 0 || (pixels_yx != nullptr && pose_ids != nullptr && point_ids != nullptr));
    dc.c.ctx = ctx; dc.c.S = S;
    dc.a = {theta, theta_const, pixels_yx, pose_ids, point_ids, outliers};
    if (const int rc = dev_probe(dc, Pn, Mn, On)) return rc;
    dev_select(dc, cams);
    if (dc.c.NB == 0) return SLAM_OK;
    if (const int rc = dev_arena(dc)) return rc;
    dev_tables(dc);
    return SLAM_OK;
}
}  // namespace

extern "C" {

// bundle_adjustment! for S windows at once (no reference counterpart, like the other *_batch entry points; the caller is the estimator
// task of S lock-stepped SlamManagers, estimator.jl:78-99 / :317-347): every kernel of slam_local_ba with the window on blockIdx.y, each
// window with its own device-side LM state; host set-up (structure analysis, staging) spread over threads; ONE host -> device copy, one
// memset, 5 launches per LM iteration for the whole batch, one device -> host copy.  Window z's results equal slam_local_ba's on its
// arrays.  Windows the banded group kernels do not cover (no banded pose order, a point with > 448 observations, no observations) are
// solved one by one through slam_local_ba afterwards.
int slam_local_ba_batch(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                        double *theta, const uint8_t *theta_const, const double *pixels_yx,
                        const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                        int iters_fast, int iterations, double repr_eps, double *stats, int32_t *status)
{
    ARG_TRY(ctx, ctx != nullptr && S >= 1 && S <= 65535 && cams != nullptr && Pn != nullptr && Mn != nullptr && On != nullptr);
    ARG_TRY(ctx, theta != nullptr && theta_const != nullptr && outliers != nullptr && iters_fast >= 0 && iterations >= 0);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto tw0 = std::chrono::steady_clock::now();
    for (int z = 0; z < S; z++) ARG_TRY(ctx, Pn[z] > 0 && Mn[z] >= 0 && On[z] >= 0);
    BatchCall c; c.ctx = ctx; c.S = S;
    batch_in(c.in, S, cams, Pn, Mn, On, theta, theta_const, pixels_yx, pose_ids, point_ids);
    const std::vector<size_t> &th_off = c.in.th_off, &pc_off = c.in.pc_off, &ob_off = c.in.ob_off;
    ARG_TRY(ctx, ob_off[S] == 0 || (pixels_yx != nullptr && pose_ids != nullptr && point_ids != nullptr));
    BAPool &pool = ba_pool();
    pool.run(S, [&](int z) { ba_plan(c.in.pl[z]); });
    const auto tw1 = std::chrono::steady_clock::now();
    c.st_code.assign(S, SLAM_OK); c.route.resize(S);
    for (int z = 0; z < S; z++) {                              // the windows the batch kernels take; the others are solved one by one afterwards
        BAPlan &q = c.in.pl[z];
        if (q.err) { c.st_code[z] = q.err; if (!status) return slam_fail(ctx, q.err, "slam_local_ba_batch: window %d: %s", z, q.msg); continue; }
        c.route[z] = solve_route(q.ba, q.P, ctx, true);
        (batch_takes(q.ba, c.route[z]) ? c.batch : c.single).push_back(z);
    }
    c.NB = (int)c.batch.size();
    int rc = SLAM_OK;
    if (c.NB > 0) {
        if ((rc = batch_arena(c)) != SLAM_OK || (rc = batch_stage(c, pool, status)) != SLAM_OK) return rc;
        BatchRoute r = batch_route(c);
        const auto tw2 = std::chrono::steady_clock::now();
        if ((rc = batch_enqueue(c, r, iters_fast, iterations, repr_eps)) != SLAM_OK) return rc;
        const auto tw3 = std::chrono::steady_clock::now();
        batch_scatter(c, pool, theta, outliers, stats);
        if (ba_knobs().host_times) {
            const auto us = [](auto a, auto b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
            fprintf(stderr, "slam_local_ba_batch host: %d windows (%d threads): plan %ld us, emit %ld us, enqueue + wait %ld us (device %.0f us), scatter %ld us; %zu B up, %zu B arena\n",
                    c.NB, (int)pool.th.size() + 1, us(tw0, tw1), us(tw1, tw2), us(tw2, tw3), c.dev_ms * 1e3, us(tw3, std::chrono::steady_clock::now()), c.up_total, c.total);
        }
    }
    for (int z : c.single) {
        if (c.st_code[z]) continue;
        const BAPlan &q = c.in.pl[z];
        double sv[8] = {0};
        const int rc1 = slam_local_ba(ctx, q.fx, q.fy, q.cx, q.cy, q.P, q.M, q.O, theta + th_off[z], theta_const + pc_off[z], q.pixels_yx, q.pose_ids, q.point_ids,
                                      outliers + ob_off[z], iters_fast, iterations, repr_eps, sv);
        if (stats) memcpy(stats + 8 * (size_t)z, sv, sizeof sv);
        c.st_code[z] = rc1;
        if (rc1 && rc1 != SLAM_ERR_NUMERIC && !status) return rc1;
    }
    int first = SLAM_OK;
    for (int z = 0; z < S; z++) { if (status) status[z] = c.st_code[z]; if (c.st_code[z] && !first) first = c.st_code[z]; }
    if (status) return SLAM_OK;                                // per-window codes are in status[]
    if (first == SLAM_ERR_NUMERIC) return slam_fail(ctx, SLAM_ERR_NUMERIC, "slam_local_ba_batch: a reduced camera system was not positive definite (that window's theta and outliers are left unchanged)");
    return first;
}


// slam_local_ba_batch on windows that are resident in HBM (include/slamhip.h has the contract): theta (in / out), theta_const, pixels_yx, pose_ids, point_ids
// and outliers (out) are DEVICE pointers.  k_ba_window's windows only; no host structure analysis, no staging, no scatter: the probe's few ints per window and
// the LM states are all that crosses the bus.
int slam_local_ba_batch_dev(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                            double *theta, const uint8_t *theta_const, const double *pixels_yx,
                            const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                            int iters_fast, int iterations, double repr_eps, double *stats, int32_t *status)
{
    ARG_TRY(ctx, ctx != nullptr && iters_fast >= 0 && iterations >= 0);
    DevCall dc;
    int rc = dev_begin(dc, ctx, S, cams, Pn, Mn, On, theta, theta_const, pixels_yx, pose_ids, point_ids, outliers);
    if (rc) return rc;
    BatchCall &c = dc.c;
    if (stats) memset(stats, 0, (size_t)S * 8 * sizeof(double));
    if (c.NB > 0) {
        BatchRoute r = batch_route(c);
        if ((rc = dev_enqueue(dc, r, true, iters_fast, iterations, repr_eps)) != SLAM_OK) return rc;
        for (int k = 0; k < c.NB; k++) {
            const int z = c.batch[k];
            const LMState &h = c.state(k);
            if (stats) lm_stats(h, c.dev_ms, stats + 8 * (size_t)z);
            if (h.chol_fail) c.st_code[z] = SLAM_ERR_NUMERIC;
        }
        if (ba_knobs().host_times) fprintf(stderr, "slam_local_ba_batch_dev: %d of %d windows, device %.0f us; %zu B of probe results and %zu B of LM states back, %zu B of tables up, %zu B arena\n", c.NB, S, c.dev_ms * 1e3, dc.probe_bytes, dc.state_bytes, c.up[0], c.total);
    }
    int first = SLAM_OK;
    for (int z = 0; z < S; z++) { if (status) status[z] = c.st_code[z]; if (c.st_code[z] && !first) first = c.st_code[z]; }
    if (status || first == SLAM_OK) return SLAM_OK;            // per-window codes are in status[]
    for (int z = 0; z < S; z++) if (c.st_code[z] == first) return slam_fail(ctx, first < 0 ? first : SLAM_ERR_ARG, "slam_local_ba_batch_dev: window %d: %s", z, first == SLAM_ERR_NUMERIC ? "the reduced camera system was not positive definite (theta and outliers are left unchanged)" : first == SLAM_BA_DEV_INELIGIBLE ? "not a window k_ba_window takes (pass status to have the others solved)" : c.in.pl[z].msg);
    return first;
}
// test aid (tests/test_gpu_ba_batch_dev.py): probe and stage the windows as slam_local_ba_batch_dev does, solve nothing, and download window z's staged
// ("uploaded") region into out[0 .. cap).  info (16 int64): the offsets of pose, pts, pconst, pix, opose, opoint, pt_start, pt_id, opk, pfs, fobs, fgrp inside it,
// then its length, the window's ksplit, p0 and free-pose count.  Returns the window's status code when it is not staged (nothing is written then).
int slam_debug_ba_dev_staged(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                             double *theta, const uint8_t *theta_const, const double *pixels_yx, const int64_t *pose_ids, const int64_t *point_ids,
                             uint8_t *outliers, int z, uint8_t *out, long long cap, long long *info)
{
    ARG_TRY(ctx, ctx != nullptr && out != nullptr && info != nullptr && z >= 0 && z < S);
    DevCall dc;
    int rc = dev_begin(dc, ctx, S, cams, Pn, Mn, On, theta, theta_const, pixels_yx, pose_ids, point_ids, outliers);
    if (rc) return rc;
    BatchCall &c = dc.c;
    if (c.st_code[z]) return c.st_code[z];
    const int k = (int)(std::find(c.batch.begin(), c.batch.end(), z) - c.batch.begin());
    const BAPlan &q = c.plan(k);
    ARG_TRY(ctx, (long long)q.up_bytes <= cap);
    BatchRoute r = batch_route(c);
    if ((rc = dev_enqueue(dc, r, false, 0, 0, 0.0)) != SLAM_OK) return rc;
    BAWin w;
    HIP_TRY(ctx, hipMemcpyAsync(out, c.A + c.up[k], q.up_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&w, c.A + (size_t)k * sizeof(BAWin), sizeof w, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    const size_t o[12] = {q.o_pose, q.o_pts, q.o_const, q.o_pix, q.o_opose, q.o_opoint, q.o_start, q.o_ptid, q.o_opk, q.o_pfs, q.o_fobs, q.o_fgrp};
    for (int i = 0; i < 12; i++) info[i] = (long long)o[i];
    info[12] = (long long)q.up_bytes; info[13] = w.ksplit; info[14] = w.B.p0; info[15] = w.B.nb;
    return SLAM_OK;
}

// slam_local_ba_batch in two halves: _begin hands the whole call (structure analysis, staging, upload, solve, download, scatter) to a thread of the
// library's own and returns; _end waits for it and returns its code.  The estimator task of a host (estimator.jl:78-99) thereby prepares key-frame
// k + 1's windows -- or does anything else -- while key-frame k's are planned and solved, without a thread of its own.  Between the two calls the
// context belongs to the job (one outstanding job per context; the arrays passed to _begin are read AND written by the job: they stay valid and
// untouched until _end returns).  A host that wants several batches in flight uses several contexts.
struct BABatchJob { std::thread th; int rc = SLAM_OK; bool active = false; };
static std::mutex g_job_mu;
static std::vector<std::pair<slam_ctx *, BABatchJob *>> g_jobs;
static BABatchJob *job_of(slam_ctx *ctx, bool create)
{
    std::lock_guard<std::mutex> lk(g_job_mu);
    for (auto &e : g_jobs) if (e.first == ctx) return e.second;
    if (!create) return nullptr;
    g_jobs.emplace_back(ctx, new BABatchJob());
    return g_jobs.back().second;
}
int slam_local_ba_batch_begin(slam_ctx *ctx, int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On,
                              double *theta, const uint8_t *theta_const, const double *pixels_yx,
                              const int64_t *pose_ids, const int64_t *point_ids, uint8_t *outliers,
                              int iters_fast, int iterations, double repr_eps, double *stats, int32_t *status)
{
    ARG_TRY(ctx, ctx != nullptr);
    BABatchJob *j = job_of(ctx, true);
    if (j->active) return slam_fail(ctx, SLAM_ERR_ARG, "slam_local_ba_batch_begin: the context already has a batch in flight (call slam_local_ba_batch_end first)");
    j->active = true; j->rc = SLAM_OK;
    j->th = std::thread([=] { j->rc = slam_local_ba_batch(ctx, S, cams, Pn, Mn, On, theta, theta_const, pixels_yx, pose_ids, point_ids, outliers, iters_fast, iterations, repr_eps, stats, status); });
    return SLAM_OK;
}
int slam_local_ba_batch_end(slam_ctx *ctx)
{
    ARG_TRY(ctx, ctx != nullptr);
    BABatchJob *j = job_of(ctx, false);
    if (!j || !j->active) return slam_fail(ctx, SLAM_ERR_ARG, "slam_local_ba_batch_end: no batch in flight on this context");
    j->th.join(); j->active = false;
    return j->rc;                                              // (the message of a failure is the context's: slam_last_error)
}
// a context that goes away takes its job record along (called by slam_ctx_destroy; a job still in flight is waited for)
extern "C" void ba_forget_jobs(slam_ctx *ctx)
{
    BABatchJob *j = nullptr;
    {   std::lock_guard<std::mutex> lk(g_job_mu);
        for (size_t i = 0; i < g_jobs.size(); i++) if (g_jobs[i].first == ctx) { j = g_jobs[i].second; g_jobs.erase(g_jobs.begin() + (long)i); break; } }
    if (j) { if (j->active) j->th.join(); delete j; }
}

// how many slam_local_ba_batch calls of this process had to be solved again because the two workgroups of a window missed each other
long slam_debug_ba_xretries(void) { return n_xretry.load(); }

// host-only timing of the batch set-up (no HIP call, no device needed): plan + emit of S windows on `threads` threads (0: the library's parked
// worker pool, as slam_local_ba_batch uses it; -N: one window at a time with its passes over the observations split into <= N tasks of the pool, as slam_local_ba does; -1: the same on the calling thread) into malloc'ed staging; out_us = {plan, emit, a 52-bit hash of everything staged and of the observation orders}; returns the number of windows whose set-up failed.  Measurement aid for tuning the host side on any machine (scripts/probes/ba_host_time.py).
int slam_debug_ba_host_time(int S, const double *cams, const int32_t *Pn, const int32_t *Mn, const int32_t *On, const double *theta, const uint8_t *theta_const,
                            const double *pixels_yx, const int64_t *pose_ids, const int64_t *point_ids, int threads, double *out_us)
{
    const auto t0 = std::chrono::steady_clock::now();
    BatchIn in;
    batch_in(in, S, cams, Pn, Mn, On, theta, theta_const, pixels_yx, pose_ids, point_ids);
    std::vector<BAPlan> &pl = in.pl;
    auto parallel = [&](auto fn) {
        if (threads == 0) { ba_pool().run(S, fn); return; }      // the parked worker pool of slam_local_ba_batch itself (callers from several threads take turns)
        if (threads <= 1) { for (int z = 0; z < S; z++) fn(z); return; }
        std::vector<std::thread> th;
        for (int t = 1; t < threads; t++) th.emplace_back([&, t] { for (int z = t; z < S; z += threads) fn(z); });
        for (int z = 0; z < S; z += threads) fn(z);
        for (auto &x : th) x.join();
    };
    if (threads < 0) for (int z = 0; z < S; z++) { pl[z].small_groups = false; pl[z].nthreads = -threads; ba_plan(pl[z]); }     // slam_local_ba's way: one window at a time, its passes split over the pool
    else parallel([&](int z) { ba_plan(pl[z]); });
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<size_t> up(S + 1, 0);
    for (int z = 0; z < S; z++) up[z + 1] = up[z] + pl[z].up_bytes;
    std::vector<char> stage(up[S] + 64);                       // (allocated and zero-filled outside the two timed spans)
    char *fake = (char *)(uintptr_t)0x100000000ull;
    const auto t1b = std::chrono::steady_clock::now();
    if (threads < 0) { for (int z = 0; z < S; z++) if (!pl[z].err) ba_emit(pl[z], fake, fake, fake, stage.data() + up[z]); }
    else parallel([&](int z) { if (!pl[z].err) ba_emit(pl[z], fake, fake, fake, stage.data() + up[z]); });
    const auto t2 = std::chrono::steady_clock::now();
    out_us[0] = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count() * 1e-3;
    out_us[1] = (double)std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1b).count() * 1e-3;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
    for (int z = 0; z < S; z++) if (!pl[z].err) { mix(stage.data() + up[z], pl[z].up_bytes); mix(pl[z].ba->perm.data(), pl[z].ba->perm.size() * sizeof(int)); }
    out_us[2] = (double)(h >> 12);
    int bad = 0;
    for (int z = 0; z < S; z++) bad += pl[z].err != 0;
    return bad;
}

} // extern "C"
