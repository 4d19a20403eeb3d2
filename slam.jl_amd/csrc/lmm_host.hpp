// lmm_host.hpp -- host staging of the local-map match (localmap.hip): lmm_plan checks the arguments and lays the call's one packed buffer out,
// lmm_emit fills it (stream table, the caller's arrays region by region, the cell grid of every stream's keypoints as a CSR).  No HIP calls and no
// HIP types, so the pair compiles and runs as plain C++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/slamhip.h"

// the two routines the device stager of the key-frame map (kfmap_lmm.inc) shares with this file compile for both sides under hipcc
#if defined(__HIPCC__)
#define LMM_HD __host__ __device__
#else
#define LMM_HD
#endif

// what the kernel reads per stream (one entry per stream that has both keypoints and local-map points)
struct LmmStream {
    double Tcw[16];                               // frame.cw, column-major
    double fx, fy, cx, cy, k1, k2, p1, p2, H, W;
    double max_proj;                              // max_projection_distance, doubled already when nb_3d_kpts < 30 (mapper.jl:332)
    double start;                                 // 256.0 * max_descriptor_distance (mapper.jl:401)
    double view_thr;                              // cos(atan(max(vfov, hfov))) (mapper.jl:326-329)
    int32_t cell, gr, gc;                         // cell size, grid rows / columns
    int32_t N, M, K;
    int32_t kp0, kf0, mp0, cell0;                 // first keypoint / key-frame row / local-map point / cell_off entry of the stream
};

// the argument block of k_lmm_match (localmap.hip), by value: the regions of one packed buffer, wherever they were filled -- by lmm_emit on the host
// (slam_local_map_match*) or on the device from the key-frame map (slam_kfmap_local_map_match, fixed per-stream strides)
struct LmmDev {
    const LmmStream *st;
    const double *kp_yx; const int32_t *kp_desc_off; const uint64_t *kp_desc; const int32_t *kp_obs_off, *kp_obs_kf; const double *kp_obs_yx;
    const double *kf_Tcw;
    const double *mp_xyz; const int32_t *mp_desc_off; const uint64_t *mp_desc; const int32_t *mp_obs_off, *mp_obs_kf;
    const int32_t *cell_off, *cell_kp;
    int32_t *best_kp; double *best_dist, *proj;
    unsigned long long *keys;
};
// the one launch of k_lmm_match<LMM_G> (localmap.hip): n_streams rows of D.st, every row's M <= max_M; enqueue-only, the caller checks hipGetLastError
struct slam_ctx;
void lmm_launch(slam_ctx *ctx, const LmmDev &D, int max_M, int n_streams);

enum { LMM_ST, LMM_KP_YX, LMM_KP_DOFF, LMM_KP_DESC, LMM_KP_OOFF, LMM_KP_OKF, LMM_KP_OYX, LMM_KF, LMM_MP_XYZ, LMM_MP_DOFF, LMM_MP_DESC, LMM_MP_OOFF,
       LMM_MP_OKF, LMM_CELL_OFF, LMM_CELL_KP, LMM_IN_REGIONS,
       LMM_BEST_KP = LMM_IN_REGIONS, LMM_BEST_DIST, LMM_PROJ, LMM_KEYS, LMM_REGIONS };

struct LmmPlan {
    int S = 0;
    std::vector<int> active;                      // streams with N > 0 and M > 0, in stream order
    std::vector<int> cell0;                       // per active stream: first entry of its cell_off block
    int Ntot = 0, Ktot = 0, Mtot = 0, max_M = 0;
    size_t off[LMM_REGIONS + 1] = {};             // byte offsets of the regions; [LMM_IN_REGIONS] = end of the uploaded part, [LMM_KEYS] = state region
    size_t in_bytes() const { return off[LMM_IN_REGIONS]; }
    size_t out_bytes() const { return off[LMM_REGIONS] - off[LMM_IN_REGIONS]; }
    size_t total() const { return off[LMM_REGIONS]; }
};

static inline bool lmm_monotone(const int32_t *o, int n, std::string &err, const char *what)
{
    if (o[0] != 0) { err = std::string(what) + "[0] is not 0"; return false; }
    for (int i = 0; i < n; i++)
        if (o[i + 1] < o[i]) { char b[160]; snprintf(b, sizeof b, "%s decreases at entry %d (%d -> %d)", what, i + 1, o[i], o[i + 1]); err = b; return false; }
    return true;
}

// the cell of a pixel coordinate: round(p) ÷ cell_size + 1, round to nearest even, ÷ truncating (SLAM.jl:30,42-45)
LMM_HD static inline long long lmm_cell(double p, int cell) { return (long long)rint(p) / cell + 1; }

// The frame constants of a local-map call that follow from a stream's camera row (fx fy cx cy k1 k2 p1 p2 H W), its cell size and its
// max_descriptor_distance -- one copy for lmm_plan / lmm_emit and the key-frame map's stager (kfmap_lmm.inc).  false: cell_size, H or W out of range
// (each seam reports it in its own words).
struct LmmFrame { double start, view_thr; int32_t gr, gc; };
static inline bool lmm_frame(const double *cam, int cell, double max_descriptor_distance, LmmFrame &F)
{
    const double H = cam[8], W = cam[9];
    if (cell < 1 || !(H >= 1.0) || !(W >= 1.0) || H > 65536.0 || W > 65536.0) return false;
    F.start = 256.0 * max_descriptor_distance;                                         // mapper.jl:401
    const double vfov = 0.5 * H / cam[1], hfov = 0.5 * W / cam[0];                     // mapper.jl:326-329
    F.view_thr = std::cos(vfov > hfov ? std::atan(vfov) : std::atan(hfov));
    F.gr = (int)std::ceil(H / cell); F.gc = (int)std::ceil(W / cell);
    return true;
}

// Checks every argument the device would trust and lays the buffer out.  false: `err` says what is wrong, nothing may be launched.
static inline bool lmm_plan(int S, const int32_t *kp_offsets, const int32_t *kf_offsets, const int32_t *mp_offsets, const slam_local_map_args *a,
                            LmmPlan &P, std::string &err)
{
    if (S < 1 || !kp_offsets || !kf_offsets || !mp_offsets || !a) { err = "S < 1 or a null offsets / argument block"; return false; }
    if (!lmm_monotone(kp_offsets, S, err, "kp_offsets") || !lmm_monotone(kf_offsets, S, err, "kf_offsets") || !lmm_monotone(mp_offsets, S, err, "mp_offsets"))
        return false;
    P = LmmPlan();
    P.S = S; P.Ntot = kp_offsets[S]; P.Ktot = kf_offsets[S]; P.Mtot = mp_offsets[S];
    if (!a->Tcw || !a->cam || !a->cell_size || !a->nb_3d_kpts || !a->max_projection_distance || !a->max_descriptor_distance) { err = "a null frame array"; return false; }
    if (P.Ntot > 0 && (!a->kp_yx || !a->kp_desc_off || !a->kp_obs_off || !a->match)) { err = "a null keypoint array"; return false; }
    if (P.Mtot > 0 && (!a->mp_xyz || !a->mp_desc_off || !a->mp_obs_off || !a->best_kp || !a->best_dist || !a->proj_yx)) { err = "a null local-map array"; return false; }
    if (P.Ktot > 0 && !a->kf_Tcw) { err = "kf_Tcw is null"; return false; }
    int kpD = 0, kpO = 0, mpD = 0, mpO = 0;
    if (P.Ntot > 0) {
        if (!lmm_monotone(a->kp_desc_off, P.Ntot, err, "kp_desc_off") || !lmm_monotone(a->kp_obs_off, P.Ntot, err, "kp_obs_off")) return false;
        kpD = a->kp_desc_off[P.Ntot]; kpO = a->kp_obs_off[P.Ntot];
        if ((kpD > 0 && !a->kp_desc) || (kpO > 0 && (!a->kp_obs_kf || !a->kp_obs_yx))) { err = "a null keypoint descriptor / observer array"; return false; }
    }
    if (P.Mtot > 0) {
        if (!lmm_monotone(a->mp_desc_off, P.Mtot, err, "mp_desc_off") || !lmm_monotone(a->mp_obs_off, P.Mtot, err, "mp_obs_off")) return false;
        mpD = a->mp_desc_off[P.Mtot]; mpO = a->mp_obs_off[P.Mtot];
        if ((mpD > 0 && !a->mp_desc) || (mpO > 0 && !a->mp_obs_kf)) { err = "a null local-map descriptor / observer array"; return false; }
    }
    size_t cells = 0;
    for (int s = 0; s < S; s++) {
        const int N = kp_offsets[s + 1] - kp_offsets[s], M = mp_offsets[s + 1] - mp_offsets[s], K = kf_offsets[s + 1] - kf_offsets[s];
        const double H = a->cam[10 * s + 8], W = a->cam[10 * s + 9];
        const int cell = a->cell_size[s];
        char b[200];
        LmmFrame F;
        if (!lmm_frame(a->cam + 10 * s, cell, a->max_descriptor_distance[s], F)) { snprintf(b, sizeof b, "stream %d: cell_size %d / image %g x %g out of range", s, cell, H, W); err = b; return false; }
        const int gr = F.gr, gc = F.gc;
        // observer rows are checked for every stream, launched or not: a caller's bad table is reported where it is
        for (int o = P.Ntot ? a->kp_obs_off[kp_offsets[s]] : 0, e = P.Ntot ? a->kp_obs_off[kp_offsets[s + 1]] : 0; o < e; o++)
            if (a->kp_obs_kf[o] < 0 || a->kp_obs_kf[o] >= K) { snprintf(b, sizeof b, "stream %d: kp_obs_kf[%d] = %d is no row of its %d key-frames", s, o, a->kp_obs_kf[o], K); err = b; return false; }
        for (int o = P.Mtot ? a->mp_obs_off[mp_offsets[s]] : 0, e = P.Mtot ? a->mp_obs_off[mp_offsets[s + 1]] : 0; o < e; o++)
            if (a->mp_obs_kf[o] < 0 || a->mp_obs_kf[o] >= K) { snprintf(b, sizeof b, "stream %d: mp_obs_kf[%d] = %d is no row of its %d key-frames", s, o, a->mp_obs_kf[o], K); err = b; return false; }
        if (N == 0 || M == 0) continue;
        for (int j = kp_offsets[s]; j < kp_offsets[s + 1]; j++) {
            const long long r = lmm_cell(a->kp_yx[2 * j], cell), c = lmm_cell(a->kp_yx[2 * j + 1], cell);
            if (!(r >= 1 && r <= gr && c >= 1 && c <= gc)) { snprintf(b, sizeof b, "stream %d: keypoint %d at (%g, %g) lies in no cell of the %d x %d grid", s, j - kp_offsets[s], a->kp_yx[2 * j], a->kp_yx[2 * j + 1], gr, gc); err = b; return false; }
        }
        P.active.push_back(s); P.cell0.push_back((int)cells);
        cells += (size_t)gr * gc + 1;
        if (M > P.max_M) P.max_M = M;
    }
    const size_t bytes[LMM_REGIONS] = {
        P.active.size() * sizeof(LmmStream), (size_t)P.Ntot * 16, ((size_t)P.Ntot + 1) * 4, (size_t)kpD * 32, ((size_t)P.Ntot + 1) * 4, (size_t)kpO * 4, (size_t)kpO * 16,
        (size_t)P.Ktot * 128, (size_t)P.Mtot * 24, ((size_t)P.Mtot + 1) * 4, (size_t)mpD * 32, ((size_t)P.Mtot + 1) * 4, (size_t)mpO * 4, cells * 4, (size_t)P.Ntot * 4,
        (size_t)P.Mtot * 4, (size_t)P.Mtot * 8, (size_t)P.Mtot * 16, (size_t)P.Ntot * 8 };
    P.off[0] = 0;
    for (int r = 0; r < LMM_REGIONS; r++) P.off[r + 1] = P.off[r] + ((bytes[r] + 255) & ~(size_t)255);
    if (P.total() > ((size_t)1 << 34)) { err = "the call's arrays exceed 16 GiB"; return false; }
    return true;
}

// Fills the uploaded part of the buffer (P.in_bytes() bytes at `buf`).
static inline void lmm_emit(const LmmPlan &P, const int32_t *kp_offsets, const int32_t *kf_offsets, const int32_t *mp_offsets, const slam_local_map_args *a, char *buf)
{
    auto put = [&](int region, const void *src, size_t n) { if (n) memcpy(buf + P.off[region], src, n); };
    const int kpD = P.Ntot ? a->kp_desc_off[P.Ntot] : 0, kpO = P.Ntot ? a->kp_obs_off[P.Ntot] : 0;
    const int mpD = P.Mtot ? a->mp_desc_off[P.Mtot] : 0, mpO = P.Mtot ? a->mp_obs_off[P.Mtot] : 0;
    put(LMM_KP_YX, a->kp_yx, (size_t)P.Ntot * 16);
    if (P.Ntot) { put(LMM_KP_DOFF, a->kp_desc_off, ((size_t)P.Ntot + 1) * 4); put(LMM_KP_OOFF, a->kp_obs_off, ((size_t)P.Ntot + 1) * 4); }
    put(LMM_KP_DESC, a->kp_desc, (size_t)kpD * 32); put(LMM_KP_OKF, a->kp_obs_kf, (size_t)kpO * 4); put(LMM_KP_OYX, a->kp_obs_yx, (size_t)kpO * 16);
    put(LMM_KF, a->kf_Tcw, (size_t)P.Ktot * 128);
    put(LMM_MP_XYZ, a->mp_xyz, (size_t)P.Mtot * 24);
    if (P.Mtot) { put(LMM_MP_DOFF, a->mp_desc_off, ((size_t)P.Mtot + 1) * 4); put(LMM_MP_OOFF, a->mp_obs_off, ((size_t)P.Mtot + 1) * 4); }
    put(LMM_MP_DESC, a->mp_desc, (size_t)mpD * 32); put(LMM_MP_OKF, a->mp_obs_kf, (size_t)mpO * 4);
    LmmStream *st = (LmmStream *)(buf + P.off[LMM_ST]);
    int32_t *cell_off = (int32_t *)(buf + P.off[LMM_CELL_OFF]), *cell_kp = (int32_t *)(buf + P.off[LMM_CELL_KP]);
    std::vector<int32_t> cur;
    for (size_t z = 0; z < P.active.size(); z++) {
        const int s = P.active[z];
        LmmStream &T = st[z];
        memcpy(T.Tcw, a->Tcw + 16 * (size_t)s, sizeof T.Tcw);
        memcpy(&T.fx, a->cam + 10 * (size_t)s, 10 * sizeof(double));
        T.max_proj = a->max_projection_distance[s];
        if (a->nb_3d_kpts[s] < 30) T.max_proj *= 2.0;                                   // mapper.jl:332
        LmmFrame F;
        (void)lmm_frame(&T.fx, a->cell_size[s], a->max_descriptor_distance[s], F);      // (in range: lmm_plan has checked)
        T.start = F.start; T.view_thr = F.view_thr;
        T.cell = a->cell_size[s]; T.gr = F.gr; T.gc = F.gc;
        T.kp0 = kp_offsets[s]; T.kf0 = kf_offsets[s]; T.mp0 = mp_offsets[s]; T.cell0 = P.cell0[z];
        T.N = kp_offsets[s + 1] - T.kp0; T.K = kf_offsets[s + 1] - T.kf0; T.M = mp_offsets[s + 1] - T.mp0;
        // stable counting sort of the keypoints over their cell (row-major r, c): inside a cell the list order is kept
        const int cells = T.gr * T.gc;
        int32_t *co = cell_off + T.cell0, *ck = cell_kp + T.kp0;
        memset(co, 0, ((size_t)cells + 1) * 4);
        auto cell_of = [&](int j) { const double *p = a->kp_yx + 2 * ((size_t)T.kp0 + j);
                                    return (int)((lmm_cell(p[0], T.cell) - 1) * T.gc + (lmm_cell(p[1], T.cell) - 1)); };
        for (int j = 0; j < T.N; j++) co[cell_of(j) + 1]++;
        for (int q = 0; q < cells; q++) co[q + 1] += co[q];
        cur.assign(co, co + cells);
        for (int j = 0; j < T.N; j++) ck[cur[cell_of(j)]++] = j;
    }
}

// key of the reverse selection -> local-map index (mapper.jl:370-381); all ones: nobody chose the keypoint
LMM_HD static inline int32_t lmm_decode(uint64_t key) { return key == ~(uint64_t)0 ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu)); }
