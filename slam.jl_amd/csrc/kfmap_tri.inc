// kfmap_tri.inc -- triangulate_temporal! (src/mapper.jl:185-262) on the key-frame map, included at the end of kfmap.hip: slam_kfmap_triangulate_temporal.
// Every input is the map's own -- the slabs' undistorted pixels, ktheta as the last bundle adjustment left it, the observer masks, the table's flags -- so
// the step has no host array and no wait.  Two kernels:
//   k_kfm_tri_poses      per selected stream and ring slot with a key-frame other than the newest: what mapper.jl:226-231 computes once per observer, the
//                        64 doubles of the set seam's table (P2 = K rel_pose_inv | rel_pose_inv | rel_pose = observer.cw frame.wc | observer.wc), into scratch
//   k_kfm_tri_temporal   one thread per observation of the newest slab: the rules below, the arithmetic temporal_pair's (geom_device.hpp: the one copy, the set
//                        seam's too), the first observer kfm_first_observer's (kfmap_ring.hpp)
// Rules, for the live observation i (point `id`) of the newest key-frame k (slot r0) of stream s:
//   1  its point is not owned by the entry, dead, or 3-D already: skipped (get_2d_keypoints, :208-211; no remove_mappoint_obs! clean-up for a missing point)
//   2  fewer than two observers, or the first observer -- the SMALLEST key-frame id among the mask's meaningful bits, as it is now -- is k itself: skipped
//   3  the first observer's slab does not hold the id alive: skipped (:234-235)
//   4  accepted (update_mappoint!): pxyz = observer.wc X, flags |= KFM_3D (not KFM_BA); with a list, the slot that carries the id NOW (binary search: a
//      merge may have moved it) takes xyz and is3d = 1; an id the list no longer holds is no error
//   5  rejected (remove_mappoint_obs!(map, id, k)): the observation becomes a tombstone, the point loses bit r0 (atomicAnd, as kfm_forget_slab), with the
//      row store the row keyed k goes (kfm_rows_lost; an observer remains by rule 2).  THE LIVE LIST KEEPS THE KEYPOINT, as the reference's current frame
//      does (slam_kpset_triangulate_temporal compacts it away)
// A thread writes its own observation, its own point's entry (ids are unique within a slab) and at most one list slot: no thread waits on another.
// counts[s] = {candidates after rule 1, triangulated, observations removed, skipped by rules 2-3}: atomicAdd into scratch the seam zeroes.

// inv(SE3, T) in closed form: [R' | -R' t], column-major 4 x 4
__device__ __forceinline__ void kfm_se3_inv(const double *T, double *O)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) O[i + 4 * j] = T[j + 4 * i];
        O[3 + 4 * i] = 0.0;
        O[12 + i] = -((T[4 * i] * T[12] + T[4 * i + 1] * T[13]) + T[4 * i + 2] * T[14]);
    }
    O[15] = 1.0;
}
// C = A B, column-major 4 x 4
__device__ __forceinline__ void kfm_mul4(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) C[i + 4 * j] = ((A[i] * B[4 * j] + A[i + 4] * B[4 * j + 1]) + A[i + 8] * B[4 * j + 2]) + A[i + 12] * B[4 * j + 3];
}

// one workgroup per selected stream, one thread per ring slot; tab: [S R][64]
__global__ __launch_bounds__(64) void k_kfm_tri_poses(KfmapView V, const double *cams, double *tab, const int *sel)
{
    const int s = KFM_STREAM(blockIdx.x), b = threadIdx.x, R = V.R, kfid = V.cur[s] - 1;
    if (b >= R || kfid < 0) return;
    const int r0 = kfid % R, t = V.tag[s * R + b];
    if (t == 0 || b == r0) return;
    const double *cam = cams + 4 * (size_t)s;
    double Tob[16], Tfr[16], A[16], REL[16], INV[16];
    kfm_tcw(V.ktheta + 6 * ((size_t)s * R + b), Tob);            // observer.cw
    kfm_tcw(V.ktheta + 6 * ((size_t)s * R + r0), Tfr);           // frame.cw
    kfm_se3_inv(Tfr, A);                                         // frame.wc
    kfm_mul4(Tob, A, REL);                                       // rel_pose = observer.cw * frame.wc
    kfm_se3_inv(REL, INV);                                       // rel_pose_inv
    kfm_se3_inv(Tob, A);                                         // observer.wc
    double *E = tab + ((size_t)s * R + b) * 64;
#pragma unroll
    for (int j = 0; j < 4; j++) {                                // P2 = K * rel_pose_inv
        E[4 * j] = cam[0] * INV[4 * j] + cam[2] * INV[4 * j + 2]; E[4 * j + 1] = cam[1] * INV[4 * j + 1] + cam[3] * INV[4 * j + 2];
        E[4 * j + 2] = INV[4 * j + 2]; E[4 * j + 3] = INV[4 * j + 3];
    }
#pragma unroll
    for (int k = 0; k < 16; k++) { E[16 + k] = INV[k]; E[32 + k] = REL[k]; E[48 + k] = A[k]; }
}

// what the kernel needs of the live lists (id == nullptr: none, the lists are the host's business)
struct KfmTriList { const int64_t *id; double *xyz; uint8_t *is3d; const int *count; int cap; };

template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_tri_temporal(KfmView<ROWS> V, KfmTriList K, const double *cams, const double *tab,
                                                                               double max_error, double min_depth, double min_parallax, int *counts, const int *sel)
{
    const int s = KFM_STREAM(blockIdx.y), i = blockIdx.x * 256 + threadIdx.x, R = V.R, kfid = V.cur[s] - 1;
    if (kfid < 0) return;
    const int r0 = kfid % R;
    const int *tag = V.tag + s * R;
    if (tag[r0] != kfid + 1 || i >= min(V.kn[s * R + r0], V.cap)) return;
    int64_t id;
    size_t pe;
    if (!kfm_slab_point(V, s, r0, i, id, pe) || !kfm_valid(V, pe, id)) return;                     // rule 1
    const uint8_t fl = V.pflags[pe];
    if (fl & KFM_3D) return;
    int *cnt = counts + 4 * s;
    atomicAdd(&cnt[0], 1);
    const int ob = kfm_first_observer(V.pmask[pe], tag, R);                                        // rule 2
    const int j = ob >= 0 && ob != r0 ? kfm_find_live(V, s, ob, id) : -1;                          // rule 3
    if (j < 0) { atomicAdd(&cnt[3], 1); return; }
    const size_t q = ((size_t)s * R + r0) * V.cap + i, qo = ((size_t)s * R + ob) * V.cap + j;
    double W[3];
    if (temporal_pair(cams + 4 * (size_t)s, tab + ((size_t)s * R + ob) * 64, V.kupx[2 * qo], V.kupx[2 * qo + 1], V.kupx[2 * q], V.kupx[2 * q + 1],
                      max_error, min_depth, min_parallax, W)) {
        for (int k = 0; k < 3; k++) V.pxyz[3 * pe + k] = W[k];                                     // update_mappoint!
        V.pflags[pe] = fl | KFM_3D;
        if (K.id) {
            const size_t lb = (size_t)s * K.cap;
            const int l = kfm_find(K.id + lb, min(K.count[s], K.cap), id);
            if (l >= 0) { for (int k = 0; k < 3; k++) K.xyz[3 * (lb + l) + k] = W[k]; K.is3d[lb + l] = 1; }
        }
        atomicAdd(&cnt[1], 1);
    } else {                                                                                       // remove_mappoint_obs!(map, id, k)
        V.klive[q] = 0;
        const unsigned long long old = atomicAnd(&V.pmask[pe], ~(1ull << r0));
        if constexpr (ROWS) { if (old >> r0 & 1) kfm_rows_lost(V, s, pe, tag[r0], old & ~(1ull << r0)); }
        atomicAdd(&cnt[2], 1);
    }
}

extern "C" {

int slam_kfmap_triangulate_temporal(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, const double *cams, double max_error, double min_depth, double min_parallax,
                                    int32_t *counts)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && cams != nullptr && (ks == nullptr || (ks->S == km->v.S && ks->v.cap <= km->v.cap)));
    const KfmapView &V = km->v;
    const int S = V.S;
    for (int s = 0; s < S; s++)                                  // every check before anything is enqueued
        if (!(std::isfinite(cams[4 * s]) && std::isfinite(cams[4 * s + 1]) && std::isfinite(cams[4 * s + 2]) && std::isfinite(cams[4 * s + 3])) || cams[4 * s] == 0.0 || cams[4 * s + 1] == 0.0)
            return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_triangulate_temporal: stream %d: camera %g %g %g %g (finite, fx and fy non-zero)", s, cams[4 * s], cams[4 * s + 1], cams[4 * s + 2], cams[4 * s + 3]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int list[128];
    const int ns = kfmap_streams(km, list);
    if (counts) memset(counts, 0, (size_t)S * 16);
    if (ns == 0) return SLAM_OK;
    Layout D;                                                    // the inputs, then the device-only regions: the counters and the observers' table
    const auto o_sel = D.take<int>(S); const auto o_cam = D.take<double>(4 * (size_t)S); const size_t in_b = D.size();
    const auto o_cnt = D.take<int>(4 * (size_t)S); const auto o_tab = D.take<double>((size_t)S * V.R * 64);
    char *scr, *h;
    int rc = kfmap_upload(ctx, km, in_b, &scr, [&](char *h) { kfmap_put_streams(o_sel, h, list, ns); memcpy(o_cam.at(h), cams, o_cam.bytes()); }, D.size());
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(o_cnt.at(scr), 0, o_cnt.bytes(), ctx->stream));
    KfmTriList K = {nullptr, nullptr, nullptr, nullptr, 0};
    if (ks) K = {ks->v.id, ks->v.xyz, ks->v.is3d, ks->v.count, ks->v.cap};
    const int *sel = o_sel.at(scr);
    { ProfScope span(ctx, "kfmap_tri");
      { ProfScope part(ctx, "kfmap_tri_poses");
        hipLaunchKernelGGL(k_kfm_tri_poses, dim3(ns), dim3(64), 0, ctx->stream, V, (const double *)o_cam.at(scr), o_tab.at(scr), sel); }
      { ProfScope part(ctx, "kfmap_tri_temporal");
        KFM_LAUNCH_ROWS(km, k_kfm_tri_temporal, dim3((V.cap + 255) / 256, ns), K, (const double *)o_cam.at(scr), (const double *)o_tab.at(scr),
                        max_error, min_depth, min_parallax, o_cnt.at(scr), sel); } }
    HIP_TRY(ctx, hipGetLastError());
    if (!counts) return SLAM_OK;
    rc = slam_pinned(ctx, (size_t)S * 16, (void **)&h);
    if (rc) return rc;
    rc = kpset_read_back(ctx, h, {{0, o_cnt.at(scr), (size_t)S * 16, nullptr}});
    if (rc) return rc;
    for (int k = 0; k < ns; k++) memcpy(counts + 4 * (size_t)list[k], h + 16 * (size_t)list[k], 16);          // (a stream the call did not act on keeps its zeros)
    return SLAM_OK;
}

}  // extern "C"
