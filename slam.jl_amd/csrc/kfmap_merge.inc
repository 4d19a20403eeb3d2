// kfmap_merge.inc -- part of kfmap.hip: slam_kfmap_merge, the mapper's merge_matches -> merge_mappoints -> update_keypoint! (mapper.jl:296-310,
// map_manager.jl:378-427, frame.jl:290-307) on the key-frame map.  The pairs (prev_id, new_id) of a local-map match -- where they lie in HBM, or a
// caller's -- are applied in HBM: a keypoint is renamed in every key-frame that observes it, and because every slab and every live list is sorted by id
// (kfm_find is a binary search) the touched slabs and lists are rebuilt in order.  tests/np_kfmap_merge.py is the model; kfmap.hpp has the scratch
// allocation's formula and the deviations; kfm_find, kfm_lower and the one-to-one rule of the pairs (device and host form) are kfmap_ring.hpp's.
//
// Three kernels, no workgroup waits for another, nothing returns to the host between them:
//   k_kfm_merge_resolve   one workgroup per stream: the pairs are checked (one-to-one), each pair by one thread: validity, then for every observer slab of
//                         prev that holds prev alive and new not: (position, new id) appended to the slab's rename list; the table is written here
//   k_kfm_merge_slabs     one workgroup per (stream, slot), leaving at once without a rename: the slab rebuilt by a rank merge (kfm_rename_plan / _dest)
//   k_kfm_merge_list      one workgroup per stream: the same rank merge for the live list, every field of the record travelling
// The rank merge: the k renamed records are ranked by new id (by counting: k is small); an untouched record goes to (untouched records kept before it) +
// (new ids below its id), a renamed record of rank r to r + (untouched records kept with an id below its new id); a tombstone whose id equals an arriving
// id is dropped.  Destinations are written into a scratch slab and copied back behind a barrier, in chunks of 256: cap need not fit in LDS.

// the rename list and the plan of one slab (or list): regions of the scratch allocation, each [cap] ([cap + 1]: kept)
struct KfmRename {
    int *pos; int64_t *id;                // the list as appended: position of the renamed record, its new id
    int64_t *sid;                         // the new ids ascending
    int *rank;                            // by position: -1 an untouched record that stays, -2 a dropped tombstone, r >= 0: renamed, rank r
    int *kept;                            // by position i: untouched records kept among [0, i); [n]: their number
};
// k_kfm_merge_list carries the fields k_kpset_compact's load and store blocks carry (kpset_kernels.inc; oyx and st are scratch of a match there as here).
// A field added to the set changes the size of its view: this assert then stops the build until the list kernel and q_* carry the field too
// (tests/test_gpu_kfmap_merge.py fills every field an upload can set and sees it travel).
static_assert(sizeof(KpsetView) == 14 * sizeof(void *) + 2 * sizeof(int), "KpsetView has changed: carry the new field through k_kfm_merge_list (and KfmMerge's q_* regions)");

// where a call's pairs lie: the result block of the last slam_kfmap_local_map_match (hn == nullptr; stride = cap pairs per stream), or the caller's,
// uploaded: hn[s] pairs from pair hoff[s] on
struct KfmPairs { const int32_t *status, *rn; const int64_t *rpairs; int stride; const int32_t *hn, *hoff; const int64_t *hpairs; };
__device__ __forceinline__ int kfm_pairs_of(const KfmPairs &P, int s, const int64_t *&p)
{
    if (P.hn) { p = P.hpairs + 2 * (size_t)P.hoff[s]; return min(max(P.hn[s], 0), P.stride); }
    p = P.rpairs + 2 * (size_t)s * P.stride;
    return P.status[s] == 0 ? min(max(P.rn[s], 0), P.stride) : 0;
}
__device__ __forceinline__ KfmRename kfm_rename_of(const KfmMerge &G, size_t z, int cap)
{
    return {G.rn_pos + z * cap, G.rn_id + z * cap, G.rs_id + z * cap, G.rank_at + z * cap, G.kept + z * ((size_t)cap + 1)};
}
// The plan of a rebuild, by the whole workgroup: ids[0 .. n) ascending, k <= n renames in Z.pos / Z.id; live == nullptr: no tombstones (a list).
// Returns the new length.  Ends behind a barrier: Z.sid, Z.rank and Z.kept are the workgroup's to read.
__device__ __forceinline__ int kfm_rename_plan(const int64_t *ids, const uint8_t *live, int n, int k, const KfmRename &Z, int *s_w, int *s_base)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) Z.rank[i] = -1;
    if (tid == 0) *s_base = 0;
    __syncthreads();
    for (int t = tid; t < k; t += 256) {
        const int64_t id = Z.id[t];
        int r = 0;
        for (int u = 0; u < k; u++) r += Z.id[u] < id;           // the new ids of one call are all different
        Z.sid[r] = id;
        if (Z.pos[t] >= 0 && Z.pos[t] < n) Z.rank[Z.pos[t]] = r;
        if (live) { const int j = kfm_find(ids, n, id); if (j >= 0 && !live[j]) Z.rank[j] = -2; }      // the equal-id tombstone (never a renamed record: those are alive)
    }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        const int off = kfm_scan(i < n && Z.rank[i] == -1, s_w, s_base);
        if (i < n) Z.kept[i] = off;
    }
    const int total = *s_base;
    if (tid == 0) Z.kept[n] = total;
    __syncthreads();
    return total + k;
}
// where record i goes (-1: dropped) and the id it carries there
__device__ __forceinline__ int kfm_rename_dest(const int64_t *ids, int n, int k, const KfmRename &Z, int i, int64_t &id)
{
    const int r = Z.rank[i];
    if (r == -2) return -1;
    if (r == -1) { id = ids[i]; return Z.kept[i] + kfm_lower(Z.sid, k, id); }
    id = Z.sid[r];
    return r + Z.kept[kfm_lower(ids, n, id)];
}

// One 256-thread workgroup per stream with pairs.  The pairs of a call are one-to-one -- no prev id twice, no new id twice, no id on both sides of two
// pairs -- so every pair reads and writes table entries of its own and no atomics are needed there; only the per-slab append counters are shared (LDS).
// The slabs are read, not written: every look-up sees the map as the call found it.  gone: no live list follows (ks == NULL): prev is marked KFM_GONE.
// ROWS (the row store is on): the pair's thread also forms the union of new's and prev's rows by key (kfm_rows_union: on an equal key new's row stays,
// beyond D rows the largest keys stay and the excess is counted) -- the pair owns both entries -- and prev's keys go with the point.
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_merge_resolve(KfmView<ROWS> V, KfmMerge G, KfmPairs P, int gone, const int *sel)
{
    __shared__ int s_cnt[KFM_MAX_R + 1], s_bad, s_stat[3];
    const int s = sel[blockIdx.x], tid = threadIdx.x, R = V.R, cap = V.cap, mcap = V.mcap;
    const int64_t *pr;
    const int n = kfm_pairs_of(P, s, pr);
    const size_t pb = (size_t)s * mcap;
    if (tid <= R) s_cnt[tid] = 0;
    if (tid == 0) { s_bad = 0; s_stat[0] = 0; s_stat[1] = 0; s_stat[2] = 0; }
    __syncthreads();
    for (int t = tid; t < n; t += 256) if (kfm_pair_clashes(pr, n, t)) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                                 // (uniform) an argument error of the device form: the stream is left as it is
        for (int t = tid; t < n; t += 256) G.applied[(size_t)s * cap + t] = 0;
        if (tid <= R) G.cnt[(size_t)s * (R + 1) + tid] = 0;
        if (tid == 0) { int32_t *st = G.stat + 4 * (size_t)s; st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 1; }
        return;
    }
    const int cur = V.cur[s], r0 = cur > 0 ? (cur - 1) % R : -1;
    for (int t = tid; t < n; t += 256) {
        const int64_t prev = pr[2 * t], neu = pr[2 * t + 1];
        const size_t pe = pb + kfm_entry(prev, mcap), ne = pb + kfm_entry(neu, mcap);
        const bool ok = prev != neu && kfm_valid(V, pe, prev) && kfm_valid(V, ne, neu) && (V.pflags[ne] & KFM_3D);     // new_mp.is_3d || return
        G.applied[(size_t)s * cap + t] = ok;
        if (!ok) { atomicAdd(&s_stat[1], 1); continue; }
        unsigned long long add = 0;
        bool obs = false;
        int nr = 0;
        for (unsigned long long mm = V.pmask[pe]; mm; mm &= mm - 1) {          // (kfm_each_observer's walk, spelled out: through it this kernel loses a wave per SIMD to SGPRs)
            const int b = __ffsll((long long)mm) - 1;
            if (b >= R || !V.tag[s * R + b]) continue;
            const int i = kfm_find_live(V, s, b, prev);
            if (i < 0 || kfm_find_live(V, s, b, neu) >= 0) continue;             // update_keypoint!: no such keypoint; has_new && return false
            const int slot = atomicAdd(&s_cnt[b], 1);
            if (slot < cap) { const size_t at = ((size_t)s * (R + 1) + b) * cap + slot; G.rn_pos[at] = i; G.rn_id[at] = neu; }     // (prev ids differ: at most one rename per record)
            add |= 1ull << b; nr++;
            obs |= b == r0 && V.tag[s * R + b] == cur;
        }
        V.pmask[ne] |= add;                                      // add_keyframe_observation!
        if (obs) V.pflags[ne] |= KFM_OBS;
        const uint8_t fl = V.pflags[pe];
        V.pmask[pe] = 0; V.pflags[pe] = KFM_DEAD | (fl & KFM_GONE) | (gone ? KFM_GONE : 0);      // pop!(m.map_points, prev_id)
        if constexpr (ROWS) {                                    // map_manager.jl:410-412; a point that takes its first row is described from then on
            int32_t *pk = V.rkey + pe * V.D;
            if (kfm_rows_count(pk, V.D)) V.dhas[ne] = 1;
            const int dropped = kfm_rows_union(V.rkey + ne * V.D, V.rrow + 4 * ne * V.D, pk, V.rrow + 4 * pe * V.D, V.D);
            if (dropped) atomicAdd(&V.rdrop[s], dropped);
            kfm_rows_clear(pk, V.D);
        }
        atomicAdd(&s_stat[0], 1); atomicAdd(&s_stat[2], nr);
    }
    __syncthreads();
    if (tid <= R) G.cnt[(size_t)s * (R + 1) + tid] = tid < R ? min(s_cnt[tid], cap) : 0;
    if (tid == 0) { int32_t *st = G.stat + 4 * (size_t)s; st[0] = s_stat[0]; st[1] = s_stat[1]; st[2] = s_stat[2]; st[3] = 0; }
}

// One workgroup per (slot, stream acted on); a slab without a rename is left at once.
__global__ __launch_bounds__(256) void k_kfm_merge_slabs(KfmapView V, KfmMerge G, const int *sel)
{
    __shared__ int s_w[4], s_base;
    const int s = sel[blockIdx.y], b = blockIdx.x, tid = threadIdx.x, R = V.R, cap = V.cap;
    const size_t z = (size_t)s * (R + 1) + b, sl = ((size_t)s * R + b) * cap;
    const int n = min(V.kn[s * R + b], cap), k = min(G.cnt[z], n);
    if (k <= 0) return;                                          // (uniform)
    const KfmRename Z = kfm_rename_of(G, z, cap);
    const int64_t *ids = V.kid + sl;
    const int n2 = kfm_rename_plan(ids, V.klive + sl, n, k, Z, s_w, &s_base);
    for (int i = tid; i < n; i += 256) {
        int64_t id = 0;
        const int d = kfm_rename_dest(ids, n, k, Z, i, id);
        if (d < 0 || d >= cap) continue;
        G.t_id[sl + d] = id; G.t_upx[2 * (sl + d)] = V.kupx[2 * (sl + i)]; G.t_upx[2 * (sl + d) + 1] = V.kupx[2 * (sl + i) + 1]; G.t_live[sl + d] = V.klive[sl + i];
        if (G.kpx) { G.t_px[2 * (sl + d)] = G.kpx[2 * (sl + i)]; G.t_px[2 * (sl + d) + 1] = G.kpx[2 * (sl + i) + 1]; }        // (uniform) the raw pixel travels with the observation
    }
    __syncthreads();                                             // every read of the slab lies behind this barrier
    for (int i = tid; i < n2; i += 256) {
        V.kid[sl + i] = G.t_id[sl + i]; V.kupx[2 * (sl + i)] = G.t_upx[2 * (sl + i)]; V.kupx[2 * (sl + i) + 1] = G.t_upx[2 * (sl + i) + 1]; V.klive[sl + i] = G.t_live[sl + i];
        if (G.kpx) { G.kpx[2 * (sl + i)] = G.t_px[2 * (sl + i)]; G.kpx[2 * (sl + i) + 1] = G.t_px[2 * (sl + i) + 1]; }
    }
    if (tid == 0) V.kn[s * R + b] = n2;
}

// update_keypoint!(m.current_frame, prev_id, new_id, is_3d) for the applied pairs: a list that carries prev and not new.  The renamed slot takes new_id,
// is3d = 1 and the new point's position in the map; the record's other fields travel with it; the count is unchanged.
__global__ __launch_bounds__(256) void k_kfm_merge_list(KfmapView V, KpsetView K, KfmMerge G, KfmPairs P, const int *sel)
{
    __shared__ int s_w[4], s_base, s_k;
    const int s = sel[blockIdx.x], tid = threadIdx.x, R = V.R, cap = V.cap;
    const size_t z = (size_t)s * (R + 1) + R, lb = (size_t)s * K.cap, qb = (size_t)s * cap, pb = (size_t)s * V.mcap;
    const int n = min(K.count[s], K.cap);
    const int64_t *pr;
    const int np = kfm_pairs_of(P, s, pr);
    const KfmRename Z = kfm_rename_of(G, z, cap);
    const int64_t *ids = K.id + lb;
    if (tid == 0) s_k = 0;
    __syncthreads();
    for (int t = tid; t < np; t += 256) {
        if (!G.applied[qb + t]) continue;
        const int i = kfm_find(ids, n, pr[2 * t]);
        if (i < 0 || kfm_find(ids, n, pr[2 * t + 1]) >= 0) continue;
        const int slot = atomicAdd(&s_k, 1);
        if (slot < cap) { Z.pos[slot] = i; Z.id[slot] = pr[2 * t + 1]; }
    }
    __syncthreads();
    const int k = min(s_k, n);
    if (k <= 0) return;                                          // (uniform)
    (void)kfm_rename_plan(ids, nullptr, n, k, Z, s_w, &s_base);
    for (int i = tid; i < n; i += 256) {
        int64_t id = 0;
        const int d = kfm_rename_dest(ids, n, k, Z, i, id);
        if (d < 0 || d >= cap) continue;
        const size_t q = lb + i, o = qb + d;
        const bool renamed = Z.rank[i] >= 0;
        const double *X = renamed ? V.pxyz + 3 * (pb + kfm_entry(id, V.mcap)) : K.xyz + 3 * q;
        G.q_yx[2 * o] = K.yx[2 * q]; G.q_yx[2 * o + 1] = K.yx[2 * q + 1]; G.q_syx[2 * o] = K.syx[2 * q]; G.q_syx[2 * o + 1] = K.syx[2 * q + 1];
        G.q_xyz[3 * o] = X[0]; G.q_xyz[3 * o + 1] = X[1]; G.q_xyz[3 * o + 2] = X[2]; G.q_id[o] = id; G.q_is3d[o] = renamed ? (uint8_t)1 : K.is3d[q]; G.q_stereo[o] = K.stereo[q];
        G.q_kyx[2 * o] = K.kyx[2 * q]; G.q_kyx[2 * o + 1] = K.kyx[2 * q + 1]; G.q_haskf[o] = K.haskf[q]; G.q_fyx[2 * o] = K.fyx[2 * q]; G.q_fyx[2 * o + 1] = K.fyx[2 * q + 1]; G.q_fkf[o] = K.fkf[q];
    }
    __syncthreads();                                             // every read of the list lies behind this barrier
    for (int i = tid; i < n; i += 256) {
        const size_t q = lb + i, o = qb + i;
        K.yx[2 * q] = G.q_yx[2 * o]; K.yx[2 * q + 1] = G.q_yx[2 * o + 1]; K.syx[2 * q] = G.q_syx[2 * o]; K.syx[2 * q + 1] = G.q_syx[2 * o + 1];
        K.xyz[3 * q] = G.q_xyz[3 * o]; K.xyz[3 * q + 1] = G.q_xyz[3 * o + 1]; K.xyz[3 * q + 2] = G.q_xyz[3 * o + 2]; K.id[q] = G.q_id[o]; K.is3d[q] = G.q_is3d[o]; K.stereo[q] = G.q_stereo[o];
        K.kyx[2 * q] = G.q_kyx[2 * o]; K.kyx[2 * q + 1] = G.q_kyx[2 * o + 1]; K.haskf[q] = G.q_haskf[o]; K.fyx[2 * q] = G.q_fyx[2 * o]; K.fyx[2 * q + 1] = G.q_fyx[2 * o + 1]; K.fkf[q] = G.q_fkf[o];
    }
}

// every region of the merge's scratch allocation, each named once (kfmap.hpp has the formula)
static size_t kfmap_merge_regions(slam_kfmap *km, char *base)
{
    Layout Lo;
    const KfmapView &v = km->v;
    KfmMerge &g = km->mg;
    const size_t S = v.S, cap = v.cap, Z = S * ((size_t)v.R + 1), n = S * v.R * cap, l = S * cap;
    Lo.bind(g.cnt, Z * 4, base); Lo.bind(g.rn_pos, Z * cap * 4, base); Lo.bind(g.rn_id, Z * cap * 8, base); Lo.bind(g.rs_id, Z * cap * 8, base); Lo.bind(g.rank_at, Z * cap * 4, base); Lo.bind(g.kept, Z * (cap + 1) * 4, base);
    Lo.bind(g.t_id, n * 8, base); Lo.bind(g.t_upx, n * 16, base); Lo.bind(g.t_live, n, base);
    Lo.bind(g.applied, l, base); Lo.bind(g.stat, S * 16, base);
    Lo.bind(g.q_yx, l * 16, base); Lo.bind(g.q_syx, l * 16, base); Lo.bind(g.q_xyz, l * 24, base); Lo.bind(g.q_kyx, l * 16, base); Lo.bind(g.q_fyx, l * 16, base); Lo.bind(g.q_id, l * 8, base);
    Lo.bind(g.q_is3d, l, base); Lo.bind(g.q_stereo, l, base); Lo.bind(g.q_haskf, l, base); Lo.bind(g.q_fkf, l * 4, base);
    if (km->kpx) Lo.bind(g.t_px, n * 16, base); else g.t_px = nullptr;           // last: every other region lies where it did without the store
    g.kpx = km->kpx;
    return Lo.size();
}

extern "C" {

int slam_kfmap_merge(slam_ctx *ctx, slam_kfmap *km, slam_kpset *ks, const int32_t *n_pairs, const int64_t *pairs, int32_t *merged)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && (ks == nullptr || (ks->S == km->v.S && ks->v.cap <= km->v.cap)));
    const KfmapView &V = km->v;
    const int S = V.S;
    int np[128], off[128];
    long long total = 0;
    // every check, for every stream, before anything is enqueued
    if (n_pairs) {
        for (int s = 0; s < S; s++) {
            if (n_pairs[s] < 0 || n_pairs[s] > V.cap) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_merge: stream %d: %d pairs (0 .. cap = %d)", s, (int)n_pairs[s], V.cap);
            np[s] = n_pairs[s]; off[s] = (int)total; total += np[s];
        }
        if (total > 0 && pairs == nullptr) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_merge: %lld pairs announced, none given", total);
        std::vector<int64_t> a, b, both;
        for (int s = 0; s < S; s++) {                            // one-to-one (kfm_sorted_one_to_one: the rule k_kfm_merge_resolve checks pair by pair)
            a.clear(); b.clear(); both.clear();
            for (int t = 0; t < np[s]; t++) {
                const int64_t p = pairs[2 * ((size_t)off[s] + t)], q = pairs[2 * ((size_t)off[s] + t) + 1];
                a.push_back(p); b.push_back(q);
                if (p != q) { both.push_back(p); both.push_back(q); }
            }
            std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end()); std::sort(both.begin(), both.end());
            if (!kfm_sorted_one_to_one(a.data(), b.data(), np[s], both.data(), (int)both.size()))
                return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_merge: the pairs of stream %d are not one-to-one (a repeated prev id, a repeated new id, or an id on both sides)", s);
        }
    } else {
        if (!km->dbase) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_merge: descriptors are not enabled (slam_kfmap_enable_descriptors): there is no local-map match whose pairs to take");
        if (!km->lm_base) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_merge: no slam_kfmap_local_map_match has run: there are no pairs to take");
        for (int s = 0; s < S; s++) { np[s] = km->lm_np[s]; off[s] = 0; total += np[s]; }
    }
    for (int s = 0; s < S; s++)                                  // the reference merges under optimization_lock
        if (np[s] > 0 && km->pend[s].valid)
            return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_merge: stream %d has pairs and a pending local-BA window (slam_kfmap_ba_update first)", s);
    if (merged) memset(merged, 0, (size_t)S * 16);
    int list[128], ns = 0;
    for (int s = 0; s < S; s++) if (np[s] > 0) list[ns++] = s;
    if (ns == 0) return SLAM_OK;                                 // no stream has pairs: nothing is enqueued
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!km->mg_base) {
        km->mg_bytes = kfmap_merge_regions(km, nullptr);
        HIP_TRY(ctx, hipMalloc((void **)&km->mg_base, km->mg_bytes));
        kfmap_merge_regions(km, km->mg_base);
    }
    const KfmMerge &G = km->mg;
    Layout D;
    const auto o_sel = D.take<int>(S), o_n = D.take<int>(S), o_off = D.take<int>(S); const auto o_pairs = D.take<int64_t>(n_pairs ? 2 * (size_t)total : 0);
    char *scr, *h;
    int rc = kfmap_upload(ctx, km, D.size(), &scr, [&](char *h) {
        kfmap_put_streams(o_sel, h, list, ns); memcpy(o_n.at(h), np, (size_t)S * 4); memcpy(o_off.at(h), off, (size_t)S * 4);
        if (n_pairs && total > 0) memcpy(o_pairs.at(h), pairs, o_pairs.bytes());
    });
    if (rc) return rc;
    KfmPairs P = {km->lm.status, km->lm.rn, km->lm.rpairs, V.cap, nullptr, nullptr, nullptr};
    if (n_pairs) P = {nullptr, nullptr, nullptr, V.cap, (const int32_t *)o_n.at(scr), (const int32_t *)o_off.at(scr), (const int64_t *)o_pairs.at(scr)};
    const int *sel = o_sel.at(scr);
    { ProfScope span(ctx, "kfmap_merge");
      { ProfScope part(ctx, "kfmap_merge_resolve");
        KFM_LAUNCH_ROWS(km, k_kfm_merge_resolve, dim3(ns), G, P, ks ? 0 : 1, sel); }
      { ProfScope part(ctx, "kfmap_merge_slabs");
        hipLaunchKernelGGL(k_kfm_merge_slabs, dim3(V.R, ns), dim3(256), 0, ctx->stream, V, G, sel); }
      if (ks) { ProfScope part(ctx, "kfmap_merge_list");
        hipLaunchKernelGGL(k_kfm_merge_list, dim3(ns), dim3(256), 0, ctx->stream, V, ks->v, G, P, sel); } }
    HIP_TRY(ctx, hipGetLastError());
    if (!n_pairs) memset(km->lm_np, 0, sizeof km->lm_np);        // consumed: the same pairs are not applied twice
    if (!merged) return SLAM_OK;
    rc = slam_pinned(ctx, (size_t)S * 16, (void **)&h);
    if (rc) return rc;
    rc = kpset_read_back(ctx, h, {{0, G.stat, (size_t)S * 16, nullptr}});
    if (rc) return rc;
    for (int k = 0; k < ns; k++) memcpy(merged + 4 * (size_t)list[k], h + 16 * (size_t)list[k], 16);          // (a stream without pairs keeps its zeros)
    return SLAM_OK;
}

}  // extern "C"
