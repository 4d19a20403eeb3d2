// kfmap_lmm.inc -- part of kfmap.hip: the descriptor store of the key-frame map and the device staging of the mapper's local-map match
// (update_frame_covisibility! map_manager.jl:302-355 + match_local_map! / do_local_map_matching mapper.jl:265-383) from the map itself.  The stager
// writes the packed buffer of k_lmm_match (lmm_host.hpp's regions, fixed per-stream strides: kfmap.hpp has the layout, its cost and the deviations),
// the match kernel of localmap.hip runs on it unchanged (lmm_launch), a closing pass turns the keypoints' keys into id pairs.  Between the upload of the
// call's arguments and the one copy of results nothing returns to the host.  tests/np_kfmap_local_map.py is the model.  With the local-map history
// (slam_kfmap_enable_local_map_history) the stager also keeps frame.local_map_ids per key-frame: kfm_lm_history below, tests/np_kfmap_local_map_history.py.
// The stager's serial decisions (kfm_rank_slots, kfm_oldest_covisible, kfm_history_rule) are kfmap_ring.hpp's, the frame constants lmm_host.hpp's lmm_frame.

// ---- descriptors: slot-parallel, one thread per appended keypoint (grid.y = stream) ---------------------------------------------------------------------
// row j of stream s belongs to id info[2 s] + j (slam_kpset_detect_describe); it is stored where the table entry carries that id
// ROWS: the row also goes into the row store under the key of the stream's newest key-frame (add_mappoint!'s current_keyframe_id)
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_desc_record(KfmView<ROWS> V, const uint64_t *desc, const int64_t *info, int dcap, const int *sel)
{
    const int s = KFM_STREAM(blockIdx.y), j = blockIdx.x * 256 + threadIdx.x;
    const int64_t n = info[2 * s + 1];
    if (j >= dcap || (int64_t)j >= n) return;
    const int64_t id = info[2 * s] + j;
    const size_t pe = (size_t)s * V.mcap + kfm_entry(id, V.mcap);
    if (!kfm_owned(V, pe, id)) return;                                          // a larger id holds the entry (or the id was never recorded): no point, no descriptor
    const uint64_t *src = desc + 4 * ((size_t)s * dcap + j);
    for (int k = 0; k < 4; k++) V.ddesc[4 * pe + k] = src[k];
    V.dhas[pe] = 1;
    if constexpr (ROWS) {
        const int dropped = kfm_rows_put(V.rkey + pe * V.D, V.rrow + 4 * pe * V.D, V.D, V.cur[s], src);
        if (dropped) atomicAdd(&V.rdrop[s], dropped);
    }
}

// ---- the local-map history (slam_kfmap_enable_local_map_history): frame.local_map_ids kept between key-frames -------------------------------------------
// Called by the whole workgroup of stream s once `mark` holds C, the local map of this key-frame's covisibility pass.  A wave takes 64 consecutive table
// entries at a time -- one word of every bitset: a ballot turns per-entry facts into that word, lane b holds the word of slot b's set (the R words of one
// entry group are adjacent: one coalesced access).  Two sweeps over the table, a barrier between them (tests/np_kfmap_local_map_history.py is the model):
//   sweep 1   purge: an entry whose tag differs from the shadow (its owner changed since the stream's last call) loses its bit in all R sets and the
//             shadow follows; the sizes of C, of P (the set stored for this key-frame, if the slot's set is its own) and of P | C
//   rule      map_manager.jl:350-354: L = C if 2 |C| > |P| else P | C; the chain (mapper.jl:274-286) runs if a key-frame is covisible and |L| < max_local,
//             with the set of the covisible key-frame of the smallest id if that slot's set is that key-frame's
//   sweep 2   L, word by word, is stored as this key-frame's set; `mark` becomes L's entries that pass the gates now (alive, 3-D, described, not
//             observed by this key-frame) -- what the ascending emission below reads
__device__ __forceinline__ unsigned long long kfm_shfl64(unsigned long long v, int lane)
{
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, lane, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), lane, 64);
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ void kfm_lm_history(const KfmapView &V, const KfmLm &Q, const KfmHist &Hs, int s, int kfid, int r0, unsigned long long covmask,
                                               const int *s_tag)
{
    __shared__ int s_len[3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, R = V.R, mcap = V.mcap;
    const size_t pb = (size_t)s * mcap;
    unsigned long long *H = Hs.bits + (size_t)s * Hs.W * R;
    int *htag = Hs.htag + s * R;
    const bool own = htag[r0] == kfid + 1;                                      // the slot's set is this key-frame's: the match runs again for it
    const int oldest = kfm_oldest_covisible(covmask, s_tag);                    // the covisible key-frame with the smallest id
    const bool linked = oldest >= 0 && htag[oldest] == s_tag[oldest];
    if (tid < 3) s_len[tid] = 0;
    __syncthreads();                                                            // (also: every thread has read htag[r0] before it is written below)
    int nC = 0, nP = 0, nU = 0;
    for (int e0 = wv * 64; e0 < mcap; e0 += 256) {
        const int e = e0 + lane, w = e0 >> 6;
        bool changed = false, inC = false;
        if (e < mcap) {
            const unsigned long long t = V.ptag[pb + e];
            changed = t != Hs.shadow[pb + e];
            if (changed) Hs.shadow[pb + e] = t;
            inC = Q.mark[pb + e] != 0;
        }
        const unsigned long long chg = __ballot(changed), cw = __ballot(inC);
        unsigned long long h = 0;
        if (lane < R) {
            h = H[(size_t)w * R + lane];
            if (h & chg) { h &= ~chg; H[(size_t)w * R + lane] = h; }
        }
        const unsigned long long pw = own ? kfm_shfl64(h, r0) : 0ull;
        nC += __popcll(cw); nP += __popcll(pw); nU += __popcll(pw | cw);
    }
    if (lane == 0) { atomicAdd(&s_len[0], nC); atomicAdd(&s_len[1], nP); atomicAdd(&s_len[2], nU); }
    __syncthreads();
    bool replace, chain;
    (void)kfm_history_rule(s_len[0], s_len[1], s_len[2], covmask, linked, Q.max_local, replace, chain);
    for (int e0 = wv * 64; e0 < mcap; e0 += 256) {
        const int e = e0 + lane, w = e0 >> 6;
        const unsigned long long cw = __ballot(e < mcap && Q.mark[pb + e] != 0);
        unsigned long long lw = cw;                                             // (every lane computes the word: uniform loads)
        if (own && !replace) lw |= H[(size_t)w * R + r0];
        if (chain) lw |= H[(size_t)w * R + oldest];
        if (lane == 0) H[(size_t)w * R + r0] = lw;
        if (e < mcap) {
            const size_t pe = pb + e;
            const bool in = (lw >> lane & 1) && V.ptag[pe] != 0 && !(V.pflags[pe] & KFM_DEAD) && (V.pflags[pe] & KFM_3D) && V.dhas[pe] && !(V.pmask[pe] >> r0 & 1);
            Q.mark[pe] = in ? 1 : 0;
        }
    }
    if (tid == 0) htag[r0] = kfid + 1;
    __syncthreads();
}

// ---- staging: one 256-thread workgroup per stream, no workgroup waits for another ------------------------------------------------------------------------
//   covisibility   kfm_covisibility over the newest key-frame's slab (the gather's and the filter's): nb_3d and the score of every other valid slot; the
//                  covisible key-frames are the slots with a score
//   mark           per covisible slab a pass over its live observations: the entry of an owned, 3-D point with a descriptor that the newest key-frame does
//                  not observe is marked (every writer writes 1: the per-entry mark is the deduplication)
//   local map      ascending by id: ids of one quotient id / mcap ascend with the entry, so the marked entries are emitted quotient by quotient, each an
//                  ordered compaction over the table (ordered_slot); the quotients present are found by a minimum search (one LDS atomicMin per pass).  Few
//                  quotients are alive at a time (ids are consecutive, the ring bounds a point's life)
//   points         per local-map point its position, descriptor and observers (mask bits whose tag matches, ascending by key-frame id); the observer
//                  offsets are a scan of the counts (kfm_scan)
//   keypoints      ordered compaction of the newest slab's live observations whose point has a descriptor; per observer the pixel by binary search in that
//                  slab (kfm_find_live), a missing or dead observation skipped (mapper.jl:429-434 without the clean-up).  Pixels come from Q.px_src: the
//                  raw pixels where the map keeps them (slam_kfmap_enable_pixels), else the undistorted ones
//   key-frames     row = rank of the slot by key-frame id; Tcw from theta by angles_to_pose
//   cells          lmm_emit's stable counting sort: counts by global atomics of this workgroup alone, offsets by kfm_scan, then the keypoints in chunks of
//                  256 in list order -- a keypoint's place is its cell's cursor plus the chunk's earlier keypoints of the same cell
// status: 0 staged, 1 nothing to match (no key-frame, no covisible key-frame, an empty local map or keypoint list), 2 the local map exceeds max_local
// (nothing of it is used).  A stream that is not staged gets M = 0 in its LmmStream row: every group of the match kernel leaves at once.
// ROWS (the row store is on): a record's descriptors are its point's rows ascending by key, kp_doff / mp_doff a scan of the row counts (kfm_scan, beside
// the observers'), a stream's rows packed from row s N1 DR / s M1 DR of kp_desc / mp_desc on; a described point without a row has an empty range.
template <bool HIST, bool ROWS>
__device__ __forceinline__ void kfm_lm_stage_body(const KfmView<ROWS> &V, const KfmLm &Q, const KfmHist &Hs, const KfmLmArg *args, const int *sel)
{
    __shared__ int s_cov[64], s_tag[64], s_rank[64], s_asc[64], s_w[4], s_cell[256], s_base, s_obase, s_nb3, s_nv;
    __shared__ unsigned long long s_covmask, s_q;
    __shared__ int s_dbase;
    const int z = blockIdx.x, s = sel[z], tid = threadIdx.x, R = V.R, cap = V.cap, mcap = V.mcap;
    LmmStream &T = Q.st[z];
    const KfmLmArg &A = args[s];
    const size_t pb = (size_t)s * mcap;
    const int kp0 = s * Q.N1, mp0 = s * Q.M1, kf0 = s * R, cell0 = s * Q.C1, kobs0 = s * Q.N1 * R, mobs0 = s * Q.M1 * R;
#define KFM_LM_LEAVE(code) { if (tid == 0) { T.N = 0; T.M = 0; T.K = 0; Q.status[s] = (code); Q.rn[s] = 0; Q.cnt[2 * s] = 0; Q.cnt[2 * s + 1] = 0; } return; }
    if (tid < 64) { s_cov[tid] = 0; s_rank[tid] = 0; s_asc[tid] = 0; s_tag[tid] = tid < R ? V.tag[s * R + tid] : 0; }
    if (tid == 0) { s_base = 0; s_obase = 0; s_nb3 = 0; s_nv = 0; s_covmask = 0; }
    if constexpr (ROWS) { if (tid == 0) s_dbase = 0; }
    __syncthreads();
    // (ROWS) the rows of entry pe, ascending by key, to dst; returns their number
    [[maybe_unused]] auto rows_out = [&](size_t pe, uint64_t *dst) {
        int n = 0;
        if constexpr (ROWS) {
            const int32_t *rk = V.rkey + pe * V.D;
            for (int j = kfm_rows_next(rk, V.D, 0); j >= 0; j = kfm_rows_next(rk, V.D, rk[j]), n++)
                for (int k = 0; k < 4; k++) dst[4 * (size_t)n + k] = V.rrow[4 * (pe * V.D + j) + k];
        }
        return n;
    };
    const int kfid = V.cur[s] - 1;
    if (kfid < 0) KFM_LM_LEAVE(1)                                               // (every branch that leaves is uniform over the workgroup)
    const int r0 = kfid % R;
    {
        const int nb3 = kfm_covisibility(V, s, r0, s_tag, s_cov);
        if (nb3) atomicAdd(&s_nb3, nb3);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long cov = 0;
        for (int b = 0; b < R; b++) if (s_tag[b] && b != r0 && s_cov[b] > 0) cov |= 1ull << b;
        s_covmask = cov; s_nv = kfm_rank_slots(s_tag, R, s_rank, s_asc);
    }
    for (int e = tid; e < mcap; e += 256) Q.mark[pb + e] = 0;
    __syncthreads();
    const unsigned long long covmask = s_covmask;
    const int nv = s_nv, nb3 = s_nb3;
    if (!HIST && covmask == 0) KFM_LM_LEAVE(1)
    for (unsigned long long cm = covmask; cm; cm &= cm - 1) {
        const int b = __ffsll((long long)cm) - 1, n = min(V.kn[s * R + b], cap);
        for (int i = tid; i < n; i += 256) {
            int64_t id;
            size_t pe;
            if (!kfm_slab_point(V, s, b, i, id, pe) || !kfm_valid(V, pe, id) || !(V.pflags[pe] & KFM_3D) || !V.dhas[pe] || (V.pmask[pe] >> r0 & 1)) continue;
            Q.mark[pe] = 1;
        }
    }
    __syncthreads();
    if constexpr (HIST) kfm_lm_history(V, Q, Hs, s, kfid, r0, covmask, s_tag);
    // the local map, ascending by id
    for (unsigned long long qlo = 0;;) {
        if (tid == 0) s_q = ~0ull;
        __syncthreads();
        unsigned long long lmin = ~0ull;
        for (int e = tid; e < mcap; e += 256)
            if (Q.mark[pb + e]) { const unsigned long long q = (V.ptag[pb + e] - 1ull) / (unsigned long long)mcap; if (q >= qlo && q < lmin) lmin = q; }
        if (lmin != ~0ull) atomicMin(&s_q, lmin);
        __syncthreads();
        const unsigned long long q = s_q;
        if (q == ~0ull) break;
        for (int e0 = 0; e0 < mcap; e0 += 256) {
            const int e = e0 + tid;
            const bool acc = e < mcap && Q.mark[pb + e] && (V.ptag[pb + e] - 1ull) / (unsigned long long)mcap == q;
            const int pos = ordered_slot(acc, s_w, &s_base);                     // (its barriers also fence s_q: read above, reset below)
            if (acc && pos < Q.max_local) Q.mp_id[mp0 + pos] = (int64_t)(V.ptag[pb + e] - 1ull);
        }
        qlo = q + 1ull;
    }
    const int M = s_base;
    __syncthreads();
    if (M > Q.max_local) KFM_LM_LEAVE(2)
    if (M == 0) KFM_LM_LEAVE(1)
    for (int m0 = 0; m0 < M; m0 += 256) {
        const int m = m0 + tid;
        unsigned long long wm = 0;
        size_t pe = 0;
        if (m < M) {
            pe = pb + kfm_entry(Q.mp_id[mp0 + m], mcap);
            kfm_each_observer(V.pmask[pe], s_tag, R, [&](int b) { wm |= 1ull << b; });
        }
        const int off = kfm_scan(__popcll(wm), s_w, &s_obase);
        int doff = 0;
        if constexpr (ROWS) doff = kfm_scan(m < M ? kfm_rows_count(V.rkey + pe * V.D, V.D) : 0, s_w, &s_dbase);
        if (m < M) {
            const size_t g = (size_t)mp0 + m;
            for (int k = 0; k < 3; k++) Q.mp_xyz[3 * g + k] = V.pxyz[3 * pe + k];
            if constexpr (ROWS) { Q.mp_doff[g] = mp0 * Q.DR + doff; (void)rows_out(pe, Q.mp_desc + 4 * ((size_t)mp0 * Q.DR + doff)); }
            else { for (int k = 0; k < 4; k++) Q.mp_desc[4 * g + k] = V.ddesc[4 * pe + k]; Q.mp_doff[g] = (int32_t)g; }
            Q.mp_ooff[g] = mobs0 + off;
            int j = 0;
            for (int k = 0; k < nv; k++) if (wm >> s_asc[k] & 1) Q.mp_okf[(size_t)mobs0 + off + j++] = k;
        }
    }
    if (tid == 0) {
        if constexpr (ROWS) { Q.mp_doff[mp0 + M] = mp0 * Q.DR + s_dbase; s_dbase = 0; } else Q.mp_doff[mp0 + M] = mp0 + M;
        Q.mp_ooff[mp0 + M] = mobs0 + s_obase; s_base = 0; s_obase = 0;
    }
    __syncthreads();
    // the keypoints: the newest slab, in slab order
    {
        const size_t sl = ((size_t)s * R + r0) * cap;
        const int n0 = min(V.kn[s * R + r0], cap);
        for (int c0 = 0; c0 < n0; c0 += 256) {
            const int i = c0 + tid;
            bool acc = false;
            int64_t id = 0;
            size_t pe = 0;
            unsigned long long wm = 0;
            if (i < n0 && kfm_slab_point(V, s, r0, i, id, pe)) acc = kfm_valid(V, pe, id) && V.dhas[pe];
            if (acc) wm = kfm_live_observers(V, s, V.pmask[pe], s_tag, id);
            const int pos = ordered_slot(acc, s_w, &s_base);
            const int off = kfm_scan(__popcll(wm), s_w, &s_obase);
            int doff = 0;
            if constexpr (ROWS) doff = kfm_scan(acc ? kfm_rows_count(V.rkey + pe * V.D, V.D) : 0, s_w, &s_dbase);
            if (acc) {
                const size_t g = (size_t)kp0 + pos;
                Q.kp_id[g] = id; Q.kp_yx[2 * g] = Q.px_src[2 * (sl + i)]; Q.kp_yx[2 * g + 1] = Q.px_src[2 * (sl + i) + 1];
                if constexpr (ROWS) { Q.kp_doff[g] = kp0 * Q.DR + doff; (void)rows_out(pe, Q.kp_desc + 4 * ((size_t)kp0 * Q.DR + doff)); }
                else { for (int k = 0; k < 4; k++) Q.kp_desc[4 * g + k] = V.ddesc[4 * pe + k]; Q.kp_doff[g] = (int32_t)g; }
                Q.kp_ooff[g] = kobs0 + off;
                size_t o = (size_t)kobs0 + off;
                for (int k = 0; k < nv; k++) {
                    const int b = s_asc[k];
                    if (!(wm >> b & 1)) continue;
                    const size_t qo = ((size_t)s * R + b) * cap + max(kfm_find_live(V, s, b, id), 0);      // (found: validated above)
                    Q.kp_okf[o] = k; Q.kp_oyx[2 * o] = Q.px_src[2 * qo]; Q.kp_oyx[2 * o + 1] = Q.px_src[2 * qo + 1];
                    o++;
                }
            }
        }
    }
    const int N = s_base;
    if (tid == 0) {
        if constexpr (ROWS) Q.kp_doff[kp0 + N] = kp0 * Q.DR + s_dbase; else Q.kp_doff[kp0 + N] = kp0 + N;
        Q.kp_ooff[kp0 + N] = kobs0 + s_obase;
    }
    __syncthreads();
    if (N == 0) KFM_LM_LEAVE(1)
    if (tid < R && s_tag[tid]) kfm_tcw(V.ktheta + 6 * ((size_t)s * R + tid), Q.kf_Tcw + 16 * (size_t)(kf0 + s_rank[tid]));
    // the cell lists (lmm_emit's counting sort)
    const int cells = A.gr * A.gc;
    int32_t *co = Q.cell_off + cell0, *cc = Q.cell_cur + cell0, *ck = Q.cell_kp + kp0;
    auto cell_of = [&](int j) -> int {
        const long long r = lmm_cell(Q.kp_yx[2 * ((size_t)kp0 + j)], A.cell), c = lmm_cell(Q.kp_yx[2 * ((size_t)kp0 + j) + 1], A.cell);
        return r >= 1 && r <= A.gr && c >= 1 && c <= A.gc ? (int)((r - 1) * A.gc + (c - 1)) : -1;
    };
    for (int c = tid; c <= cells; c += 256) co[c] = 0;
    if (tid == 0) s_obase = 0;
    __syncthreads();
    for (int j = tid; j < N; j += 256) { const int c = cell_of(j); if (c >= 0) atomicAdd(&co[c + 1], 1); }
    __syncthreads();
    for (int c0 = 0; c0 < cells; c0 += 256) {
        const int c = c0 + tid, cnt = c < cells ? co[c + 1] : 0;
        const int off = kfm_scan(cnt, s_w, &s_obase);
        if (c < cells) { co[c + 1] = off + cnt; cc[c] = off; }
    }
    __syncthreads();
    for (int c0 = 0; c0 < N; c0 += 256) {
        const int j = c0 + tid, c = j < N ? cell_of(j) : -1;
        s_cell[tid] = c;
        __syncthreads();
        if (c >= 0) {
            int before = 0;
            for (int k = 0; k < tid; k++) before += s_cell[k] == c;
            ck[cc[c] + before] = j;
        }
        __syncthreads();
        if (c >= 0) atomicAdd(&cc[c], 1);
        __syncthreads();
    }
    if (tid == 0) {
        kfm_tcw(V.ktheta + 6 * ((size_t)s * R + r0), T.Tcw);
        T.fx = A.cam[0]; T.fy = A.cam[1]; T.cx = A.cam[2]; T.cy = A.cam[3]; T.k1 = A.cam[4]; T.k2 = A.cam[5]; T.p1 = A.cam[6]; T.p2 = A.cam[7];
        T.H = A.cam[8]; T.W = A.cam[9];
        T.max_proj = nb3 < 30 ? A.max_proj * 2.0 : A.max_proj;                   // mapper.jl:332, nb_3d from the slab
        T.start = A.start; T.view_thr = A.view_thr;
        T.cell = A.cell; T.gr = A.gr; T.gc = A.gc;
        T.N = N; T.M = M; T.K = nv; T.kp0 = kp0; T.kf0 = kf0; T.mp0 = mp0; T.cell0 = cell0;
        Q.status[s] = 0; Q.cnt[2 * s] = N; Q.cnt[2 * s + 1] = M;
    }
#undef KFM_LM_LEAVE
}
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_lm_stage(KfmView<ROWS> V, KfmLm Q, const KfmLmArg *args, const int *sel)
{
    kfm_lm_stage_body<false, ROWS>(V, Q, KfmHist{}, args, sel);
}
// the same stager for a map with the local-map history: `mark` comes out of kfm_lm_history, and a stream without a covisible key-frame is still staged
// (its stored set may hold points)
template <bool ROWS> __global__ __launch_bounds__(256) void k_kfm_lm_stage_hist(KfmView<ROWS> V, KfmLm Q, KfmHist Hs, const KfmLmArg *args, const int *sel)
{
    kfm_lm_stage_body<true, ROWS>(V, Q, Hs, args, sel);
}

// prev_new_map (mapper.jl:370-382) as id pairs: ordered compaction of the keypoints somebody chose, in list order = ascending keypoint id
__global__ __launch_bounds__(256) void k_kfm_lm_pairs(KfmapView V, KfmLm Q, const int *sel)
{
    __shared__ int s_w[4], s_base;
    const int s = sel[blockIdx.x], tid = threadIdx.x;
    if (Q.status[s] != 0) return;                                               // (uniform; the stager has written rn = 0)
    const int N = Q.cnt[2 * s], kp0 = s * Q.N1, mp0 = s * Q.M1;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < N; c0 += 256) {
        const int j = c0 + tid;
        const unsigned long long key = j < N ? Q.keys[kp0 + j] : ~0ull;
        const int m = lmm_decode(key);
        const int pos = ordered_slot(m >= 0, s_w, &s_base);
        if (m >= 0) {
            const size_t o = (size_t)s * V.cap + pos;
            Q.rpairs[2 * o] = Q.kp_id[kp0 + j]; Q.rpairs[2 * o + 1] = Q.mp_id[mp0 + m]; Q.rdist[o] = (double)(key >> 32);
        }
    }
    if (tid == 0) Q.rn[s] = s_base;
}

// the descriptor store's and the history's regions, each named once (kfmap.hpp has the formulas)
static size_t kfmap_desc_regions(slam_kfmap *km, char *base)
{
    Layout Lo;
    const size_t m = (size_t)km->v.S * km->v.mcap;
    Lo.bind(km->v.ddesc, m * 32, base); Lo.bind(km->v.dhas, m, base);
    return Lo.size();
}
static size_t kfmap_hist_regions(slam_kfmap *km, char *base)
{
    Layout Lo;
    const KfmapView &v = km->v;
    KfmHist &hs = km->hs;
    const size_t W = ((size_t)v.mcap + 63) / 64;
    Lo.bind(hs.bits, (size_t)v.S * W * v.R * 8, base); Lo.bind(hs.htag, (size_t)v.S * v.R * 4, base); Lo.bind(hs.shadow, (size_t)v.S * v.mcap * 8, base);
    if (base) hs.W = (int)W;
    return Lo.size();
}
// the row store's regions, each named once (kfmap.hpp has the formula)
static size_t kfmap_rows_regions(slam_kfmap *km, int D, char *base)
{
    Layout Lo;
    const size_t m = (size_t)km->v.S * km->v.mcap;
    Lo.bind(km->v.rkey, m * D * 4, base); Lo.bind(km->v.rrow, m * D * 32, base); Lo.bind(km->v.rdrop, (size_t)km->v.S * 4, base);
    return Lo.size();
}
// every region of the staging allocation, each named once (kfmap.hpp has the formula); the results last, one block
static size_t kfmap_lm_regions(slam_kfmap *km, int max_local, int C1, char *base)
{
    Layout Lo;
    const KfmapView &v = km->v;
    KfmLm &q = km->lm;
    const size_t S = v.S, N1 = (size_t)v.cap + 1, M1 = (size_t)max_local + 1, n = S * N1, m = S * M1, R = v.R, DR = km->v.D ? km->v.D : 1;
    q.N1 = (int)N1; q.M1 = (int)M1; q.C1 = C1; q.max_local = max_local; q.DR = (int)DR;
    Lo.bind(q.st, S * sizeof(LmmStream), base);
    Lo.bind(q.kp_yx, n * 16, base); Lo.bind(q.kp_doff, n * 4, base); Lo.bind(q.kp_desc, n * DR * 32, base); Lo.bind(q.kp_ooff, n * 4, base); Lo.bind(q.kp_okf, n * R * 4, base); Lo.bind(q.kp_oyx, n * R * 16, base);
    Lo.bind(q.kp_id, n * 8, base); Lo.bind(q.kf_Tcw, S * R * 128, base);
    Lo.bind(q.mp_xyz, m * 24, base); Lo.bind(q.mp_doff, m * 4, base); Lo.bind(q.mp_desc, m * DR * 32, base); Lo.bind(q.mp_ooff, m * 4, base); Lo.bind(q.mp_okf, m * R * 4, base); Lo.bind(q.mp_id, m * 8, base);
    Lo.bind(q.cell_off, S * (size_t)C1 * 4, base); Lo.bind(q.cell_kp, n * 4, base); Lo.bind(q.cell_cur, S * (size_t)C1 * 4, base);
    Lo.bind(q.best_kp, m * 4, base); Lo.bind(q.best_dist, m * 8, base); Lo.bind(q.proj, m * 16, base); Lo.bind(q.keys, n * 8, base);
    Lo.bind(q.mark, S * (size_t)v.mcap * 4, base); Lo.bind(q.cnt, S * 8, base);
    km->lm_res_off = Lo.size();
    Lo.bind(q.status, S * 4, base); Lo.bind(q.rn, S * 4, base); Lo.bind(q.rpairs, S * (size_t)v.cap * 16, base); Lo.bind(q.rdist, S * (size_t)v.cap * 8, base);
    km->lm_res_bytes = Lo.size() - km->lm_res_off;
    return Lo.size();
}

extern "C" {

int slam_kfmap_enable_descriptors(slam_ctx *ctx, slam_kfmap *km, int n_bits)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr);
    if (n_bits != 256) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_enable_descriptors: n_bits = %d, the local-map match handles 256-bit descriptors only", n_bits);
    if (km->dbase) return SLAM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = kfmap_alloc_zeroed(ctx, "slam_kfmap_enable_descriptors", kfmap_desc_regions(km, nullptr), &km->dbase);
    if (rc) return rc;
    kfmap_desc_regions(km, km->dbase);
    return SLAM_OK;
}

int slam_kfmap_enable_descriptor_rows(slam_ctx *ctx, slam_kfmap *km, int max_rows)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr);
    if (!km->dbase) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_enable_descriptor_rows: descriptors are not enabled (slam_kfmap_enable_descriptors)");
    if (max_rows < 2 || max_rows > KFM_MAX_ROWS) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_enable_descriptor_rows: max_rows = %d (2 .. %d)", max_rows, KFM_MAX_ROWS);
    if (km->rbase) {
        if (km->v.D == max_rows) return SLAM_OK;
        return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_enable_descriptor_rows: max_rows = %d, but the map keeps %d rows per point", max_rows, km->v.D);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = kfmap_alloc_zeroed(ctx, "slam_kfmap_enable_descriptor_rows", kfmap_rows_regions(km, max_rows, nullptr), &km->rbase);      // zeroed: no rows
    if (rc) return rc;
    kfmap_rows_regions(km, max_rows, km->rbase);
    km->v.D = max_rows;
    if (km->lm_base) {                                           // the staging was laid out for one row per record: the next match makes it anew
        HIP_TRY(ctx, hipDeviceSynchronize());
        (void)hipFree(km->lm_base); km->lm_base = nullptr; km->lm = KfmLm{};
        memset(km->lm_np, 0, sizeof km->lm_np);
    }
    return SLAM_OK;
}

int slam_kfmap_download_descriptor_rows(slam_ctx *ctx, slam_kfmap *km, int s, int64_t *ids, uint8_t *described, int32_t *row_off, int32_t *keys, uint64_t *rows,
                                        int cap_points, int cap_rows, int32_t *n_points, int32_t *dropped)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && n_points != nullptr && cap_points >= 0 && cap_rows >= 0);
    if (!km->rbase) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_download_descriptor_rows: descriptor rows are not enabled (slam_kfmap_enable_descriptor_rows)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapRows &V = km->v;
    const size_t m = V.mcap, pb = (size_t)s * m, D = V.D;
    std::vector<unsigned long long> tag(m);
    std::vector<uint8_t> fl(m), has(m);
    std::vector<int32_t> key(m * D);
    std::vector<uint64_t> row(m * D * 4);
    int32_t drop = 0;
    HIP_TRY(ctx, hipMemcpyAsync(tag.data(), V.ptag + pb, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(fl.data(), V.pflags + pb, m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(has.data(), V.dhas + pb, m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(key.data(), V.rkey + pb * D, m * D * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(row.data(), V.rrow + pb * D * 4, m * D * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&drop, V.rdrop + s, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    std::vector<std::pair<int64_t, size_t>> live;                // the set slam_kfmap_download_points lists
    size_t nrows = 0;
    for (size_t e = 0; e < m; e++) if (tag[e] && !(fl[e] & KFM_DEAD)) { live.push_back({(int64_t)(tag[e] - 1), e}); nrows += kfm_rows_count(key.data() + e * D, (int)D); }
    std::sort(live.begin(), live.end());
    *n_points = (int32_t)live.size();
    if (dropped) *dropped = drop;
    if (live.size() > (size_t)cap_points || ((keys || rows) && nrows > (size_t)cap_rows))
        return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_kfmap_download_descriptor_rows: %zu points with %zu rows, caps %d and %d", live.size(), nrows, cap_points, cap_rows);
    int32_t at = 0;
    for (size_t k = 0; k < live.size(); k++) {
        const size_t e = live[k].second;
        const int32_t *rk = key.data() + e * D;
        if (ids) ids[k] = live[k].first;
        if (described) described[k] = has[e];
        if (row_off) row_off[k] = at;
        for (int j = kfm_rows_next(rk, (int)D, 0); j >= 0; j = kfm_rows_next(rk, (int)D, rk[j]), at++) {
            if (keys) keys[at] = rk[j] - 1;
            if (rows) memcpy(rows + 4 * (size_t)at, row.data() + 4 * (e * D + j), 32);
        }
    }
    if (row_off) row_off[live.size()] = at;
    return SLAM_OK;
}

int slam_kfmap_enable_local_map_history(slam_ctx *ctx, slam_kfmap *km)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr);
    if (km->hs_base) return SLAM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    km->hs_bytes = kfmap_hist_regions(km, nullptr);                             // zeroed: empty sets without owners; the first match brings the shadow up to the table
    const int rc = kfmap_alloc_zeroed(ctx, "slam_kfmap_enable_local_map_history", km->hs_bytes, &km->hs_base);
    if (rc) return rc;
    kfmap_hist_regions(km, km->hs_base);
    return SLAM_OK;
}

int slam_kfmap_download_local_map_ids(slam_ctx *ctx, slam_kfmap *km, int s, int kfid, int64_t *ids, int cap_ids, int32_t *n_ids)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && kfid >= 0 && n_ids != nullptr && cap_ids >= 0 && (cap_ids == 0 || ids != nullptr));
    if (!km->hs_base) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_download_local_map_ids: the local-map history is not enabled (slam_kfmap_enable_local_map_history)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmapView &V = km->v;
    const KfmHist &H = km->hs;
    const int b = kfid % V.R;
    const size_t sr = (size_t)s * V.R + b, W = (size_t)H.W;
    int tg[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&tg[0], V.tag + sr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&tg[1], H.htag + sr, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    *n_ids = 0;
    if (tg[0] != kfid + 1) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_download_local_map_ids: key-frame %d of stream %d is not in the ring", kfid, s);
    if (tg[1] != kfid + 1) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_download_local_map_ids: no local map was stored for key-frame %d of stream %d", kfid, s);
    std::vector<unsigned long long> bits(W * V.R), shadow((size_t)V.mcap);
    HIP_TRY(ctx, hipMemcpyAsync(bits.data(), H.bits + (size_t)s * W * V.R, W * V.R * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(shadow.data(), H.shadow + (size_t)s * V.mcap, (size_t)V.mcap * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    std::vector<int64_t> got;                                    // a set bit's id is the entry's tag at the store, which the shadow still holds
    for (int e = 0; e < V.mcap; e++)
        if ((bits[(size_t)(e >> 6) * V.R + b] >> (e & 63) & 1) && shadow[e]) got.push_back((int64_t)(shadow[e] - 1ull));
    std::sort(got.begin(), got.end());
    *n_ids = (int32_t)got.size();
    if (got.size() > (size_t)cap_ids) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_kfmap_download_local_map_ids: %zu ids but cap_ids = %d", got.size(), cap_ids);
    if (!got.empty()) memcpy(ids, got.data(), got.size() * 8);
    return SLAM_OK;
}

int slam_kfmap_add_descriptors(slam_ctx *ctx, slam_kfmap *km, const uint64_t *desc_dev, const int64_t *info_dev, int dcap)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && desc_dev != nullptr && info_dev != nullptr && dcap >= 1);
    if (!km->dbase) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_add_descriptors: descriptors are not enabled (slam_kfmap_enable_descriptors)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int list[128];
    const int ns = kfmap_streams(km, list);
    if (ns == 0) return SLAM_OK;
    const int *sel = nullptr;
    if (km->n_sel != KPSEL_ALL) {                                // the streams of the last add_keyframe, staged like the filter's table
        char *scr;
        const int rc = kfmap_upload(ctx, km, (size_t)ns * 4, &scr, [&](char *h) { kfmap_put_streams(Region<int>{0, (size_t)ns}, h, list, ns); });
        if (rc) return rc;
        sel = (const int *)scr;
    }
    { ProfScope span(ctx, "kfmap_add_descriptors");
      KFM_LAUNCH_ROWS(km, k_kfm_desc_record, dim3((dcap + 255) / 256, ns), desc_dev, info_dev, dcap, sel); }
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

int slam_kfmap_local_map_match(slam_ctx *ctx, slam_kfmap *km, const double *cam, const int32_t *cell_size, const double *max_projection_distance,
                               const double *max_descriptor_distance, int max_local, int32_t *status, int32_t *n_pairs, int64_t *pairs, double *dist,
                               int cap_pairs)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && cam != nullptr && cell_size != nullptr && max_projection_distance != nullptr &&
                     max_descriptor_distance != nullptr && status != nullptr && n_pairs != nullptr && max_local >= 1 && max_local <= (1 << 22) &&
                     cap_pairs >= 0 && (cap_pairs == 0 || (pairs != nullptr && dist != nullptr)));
    if (!km->dbase) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_local_map_match: descriptors are not enabled (slam_kfmap_enable_descriptors)");
    const KfmapView &V = km->v;
    const int S = V.S;
    std::vector<KfmLmArg> args((size_t)S);
    int C1 = 2;
    for (int s = 0; s < S; s++) {                                // every check, for every stream, before anything is enqueued
        const double *c = cam + 10 * (size_t)s;
        KfmLmArg &A = args[s];
        if (!km->kpx && (c[4] != 0.0 || c[5] != 0.0 || c[6] != 0.0 || c[7] != 0.0))          // (with the raw-pixel store the match reads kp.pixel: any lens)
            return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_local_map_match: stream %d has lens distortion (%g %g %g %g); the map's pixels are undistorted", s, c[4], c[5], c[6], c[7]);
        const double H = c[8], W = c[9];
        const int cell = cell_size[s];
        LmmFrame F;
        if (!lmm_frame(c, cell, max_descriptor_distance[s], F) || !(c[0] > 0.0) || !(c[1] > 0.0))
            return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_local_map_match: stream %d: cell_size %d / image %g x %g / focal lengths %g %g out of range", s, cell, H, W, c[0], c[1]);
        memcpy(A.cam, c, sizeof A.cam);
        A.max_proj = max_projection_distance[s];
        A.start = F.start; A.view_thr = F.view_thr;
        A.cell = cell; A.gr = F.gr; A.gc = F.gc; A.pad = 0;
        if ((long long)A.gr * A.gc > (1 << 22)) return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_local_map_match: stream %d: a grid of %d x %d cells", s, A.gr, A.gc);
        C1 = std::max(C1, A.gr * A.gc + 1);
    }
    if ((size_t)S * ((size_t)max_local + 1) * V.R >= ((size_t)1 << 31) || (size_t)S * ((size_t)V.cap + 1) * V.R >= ((size_t)1 << 31))
        return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_local_map_match: S (max_local + 1) R or S (cap + 1) R exceeds 2^31");
    if (km->v.D && ((size_t)S * ((size_t)max_local + 1) * km->v.D >= ((size_t)1 << 31) || (size_t)S * ((size_t)V.cap + 1) * km->v.D >= ((size_t)1 << 31)))
        return slam_fail(ctx, SLAM_ERR_ARG, "slam_kfmap_local_map_match: S (max_local + 1) D or S (cap + 1) D exceeds 2^31 descriptor rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int list[128];
    const int ns = kfmap_streams(km, list);
    for (int s = 0; s < S; s++) { status[s] = 1; n_pairs[s] = 0; km->lm_np[s] = 0; }
    if (ns == 0) return SLAM_OK;
    if (!km->lm_base || km->lm.max_local < max_local || km->lm.C1 < C1) {          // (re)made for the larger of what it had and what is asked
        const int ml = std::max(max_local, km->lm_base ? km->lm.max_local : 0), c1 = std::max(C1, km->lm_base ? km->lm.C1 : 0);
        if (km->lm_base) { HIP_TRY(ctx, hipDeviceSynchronize()); (void)hipFree(km->lm_base); km->lm_base = nullptr; }
        km->lm_bytes = kfmap_lm_regions(km, ml, c1, nullptr);
        HIP_TRY(ctx, hipMalloc((void **)&km->lm_base, km->lm_bytes));
        kfmap_lm_regions(km, ml, c1, km->lm_base);
    }
    KfmLm Q = km->lm;
    Q.max_local = max_local;                                                       // the call's bound; the strides stay the allocation's
    Q.px_src = km->kpx ? km->kpx : V.kupx;                                         // find_best_match's kp.pixel where the map keeps it
    Layout D;
    const auto o_sel = D.take<int>(S); const auto o_arg = D.take<KfmLmArg>(S); const size_t in_b = D.size();
    const size_t o_res = D.take(km->lm_res_bytes);
    char *scr, *h;
    int rc = slam_scratch(ctx, in_b, (void **)&scr);
    if (rc) return rc;
    rc = slam_pinned(ctx, D.size(), (void **)&h);
    if (rc) return rc;
    kfmap_put_streams(o_sel, h, list, ns); memcpy(o_arg.at(h), args.data(), o_arg.bytes());
    const LmmDev L = kfm_lmm_dev(Q);
    const int *sel = o_sel.at(scr);
    { ProfScope span(ctx, "kfmap_local_map_match");
      HIP_TRY(ctx, hipMemcpyAsync(scr, h, in_b, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemsetAsync(Q.keys, 0xFF, (size_t)S * Q.N1 * 8, ctx->stream));
      { ProfScope stage(ctx, "kfmap_lm_stage");
        if (km->hs_base) KFM_LAUNCH_ROWS(km, k_kfm_lm_stage_hist, dim3(ns), Q, km->hs, (const KfmLmArg *)o_arg.at(scr), sel);
        else KFM_LAUNCH_ROWS(km, k_kfm_lm_stage, dim3(ns), Q, (const KfmLmArg *)o_arg.at(scr), sel); }
      lmm_launch(ctx, L, max_local, ns);
      hipLaunchKernelGGL(k_kfm_lm_pairs, dim3(ns), dim3(256), 0, ctx->stream, V, Q, sel);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(h + o_res, km->lm_base + km->lm_res_off, km->lm_res_bytes, hipMemcpyDeviceToHost, ctx->stream)); }
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    auto result = [&](const auto *p) { return (decltype(p))(h + o_res + ((const char *)p - (km->lm_base + km->lm_res_off))); };        // a result region in the host's copy of the block
    const int32_t *st = result(Q.status), *rn = result(Q.rn);
    const int64_t *rp = result(Q.rpairs);
    const double *rd = result(Q.rdist);
    long long total = 0;
    for (int k = 0; k < ns; k++) { const int s = list[k]; status[s] = st[s]; n_pairs[s] = st[s] == 0 ? rn[s] : 0; total += n_pairs[s]; km->lm_np[s] = n_pairs[s]; }
    if (total > cap_pairs) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_kfmap_local_map_match: %lld pairs but cap_pairs = %d", total, cap_pairs);
    size_t at = 0;
    for (int k = 0; k < ns; k++) {
        const int s = list[k], n = n_pairs[s];
        if (n == 0) continue;
        memcpy(pairs + 2 * at, rp + 2 * (size_t)s * V.cap, (size_t)n * 16); memcpy(dist + at, rd + (size_t)s * V.cap, (size_t)n * 8);
        at += n;
    }
    return SLAM_OK;
}

// Test hook (not declared in slamhip.h): what the last slam_kfmap_local_map_match staged for stream s -- the local-map ids in order with the match
// kernel's proj_yx, best_kp and best_dist, and the keypoint ids in order.  counts[0] = N, counts[1] = M (0, 0 unless the stream's status was 0).
int slam_debug_kfmap_local_map(slam_ctx *ctx, slam_kfmap *km, int s, int64_t *lm_ids, double *proj_yx, int32_t *best_kp, double *best_dist, int64_t *kp_ids,
                               int cap_lm, int cap_kp, int32_t *counts)
{
    ARG_TRY(ctx, ctx != nullptr && km != nullptr && s >= 0 && s < km->v.S && counts != nullptr && km->lm_base != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KfmLm &Q = km->lm;
    HIP_TRY(ctx, hipMemcpyAsync(counts, Q.cnt + 2 * s, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    const int N = counts[0], M = counts[1];
    if (N > cap_kp || M > cap_lm) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_debug_kfmap_local_map: %d keypoints, %d points, caps %d and %d", N, M, cap_kp, cap_lm);
    const size_t kp0 = (size_t)s * Q.N1, mp0 = (size_t)s * Q.M1;
    if (N > 0 && kp_ids) HIP_TRY(ctx, hipMemcpyAsync(kp_ids, Q.kp_id + kp0, (size_t)N * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (M > 0 && lm_ids) HIP_TRY(ctx, hipMemcpyAsync(lm_ids, Q.mp_id + mp0, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (M > 0 && proj_yx) HIP_TRY(ctx, hipMemcpyAsync(proj_yx, Q.proj + 2 * mp0, (size_t)M * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (M > 0 && best_kp) HIP_TRY(ctx, hipMemcpyAsync(best_kp, Q.best_kp + mp0, (size_t)M * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (M > 0 && best_dist) HIP_TRY(ctx, hipMemcpyAsync(best_dist, Q.best_dist + mp0, (size_t)M * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    return SLAM_OK;
}

}  // extern "C"
