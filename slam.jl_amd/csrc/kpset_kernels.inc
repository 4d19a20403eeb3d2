// kpset_kernels.inc -- the three keypoint-list kernels that exist in two forms, each written once: kpset.hip includes this file twice.
//   plain     SEL_NAME(k) = k, SEL_STREAM(b) = b, SEL_STREAMS(S) = S, SEL_SELF(s) = s: workgroup (or grid row) b works on stream b, all S of them --
//             every seam without a selection, and the seams that ignore it (flow_match, remove, the pose calls: kpset.hpp)
//   selected  SEL_NAME(k) = k_sel, SEL_STREAM(b) = sel[b], SEL_STREAMS(S) = gridDim.x, SEL_SELF(s) = blockIdx.x, one more argument (SEL_ARG)
//             `const int *sel`: the ascending table of the streams slam_kpset_select names (kpset_select.hpp).  The launch is sized by their number
//             (grid.x, or grid.y of k_kpset_keyframe), so no workgroup exists for an unselected stream and nothing of it is read or written.
// An include, not a template over a shared __device__ body: the plain kernels then compile from the token sequence they had before there was a
// selection, and their code objects stay instruction for instruction what they were (profiles/r21a_select_kernel_table.txt; with an inlined body
// k_kpset_worklist came out with two operands of one instruction swapped, the detection kernels with other registers).
// (Round 22 gave k_kpset_worklist the work records of a match -- both forms, here, once: profiles/r22a_lk_kernel_table.txt has its new figures.)

// live slots of all streams back to back + their number.  One small workgroup per stream (it sums the counts before its own: S
// loads): a single 1024-thread workgroup had to wait for sixteen free wave slots on one CU while the pyramid kernels fill the chip
// (58 us on average in the pipeline for 12 us of work).
// Stream s's segment [off_s, off_s + count_s) holds its live slots; O.band > 0 sorts them by work_key (x-band, row, slot:
// work_order.hpp) with a bitonic network in LDS over the segment padded to a power of two with maximal words -- lists are queues
// of many detect generations (stable compaction, new keypoints appended behind), so slot order is not a spatial order.  Every wave
// sums the counts itself (S loads, no barrier); the sort's words are (key << 32 | slot), all different.
// Selected form: only the selected streams' segments are laid back to back and ntot is their sum, so whatever walks the list (k_kpset_match,
// both triangulation kernels) never sees a slot of an unselected stream.
// R.rec != nullptr (the caller is a match): entry off + j also gets its work record (KpWorkRec, kpset.hpp; placed by work_rec_slot, work_order.hpp).
// The record's target member zt is the stream -- or, for a compact stereo match (R.compact), SEL_SELF(s): the workgroup's index in the selected launch,
// which is the stream's rank.
__global__ __launch_bounds__(256) void SEL_NAME(k_kpset_worklist)(const int *count, int S, int cap, int *work, int *ntot, const double *yx, WorkOrder O, KpWorkRecs R SEL_ARG)
{
    extern __shared__ unsigned long long s_word[];
    const int s = SEL_STREAM(blockIdx.x), tid = threadIdx.x, lane = tid & 63;
    int off = 0, t = 0;
    for (int i = lane; i < SEL_STREAMS(S); i += 64) { const int v = count[SEL_STREAM(i)]; t += v; off += i < SEL_SELF(s) ? v : 0; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { off += __shfl_xor(off, m); t += __shfl_xor(t, m); }
    if (SEL_SELF(s) == 0 && tid == 0) ntot[0] = t;
    const int n = count[s], per = work_rec_per(t), zt = R.compact ? SEL_SELF(s) : s;
    if (O.band <= 0 || n > O.pad) {                              // (n > pad cannot happen: n <= cap <= pad; it guards the LDS array)
        for (int j = tid; j < n; j += 256) { work[off + j] = s * cap + j; if (R.rec) kp_write_rec(R, yx, O.H, O.W, off + j, per, s * cap + j, s, zt); }
        return;
    }
    int P = 1;
    while (P < n) P <<= 1;
    const double *p = yx + 2 * (size_t)s * cap;
    for (int j = tid; j < P; j += 256)
        s_word[j] = j < n ? ((unsigned long long)work_key(p[2 * j], p[2 * j + 1], O.H, O.W, O.band) << 32) | (unsigned)j : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
            for (int u = tid; u < (P >> 1); u += 256) {
                const int i = ((u & ~(d - 1)) << 1) | (u & (d - 1));             // the lower index of the u-th pair at distance d
                const unsigned long long a = s_word[i], c = s_word[i + d];
                if ((a > c) == ((i & k) == 0)) { s_word[i] = c; s_word[i + d] = a; }
            }
            __syncthreads();
        }
    for (int j = tid; j < n; j += 256) {
        const int q = s * cap + (int)(unsigned)s_word[j];
        work[off + j] = q;
        if (R.rec) kp_write_rec(R, yx, O.H, O.W, off + j, per, q, s, zt);   // a match follows: everything its prologue looks up, where its wave will read it
    }
}

// Stable in-place compaction of every stream's list, one 256-thread workgroup per stream.
// mode 0 (after a temporal match): keep st != 0; a tracked keypoint (st == 1) takes its new position from oyx.
// mode 1 (removal by flags): keep flags[slot] == 0.
// Chunks of 256 slots are read (all fields into registers), ranked with a wave ballot + the popcount of the lower lanes,
// and written back after a barrier: destinations never lie to the right of their sources, so in place is safe.
// (The load and the store block stay spelled out: a record struct with load / store members changes the kernel's register assignment -- HISTORY.md, round 20.)
// Selected form: an unselected stream's list is not visited -- its st is stale from its last temporal match, and mode 0 would compact it by
// statuses that say nothing about this frame.
__global__ __launch_bounds__(256) void SEL_NAME(k_kpset_compact)(KpsetView K, int mode, const uint8_t *flags SEL_ARG)
{
    __shared__ int s_w[4], s_base;
    const int s = SEL_STREAM(blockIdx.x), tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t b = (size_t)s * K.cap;
    const int n = K.count[s];
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int j = c0 + tid;
        bool keep = false;
        double y = 0, x = 0, sy = 0, sx = 0, X0 = 0, X1 = 0, X2 = 0, ky = 0, kx = 0, fy0 = 0, fx0 = 0; int64_t id = 0; uint8_t f3 = 0, fs = 0, fk = 0; int fkid = 0;
        if (j < n) {
            const size_t q = b + j;
            if (mode == 0) { const uint8_t t = K.st[q]; keep = t != 0; if (t == 1) { y = K.oyx[2 * q]; x = K.oyx[2 * q + 1]; } else { y = K.yx[2 * q]; x = K.yx[2 * q + 1]; } }
            else { keep = flags[q] == 0; y = K.yx[2 * q]; x = K.yx[2 * q + 1]; }
            if (keep) { sy = K.syx[2 * q]; sx = K.syx[2 * q + 1]; X0 = K.xyz[3 * q]; X1 = K.xyz[3 * q + 1]; X2 = K.xyz[3 * q + 2]; id = K.id[q]; f3 = K.is3d[q]; fs = K.stereo[q];
                        ky = K.kyx[2 * q]; kx = K.kyx[2 * q + 1]; fk = K.haskf[q]; fy0 = K.fyx[2 * q]; fx0 = K.fyx[2 * q + 1]; fkid = K.fkf[q]; }
        }
        // (its own loop, not ordered_slot: the writes follow the one barrier that ends the chunk's reads, and this kernel runs after every match)
        const unsigned long long m = __ballot(keep);
        const int rank = __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[wv] = __builtin_popcountll(m);
        __syncthreads();                                        // all reads of the chunk done; wave totals visible
        int wbase = 0;
        for (int i = 0; i < wv; i++) wbase += s_w[i];
        const int total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (keep) {
            const size_t q = b + s_base + wbase + rank;
            K.yx[2 * q] = y; K.yx[2 * q + 1] = x; K.syx[2 * q] = sy; K.syx[2 * q + 1] = sx;
            K.xyz[3 * q] = X0; K.xyz[3 * q + 1] = X1; K.xyz[3 * q + 2] = X2; K.id[q] = id; K.is3d[q] = f3; K.stereo[q] = fs;
            K.kyx[2 * q] = ky; K.kyx[2 * q + 1] = kx; K.haskf[q] = fk; K.fyx[2 * q] = fy0; K.fyx[2 * q + 1] = fx0; K.fkf[q] = fkid;
        }
        __syncthreads();
        if (tid == 0) s_base += total;
        __syncthreads();
    }
    if (tid == 0) K.count[s] = s_base;
}

// create_keyframe! (map_manager.jl:60-96) as far as the lists are concerned: the current frame becomes the previous key-frame
// of every keypoint it holds (frames_map[kfid] is a copy of the frame, new keypoints included: call it after slam_kpset_detect)
// (C linkage: the plain kernel has carried an unmangled name since it was written inside kpset.hip's extern "C" block)
extern "C" __global__ __launch_bounds__(256) void SEL_NAME(k_kpset_keyframe)(KpsetView K SEL_ARG)
{
    const int s = SEL_STREAM(blockIdx.y), j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K.count[s]) return;
    const size_t q = (size_t)s * K.cap + j;
    const double y = K.yx[2 * q], x = K.yx[2 * q + 1];
    if (!K.haskf[q]) { K.fyx[2 * q] = y; K.fyx[2 * q + 1] = x; K.fkf[q] = K.kfcount[s]; }     // detected by this key-frame: its first observer
    K.kyx[2 * q] = y; K.kyx[2 * q + 1] = x; K.haskf[q] = 1;
}
