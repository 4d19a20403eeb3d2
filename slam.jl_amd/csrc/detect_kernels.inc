// detect_kernels.inc -- the three detection kernels that exist in two forms, each written once: detect.hip includes this file twice.
//   plain     SEL_NAME(k) = k, SEL_STREAM(b) = b: workgroup (or grid row) b works on stream b -- slam_detect*, and the keypoint-set seams without a selection
//   selected  SEL_NAME(k) = k_sel, SEL_STREAM(b) = stream_sel[b], one more argument (SEL_ARG) `const int *stream_sel`: the ascending table of the streams
//             slam_kpset_select names (kpset_select.hpp); the launch is sized by their number, so no workgroup exists for an unselected stream: none of
//             its cells is computed, its cell lists are neither written nor read, its list, its id counter and its info entries are not touched
// An include, not a template over a shared __device__ body: the plain kernels then compile from the token sequence they had before there was a
// selection, and their code objects stay instruction for instruction what they were (profiles/r21a_select_kernel_table.txt; an inlined body did
// not: other registers, another order of independent instructions).

// One workgroup per grid cell (grid.x) and stream (grid.y): see the head of detect.hip.  detect_cells takes the argument struct FIRST in both forms: the
// kernel reads its taps and its disk table from offset 0 of the kernel-argument segment.
__global__ __launch_bounds__(DET_THREADS) void SEL_NAME(detect_cells)(DetectArgs A SEL_ARG)
{
    extern __shared__ double lds[];
#ifdef DET_TRACE
    long long dt_clk[12]; const long long dt_t0 = clock64();
    for (int q = 0; q < 12; q++) dt_clk[q] = 0;
#endif
    // per-stream view of the arguments in locals: writing to the argument struct (or indexing its tap array with a lane
    // index) makes the compiler copy all 472 bytes of it to scratch and read every field back from there
    const double *a_img = A.img, *a_cur = A.cur;
    int a_ncur = A.n_cur, a_k = A.k;
    int64_t *a_cell_out = A.cell_out; int *a_cell_cnt = A.cell_cnt;
    if (A.cur_cnt) {
        const int z = SEL_STREAM(blockIdx.y), nc = A.grid_rows * A.grid_cols, ncur = A.cur_cnt[z];
        a_img += (size_t)z * A.zs; a_cur += 2 * (size_t)z * A.cur_stride; a_ncur = ncur;
        a_k = ncur >= A.max_points ? 0 : (A.max_points - ncur + nc - 1) / nc;                 // extractor.jl:64-66, 74-76
        a_cell_out += (size_t)z * nc * A.kmax * 2; a_cell_cnt += (size_t)z * nc;
    } else if (A.cur_off) {
        const int z = blockIdx.y, o = A.cur_off[z], nc = A.grid_rows * A.grid_cols;
        a_img += (size_t)z * A.zs; a_cur += 2 * (size_t)o; a_ncur = A.cur_off[z + 1] - o; a_k = A.k_s[z];
        a_cell_out += (size_t)z * nc * A.kmax * 2; a_cell_cnt += (size_t)z * nc;
    }
    const int cs = A.cs, H = A.H, W = A.W;
    const int cell = blockIdx.x;
    const int cyi = cell / A.grid_cols, cxi = cell % A.grid_cols;
    const int y0 = cyi * cs, x0 = cxi * cs;
    const int h = min(H, (cyi + 1) * cs) - y0, w = min(W, (cxi + 1) * cs) - x0;
    const int tid = threadIdx.x;
    const int n = cs * cs;
    double *bA = lds, *bB = lds + n, *bC = lds + 2 * n, *bD = lds + 3 * n;
    __shared__ int s_ncand, s_cnt;
    __shared__ __attribute__((aligned(16))) int s_cand[2 * DET_MAXCAND];
    __shared__ int s_lim[DET_MAXR + 1];
    __shared__ double s_taps[DET_MAXTAPS];

    if (h <= 0 || w <= 0 || a_k <= 0) { if (tid == 0) a_cell_cnt[cell] = 0; return; }

    // taps -> LDS once.  Indexing A.taps with a lane index makes the compiler copy the argument struct to scratch, and 41 statically
    // indexed copies are 41 serialised scalar loads (6.5 k cycles): read the kernel-argument segment itself with one vector load per
    // lane instead (detect_cells has a single argument: the struct starts at offset 0 of the segment).
    if (a_ncur > 0 && A.ntaps > 0 && tid < A.ntaps) {
        const double *kt = (const double *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(DetectArgs, taps));
        s_taps[tid] = kt[tid];
    }
    // ---- image tile -> bA ---------------------------------------------------
    const DetDiv dvh(h), dnstr((h + DET_SL - 1) / DET_SL);
    for (int i0 = tid; i0 < h * w; i0 += 5 * DET_THREADS) {          // five loads per thread in flight (a 35 x 35 cell: one trip)
        double v[5];
#pragma unroll
        for (int u = 0; u < 5; u++) {
            const int i = i0 + u * DET_THREADS, ic = i < h * w ? i : i0;
            const int icx = dvh.div(ic);
            v[u] = a_img[(size_t)(y0 + ic - icx * h) + (size_t)(x0 + icx) * A.pitch];
        }
#pragma unroll
        for (int u = 0; u < 5; u++) { const int i = i0 + u * DET_THREADS; if (i < h * w) bA[i] = v[u]; }
    }

    DT(0);
    // ---- avoidance mask (get_mask + imfilter(mask, Kernel.gaussian) + .*) ---
    if (a_ncur > 0) {
        const int hw = A.ntaps >> 1;
        const int mh = h + 2 * hw, mw = w + 2 * hw;
        const int r = A.radius;
        if (tid == 0) s_ncand = 0;
        // ImageDraw's disk test ((dy/r)^2 + (dx/r)^2 < 1, f64) as a table: s_lim[|dy|] = largest |dx| inside the
        // disk (-1: none).  Same operations on the same operands as the per-pixel test, evaluated once per cell
        // instead of two f64 divisions per (pixel, keypoint) pair.
        // (the r + 1 quotients d / r are formed once, one per thread, instead of r + 1 divisions in sequence by every table thread)
        if (tid <= r) s_lim[tid] = ((const signed char *)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(DetectArgs, lim) + tid];      // (a lane-indexed read of the by-value struct would copy all of it to scratch)
        __syncthreads();
        // candidate keypoints: disk (+halo) touches the clamped tile region
        const int ylo = clampi(y0 - hw, 0, H - 1) + 1, yhi = clampi(y0 + h - 1 + hw, 0, H - 1) + 1; // 1-based
        const int xlo = clampi(x0 - hw, 0, W - 1) + 1, xhi = clampi(x0 + w - 1 + hw, 0, W - 1) + 1;
        // (four keypoints per thread requested at once: one L2 round trip per 1024 keypoints instead of one per 256)
        for (int k0 = tid; k0 < a_ncur; k0 += 4 * DET_THREADS) {
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const int k = k0 + u * DET_THREADS; v[u] = ((const double2 *)a_cur)[k < a_ncur ? k : k0]; }
            // compaction by wave ballot: a hit's slot is the wave's base (one LDS atomic per wave and pass) + the number of hits in
            // the lower lanes (popcount of the ballot below the lane) -- no per-hit atomics
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const bool live = k0 + u * DET_THREADS < a_ncur;
                const long py = (long)rint(v[u].x), px = (long)rint(v[u].y);
                const bool hit = live && py + r >= ylo && py - r <= yhi && px + r >= xlo && px - r <= xhi;
                const unsigned long long bal = __ballot(hit);
                if (bal) {                                                        // wave-uniform
                    int base = 0;
                    if ((tid & 63) == 0) base = atomicAdd(&s_ncand, __popcll(bal));
                    base = __shfl(base, 0);
                    const int slot = base + __popcll(bal & ((1ull << (tid & 63)) - 1ull));
                    if (hit && slot < DET_MAXCAND) { s_cand[2 * slot] = (int)py; s_cand[2 * slot + 1] = (int)px; }
                }
            }
        }
        __syncthreads();
        DT(1);
        const int ncand = s_ncand;
        const bool overflow = ncand > DET_MAXCAND;
        // raw mask over the halo'd tile (replicate = clamped coordinates) -> bB (as 0/1 doubles)
        // the halo'd raw mask is stored as bytes
        unsigned char *m0 = (unsigned char *)(lds + 4 * n) - ((mh * mw + 7) & ~7);   // byte mask at the tail of bD (sizes checked on host)
        if (!overflow) {
            // Rasterised: the mask starts as ones, every (candidate, disk row) pair clears its x-interval (ImageDraw draws
            // in-image pixels only), then halo pixels outside the image replicate the border pixel they clamp to.  Same
            // mask as testing every pixel against every candidate, ~5x fewer LDS operations.
            for (int i = tid; i < mh * mw; i += DET_THREADS) m0[i] = 1;
            __syncthreads();
            const int nrow = 2 * r + 1, ty0 = y0 - hw, tx0 = x0 - hw;
            const DetDiv dnrow(nrow), dmh(mh);
            for (int q = tid; q < ncand * nrow; q += DET_THREADS) {
                const int c = dnrow.div(q), dyi = q - c * nrow - r;
                const int yy = s_cand[2 * c] + dyi, px = s_cand[2 * c + 1];      // 1-based image coordinates
                const int lim = s_lim[abs(dyi)];
                const int ty = (yy - 1) - ty0;
                if (yy < 1 || yy > H || lim < 0 || ty < 0 || ty >= mh) continue;
                int txa = (max(px - lim, 1) - 1) - tx0, txb = (min(px + lim, W) - 1) - tx0;
                txa = txa < 0 ? 0 : txa; txb = txb > mw - 1 ? mw - 1 : txb;
                for (int tx = txa; tx <= txb; tx++) m0[ty + tx * mh] = 0;
            }
            __syncthreads();
            if (ty0 < 0 || ty0 + mh - 1 > H - 1 || tx0 < 0 || tx0 + mw - 1 > W - 1) {        // border cell: replicate
                for (int i = tid; i < mh * mw; i += DET_THREADS) {
                    const int imx = dmh.div(i);
                    const int uy = ty0 + i - imx * mh, ux = tx0 + imx;
                    if (uy < 0 || uy > H - 1 || ux < 0 || ux > W - 1)
                        m0[i] = m0[(clampi(uy, 0, H - 1) - ty0) + (clampi(ux, 0, W - 1) - tx0) * mh];
                }
            }
        } else {
            for (int i = tid; i < mh * mw; i += DET_THREADS) {
                const int yy = clampi(y0 + i % mh - hw, 0, H - 1) + 1, xx = clampi(x0 + i / mh - hw, 0, W - 1) + 1; // 1-based
                unsigned char m = 1;
                for (int c = 0; c < a_ncur; c++) {
                    long py = (long)rint(a_cur[2 * c]), px = (long)rint(a_cur[2 * c + 1]);
                    const long dy = labs(yy - py), dx = labs(xx - px);
                    if (dy <= r && dx <= s_lim[dy]) { m = 0; break; }
                }
                m0[i] = m;
            }
        }
        DT(2);
        __syncthreads();
        if (A.ntaps > 0) {
            double *T = bB;                                   // h*mw doubles: bB, bC and the part of bD below the byte mask (checked on host)
            if (A.ntaps == 13) blur_mask<13>(bA, T, m0, s_taps, h, w, mh, mw, tid, dnstr, dvh);      // sigma_mask = 3 (the default): unrolled
            else blur_mask<0>(bA, T, m0, s_taps, h, w, mh, mw, tid, dnstr, dvh, A.ntaps);
        } else {
            for (int i = tid; i < h * w; i += DET_THREADS) {
                const int x = dvh.div(i), y = i - x * h;
                bA[i] = bA[i] * (double)m0[(y + hw) + (x + hw) * mh];
            }
        }
    }
    __syncthreads();

    DT(3);
    // ---- Images.shi_tomasi on the cell view (replicate border at cell edges) -
    // imgradients(cell, KernelFactors.sobel): g1 = (d/dy along dim 1, then (1,2,1)/4 along dim 2),
    // g2 = ((1,2,1)/4 along dim 1, then d/dx along dim 2); products -> bB, bC, bD
    // thread = (column x, strip of DET_SL rows): 21 LDS reads per DET_SL pixels and plane instead of 9 per pixel
    const int nstr = (h + DET_SL - 1) / DET_SL;
    for (int it = tid; it < w * nstr; it += DET_THREADS) {
        const int x = dnstr.div(it), ys = (it - x * nstr) * DET_SL;
        DetStrip S;
        det_strip_load(S, bA, h, w, ys, x);
#pragma unroll
        for (int q = 0; q < DET_SL; q++) {
            if (ys + q < h) {
                const double g1 = det_strip_sep3(S, q, -1.0 / 2, 0.0 / 2, 1.0 / 2, 1.0 / 4, 2.0 / 4, 1.0 / 4);
                const double g2 = det_strip_sep3(S, q, 1.0 / 4, 2.0 / 4, 1.0 / 4, -1.0 / 2, 0.0 / 2, 1.0 / 2);
                const int i = (ys + q) + x * h;
                bB[i] = g1 * g1; bC[i] = g1 * g2; bD[i] = g2 * g2;
            }
        }
    }
    __syncthreads();
    DT(4);
    // 3x3 box mean of the products (1/3 x 1/3, two-pass arithmetic) and the min-eigenvalue response -> bA
    double *resp = bA;
    for (int it = tid; it < w * nstr; it += DET_THREADS) {
        const int x = dnstr.div(it), ys = (it - x * nstr) * DET_SL;
        double xx[DET_SL], xy[DET_SL], yy[DET_SL];
        DetStrip S;
        det_strip_load(S, bB, h, w, ys, x);
#pragma unroll
        for (int q = 0; q < DET_SL; q++) xx[q] = det_strip_sep3(S, q, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3);
        det_strip_load(S, bC, h, w, ys, x);
#pragma unroll
        for (int q = 0; q < DET_SL; q++) xy[q] = det_strip_sep3(S, q, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3);
        det_strip_load(S, bD, h, w, ys, x);
#pragma unroll
        for (int q = 0; q < DET_SL; q++) yy[q] = det_strip_sep3(S, q, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3, 1.0 / 3);
#pragma unroll
        for (int q = 0; q < DET_SL; q++) {
            if (ys + q < h) {
                const double dd = xx[q] - yy[q];
                resp[(ys + q) + x * h] = ((xx[q] + yy[q]) - sqrt(dd * dd + 4 * (xy[q] * xy[q]))) / 2;
            }
        }
    }
    __syncthreads();
    DT(5);

    // ---- findlocalmaxima: strict, 8-neighbourhood, edges included (neighbours outside the cell are not compared) ------------
    // The strict maxima (typically 20-40 of a 35 x 35 cell) are compacted as they are found -- wave ballot + popcount of the lower lanes,
    // one LDS atomic per wave and strip pass -- into a list of (pixel index, response); the top-k selection then runs on ONE wave
    // over that list: k rounds of a wave arg-max on the key (response descending, pixel index ascending = Julia's stable sortperm over
    // the column-major maxima, extractor.jl:27-40), no workgroup barrier and no merge thread per round.
    int *mx_idx = (int *)bC;                                  // compacted maxima: pixel index (column-major) ...
    double *mx_val = bD;                                      // ... and response
    if (tid == 0) { s_cnt = 0; s_ncand = 0; }
    __syncthreads();
    for (int it0 = 0; it0 < w * nstr; it0 += DET_THREADS) {   // (whole waves enter every pass: the ballots need them)
        const int it = it0 + tid;
        const bool act = it < w * nstr;
        const int x = act ? dnstr.div(it) : 0, ys = act ? (it - x * nstr) * DET_SL : 0;
        DetStrip S;
        det_strip_load(S, resp, h, w, ys, x);
        const bool cl = x > 0, cr = x < w - 1;
#pragma unroll
        for (int q = 0; q < DET_SL; q++) {
            const int y = ys + q;
            const double c = S.v[1][q + 1];
            bool ismax = act && y < h;
            const bool ru = y > 0, rd = y < h - 1;
            if (cl) { if (ru && !(S.v[0][q] < c)) ismax = false; if (!(S.v[0][q + 1] < c)) ismax = false; if (rd && !(S.v[0][q + 2] < c)) ismax = false; }
            if (ru && !(S.v[1][q] < c)) ismax = false;
            if (rd && !(S.v[1][q + 2] < c)) ismax = false;
            if (cr) { if (ru && !(S.v[2][q] < c)) ismax = false; if (!(S.v[2][q + 1] < c)) ismax = false; if (rd && !(S.v[2][q + 2] < c)) ismax = false; }
            const unsigned long long bal = __ballot(ismax);
            if (bal) {
                int base = 0;
                if ((tid & 63) == 0) base = atomicAdd(&s_ncand, __popcll(bal));
                base = __shfl(base, 0);
                const int slot = base + __popcll(bal & ((1ull << (tid & 63)) - 1ull));
                if (ismax) { mx_idx[slot] = y + x * h; mx_val[slot] = c; }      // (at most h w / 4 strict maxima: the planes have room)
            }
        }
    }
    __syncthreads();

    DT(6);
    // ---- top-k by response (stable: ties keep column-major order), wave 0 only ------------
    int *sel = (int *)bB;                                     // selected pixel indices
    if (tid < 64) {
        const int nmx = s_ncand;
        int cnt = 0;
        for (int round = 0; round < a_k; round++) {
            double bv = -INFINITY; int bi = 0x7fffffff, bs = -1;
            for (int j = tid; j < nmx; j += 64) {
                const int i = mx_idx[j];
                if (i >= 0) {                                                     // (taken entries are marked -1)
                    const double v = mx_val[j];
                    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; bs = j; }
                }
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(bv, off); const int oi = __shfl_xor(bi, off), os = __shfl_xor(bs, off);
                if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; bs = os; }
            }
            if (bi == 0x7fffffff) break;                                          // wave-uniform after the butterfly
            if (tid == 0) {
                mx_idx[bs] = -1;
                if (!(bv < A.min_response)) sel[cnt] = bi;                       // `responses[mx] < min_response && continue`
            }
            if (!(bv < A.min_response)) cnt++;
        }
        if (tid == 0) s_cnt = cnt;
    }
    __syncthreads();

    DT(7);
    // ---- emit in column-major order (Keypoints(::Matrix{Bool}) = findall) ----
    if (tid == 0) {
        int cnt = s_cnt;
        for (int i = 1; i < cnt; i++) { int v = sel[i], j = i - 1; while (j >= 0 && sel[j] > v) { sel[j + 1] = sel[j]; j--; } sel[j + 1] = v; }
        int64_t *o = a_cell_out + (size_t)cell * a_k * 2;
        for (int i = 0; i < cnt; i++) {
            int y = sel[i] % h, x = sel[i] / h;
            o[2 * i] = y + 1 + y0; o[2 * i + 1] = x + 1 + x0;
        }
        a_cell_cnt[cell] = cnt;
    }
#ifdef DET_TRACE
    DT(8);
    if (tid == 0 && cell == 200 && blockIdx.y == 3) printf("detect cell: ncur %d k %d | tile %lld scan %lld raster %lld blur %lld grad %lld resp %lld lmax %lld topk %lld emit %lld cycles\n", a_ncur, a_k, dt_clk[0], dt_clk[1] - dt_clk[0], dt_clk[2] - dt_clk[1], dt_clk[3] - dt_clk[2], dt_clk[4] - dt_clk[3], dt_clk[5] - dt_clk[4], dt_clk[6] - dt_clk[5], dt_clk[7] - dt_clk[6], dt_clk[8] - dt_clk[7]);
#endif
}

// detect() into a device-resident keypoint set: the avoidance list of stream z is its current list in the set, the new
// keypoints (cells row-major, column-major inside a cell: extractor.jl:81-91) are appended behind it as (row, col) Float64
// pixels with is_3d = 0 and fresh ids -- extract_keypoints! + add_keypoints_to_frame! (map_manager.jl:98-113) on arrays.
// One 1024-thread workgroup per stream, cell_scan over chunks of 1024 cells (as detect_compact).
__global__ __launch_bounds__(1024) void SEL_NAME(detect_append)(const int64_t *cell_out, const int *cell_cnt, int n_cells, int kmax, int max_points, KpsetView K,
                                                                int64_t *next_id SEL_ARG)
{
    const int z = SEL_STREAM(blockIdx.x), cap = K.cap;
    cell_out += (size_t)z * n_cells * kmax * 2; cell_cnt += (size_t)z * n_cells;
    const size_t b = (size_t)z * cap;
    const int n0 = K.count[z];
    const int64_t id0 = next_id[z];
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    if (n0 >= max_points) return;                                 // extractor.jl:64: nothing detected (cell counts are zero as well)
    const int kz = (max_points - n0 + n_cells - 1) / n_cells;      // this stream's per-cell quota = the stride of its cell lists (detect_cells)
    for (int c0 = 0; c0 < n_cells; c0 += 1024) {
        const int c = c0 + tid, cnt = c < n_cells ? cell_cnt[c] : 0;
        const int start = cell_scan(cnt, s_w, &s_base);
        for (int i = 0; i < cnt; i++) {
            const int j = n0 + start + i;
            if (j < cap) {
                const size_t q = b + j;
                K.yx[2 * q] = (double)cell_out[((size_t)c * kz + i) * 2]; K.yx[2 * q + 1] = (double)cell_out[((size_t)c * kz + i) * 2 + 1];
                K.syx[2 * q] = 0.0; K.syx[2 * q + 1] = 0.0; K.xyz[3 * q] = 0.0; K.xyz[3 * q + 1] = 0.0; K.xyz[3 * q + 2] = 0.0;
                K.id[q] = id0 + start + i; K.is3d[q] = 0; K.stereo[q] = 0; K.haskf[q] = 0;
            }
        }
    }
    if (tid == 0) { const int n1 = n0 + s_base; K.count[z] = n1 < cap ? n1 : cap; next_id[z] = id0 + s_base; }
}

// describe()'s border drop on the cell lists (map_manager.jl:105-106: detect, then describe returns the keypoints it kept): every cell's
// candidates whose +-lim box leaves the image go, order kept, before detect_append merges the lists -- the dropped ones are not replaced, as in
// the reference.  One thread per cell (a list holds the cell's quota, a handful of entries); kz as in detect_append.  The thread of cell 0 notes
// the stream's list length and id counter before the append (cnt0, info[2 z]).
// (selected form: the unselected streams' cnt0 and info come from k_unselected_info)
__global__ __launch_bounds__(256) void SEL_NAME(detect_box_filter)(int64_t *cell_out, int *cell_cnt, int n_cells, int kmax, int max_points, const int *count,
                                                                   const int64_t *next_id, int H, int W, int lim, int *cnt0, int64_t *info SEL_ARG)
{
    const int z = SEL_STREAM(blockIdx.y), c = blockIdx.x * 256 + threadIdx.x;
    const int n0 = count[z];
    if (c == 0) { cnt0[z] = n0; info[2 * z] = next_id[z]; }
    if (c >= n_cells || n0 >= max_points) return;
    const int kz = (max_points - n0 + n_cells - 1) / n_cells;
    int64_t *o = cell_out + ((size_t)z * n_cells * kmax + (size_t)c * kz) * 2;
    int *pc = cell_cnt + (size_t)z * n_cells + c;
    const int cnt = *pc;
    int m = 0;
    for (int i = 0; i < cnt; i++) {
        const int64_t y = o[2 * i], x = o[2 * i + 1];
        if (y - lim < 1 || y + lim > H || x - lim < 1 || x + lim > W) continue;
        o[2 * m] = y; o[2 * m + 1] = x; m++;
    }
    *pc = m;
}
