// detect.hip -- grid-cell Shi-Tomasi keypoint extraction on gfx950.
//
// Replaces detect / get_mask / _shi_tomasi of the reference
// (src/extractor.jl:24-42, 63-95, 116-122).  One workgroup per grid cell: the
// cell's pixels, the avoidance-mask halo and every intermediate plane live in
// LDS (four cell-sized planes; the avoidance mask is rasterised per disk row; the separable Sobel and box stages are evaluated
// per pixel from the 3x3 neighbourhood with exactly the two-stage arithmetic,
// so no intermediate plane is stored and four workgroups share a CU); HBM traffic is one read of the image plus the keypoint lists, i.e. the
// algorithmic minimum (8*H*W + 16*(K + n_out) bytes).  Keypoint order and
// indices are bit-exact with the CPU oracle: every sum runs in the reference's
// order and the build uses -ffp-contract=off.
#include "kpset.hpp"
#include "geom_device.hpp"
#include <cmath>
#include <cstddef>

#define DET_THREADS 256
#define DET_MAXCAND 512
#define DET_MAXTAPS 41
#define DET_MAXR 64                // disk radius of the avoidance mask (extractor radius, SLAM.jl:158: 17)

struct DetectArgs {
    const double *img; int H, W, pitch;
    const double *cur; int n_cur;      // device (y,x) pairs
    int radius, grid_rows, grid_cols, cs, k;
    double min_response;
    int ntaps;                         // 0: no blur of the mask
    double taps[DET_MAXTAPS];
    int64_t *cell_out;                 // n_cells * k * 2
    int *cell_cnt;                     // n_cells
    // batched launch (grid.y = stream): per-stream image offset, slice of `cur` and k; nullptr for a single image
    const int *cur_off, *k_s; size_t zs; int kmax;
    // keypoint-set launch (slam_kpset_detect): stream z's current keypoints are cur[2 * z * cur_stride ..], cur_cnt[z] of them
    // (device-side count), k follows from it
    const int *cur_cnt; int cur_stride, max_points;
    // ImageDraw's disk test ((dy/r)^2 + (dx/r)^2 < 1, f64) as a table: lim[|dy|] = largest |dx| inside the disk (-1: none), formed once
    // on the host with the per-pixel test's operations (det_disk_table; every cell used to rebuild it: ~3 k of a cell's 39 k cycles)
    signed char lim[DET_MAXR + 1];
};
static void det_disk_table(DetectArgs &A)
{
    const int r = A.radius;
    for (int dy = 0; dy <= DET_MAXR; dy++) A.lim[dy] = -1;
    for (int dy = 0; dy <= r && dy <= DET_MAXR; dy++) {
        const volatile double a = (double)dy / (double)r;
        int lim = -1;
        for (int dx = 0; dx <= r; dx++) {
            const volatile double b = (double)dx / (double)r;
            const volatile double aa = a * a, bb = b * b;       // (separately rounded products: no contraction)
            if (aa + bb < 1) lim = dx; else break;
        }
        A.lim[dy] = (signed char)lim;
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Separable 3x3 correlation evaluated at one pixel with the arithmetic of the two-pass form (ImageFiltering:
// first factor along dim 1 into an intermediate, second factor along dim 2; acc = 0; acc += v[j]*k[j], j ascending;
// replicate border at the cell edge): the three intermediate values of columns x-1, x, x+1 are recomputed in
// registers instead of being stored as a plane.
__device__ __forceinline__ double sep3(const double *src, int h, int w, int y, int x,
                                       double ky0, double ky1, double ky2, double kx0, double kx1, double kx2)
{
    const int ym = clampi(y - 1, 0, h - 1), yp = clampi(y + 1, 0, h - 1);
    double t[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int xx = clampi(x + j - 1, 0, w - 1);
        double acc = 0.0;
        acc += src[ym + xx * h] * ky0; acc += src[y + xx * h] * ky1; acc += src[yp + xx * h] * ky2;
        t[j] = acc;
    }
    double acc = 0.0;
    acc += t[0] * kx0; acc += t[1] * kx1; acc += t[2] * kx2;
    return acc;
}

// imfilter(mask, Kernel.gaussian(sigma)) as two separable passes over the halo'd byte mask, then image .* mask.
// acc = 0; acc += v[j] * k[j], j ascending (ImageFiltering order) in both passes.  NT > 0: tap count known at compile time.
// Strips: a thread produces DET_SL consecutive outputs along the filtered dimension from one run of DET_SL + NT - 1 inputs held in
// registers (NT known at compile time) -- 3.4 instead of 13 LDS reads per output; every output is still acc = 0; acc += v[j] * k[j]
// with j ascending.
#define DET_SL 5
// i / d and i % d for a divisor that is only known at run time (cell height, strips per column, disk rows): the compiler expands such a division into
// ~25 instructions at every site.  One multiplication by m = ceil(2^32 / d), formed once per workgroup, is exact for i < 2^16 <= 2^32 / d (every index of a
// cell tile is far below that).
struct DetDiv {
    unsigned m, d;
    __device__ __forceinline__ explicit DetDiv(int dd) : m(0xffffffffu / (unsigned)(dd > 0 ? dd : 1) + 1u), d((unsigned)(dd > 0 ? dd : 1)) {}
    __device__ __forceinline__ int div(int i) const { return d == 1 ? i : (int)__umulhi((unsigned)i, m); }
    __device__ __forceinline__ int mod(int i) const { return i - div(i) * (int)d; }
};
template <int NT>
__device__ __forceinline__ void blur_mask(double *bA, double *T, const unsigned char *m0, const double *taps, int h, int w, int mh, int mw, int tid, const DetDiv &dns, const DetDiv &dh, int ntaps = NT)
{
    const int nt = NT > 0 ? NT : ntaps;
    if (NT > 0) {
        constexpr int NK = NT > 0 ? NT : 1;
        double k[NK];
#pragma unroll
        for (int j = 0; j < NK; j++) k[j] = taps[j];
        // dim-1 pass: T(y, tx) = sum_j m0(y+j, tx) * k[j]; thread = (column tx, strip of DET_SL rows)
        const int ns = (h + DET_SL - 1) / DET_SL;
        for (int it = tid; it < mw * ns; it += DET_THREADS) {
            const int tx = dns.div(it), ys = (it - tx * ns) * DET_SL;
            double v[DET_SL + NK - 1];
#pragma unroll
            for (int i = 0; i < DET_SL + NK - 1; i++) { const int yy = ys + i < mh ? ys + i : mh - 1; v[i] = (double)m0[yy + tx * mh]; }
#pragma unroll
            for (int q = 0; q < DET_SL; q++) {
                if (ys + q < h) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < NK; j++) acc += v[q + j] * k[j];
                    T[(ys + q) + tx * h] = acc;
                }
            }
        }
        __syncthreads();
        // dim-2 pass and image .* mask; thread = (row y, strip of DET_SL columns)
        const int nsx = (w + DET_SL - 1) / DET_SL;
        for (int it = tid; it < h * nsx; it += DET_THREADS) {
            const int sx = dh.div(it), y = it - sx * h, xs = sx * DET_SL;
            double v[DET_SL + NK - 1];
#pragma unroll
            for (int i = 0; i < DET_SL + NK - 1; i++) { const int xx = xs + i < mw ? xs + i : mw - 1; v[i] = T[y + xx * h]; }
#pragma unroll
            for (int q = 0; q < DET_SL; q++) {
                if (xs + q < w) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < NK; j++) acc += v[q + j] * k[j];
                    bA[y + (xs + q) * h] = bA[y + (xs + q) * h] * acc;
                }
            }
        }
        return;
    }
    // dim-1 pass: T(y, tx) = sum_j m0(y+j, tx) * k[j]
    for (int i = tid; i < h * mw; i += DET_THREADS) {
        const int tx = dh.div(i), y = i - tx * h;
        double acc = 0.0;
        for (int j = 0; j < nt; j++) acc += (double)m0[(y + j) + tx * mh] * taps[j];
        T[i] = acc;
    }
    __syncthreads();
    // dim-2 pass and image .* mask
    for (int i = tid; i < h * w; i += DET_THREADS) {
        const int x = dh.div(i), y = i - x * h;
        double acc = 0.0;
        for (int j = 0; j < nt; j++) acc += T[y + (x + j) * h] * taps[j];
        bA[i] = bA[i] * acc;
    }
}

// A (DET_SL + 2) x 3 neighbourhood of a cell plane in registers: rows ys - 1 .. ys + DET_SL, columns x - 1 .. x + 1, replicate
// border at the cell edge (clamped indices), for the DET_SL outputs (ys .. ys + DET_SL - 1, x).
struct DetStrip { double v[3][DET_SL + 2]; };
__device__ __forceinline__ void det_strip_load(DetStrip &S, const double *src, int h, int w, int ys, int x)
{
    const int xm = clampi(x - 1, 0, w - 1), xp = clampi(x + 1, 0, w - 1);
#pragma unroll
    for (int i = 0; i < DET_SL + 2; i++) {
        const int yy = clampi(ys - 1 + i, 0, h - 1);
        S.v[0][i] = src[yy + xm * h]; S.v[1][i] = src[yy + x * h]; S.v[2][i] = src[yy + xp * h];
    }
}
// sep3 (above) for output q of the strip: the same operations on the same operands
__device__ __forceinline__ double det_strip_sep3(const DetStrip &S, int q, double ky0, double ky1, double ky2, double kx0, double kx1, double kx2)
{
    double t[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        double acc = 0.0;
        acc += S.v[j][q] * ky0; acc += S.v[j][q + 1] * ky1; acc += S.v[j][q + 2] * ky2;
        t[j] = acc;
    }
    double acc = 0.0;
    acc += t[0] * kx0; acc += t[1] * kx1; acc += t[2] * kx2;
    return acc;
}

#ifdef DET_TRACE
#define DT(k) do { __syncthreads(); dt_clk[k] = clock64() - dt_t0; } while (0)
#else
#define DT(k)
#endif
// detect_cells, detect_append and detect_box_filter, plain and selected (slam_kpset_select): detect_kernels.inc, included once per form
#define SEL_NAME(k) k
#define SEL_ARG
#define SEL_STREAM(b) b
#include "detect_kernels.inc"
#undef SEL_NAME
#undef SEL_ARG
#undef SEL_STREAM
#define SEL_NAME(k) k##_sel
#define SEL_ARG , const int *stream_sel
#define SEL_STREAM(b) stream_sel[b]
#include "detect_kernels.inc"
#undef SEL_NAME
#undef SEL_ARG
#undef SEL_STREAM

// Ordered compaction of the per-cell lists (cells row-major: extractor.jl:81), cell_scan over chunks of 1024 cells.
__global__ __launch_bounds__(1024) void detect_compact(const int64_t *cell_out, const int *cell_cnt, int n_cells, int k,
                                                        int64_t *out /* [0] = n_out, then pairs */, int cap,
                                                        const int *k_s /* batched: grid.x = stream, per-stream k, lists strided by kmax = k */)
{
    if (k_s) {
        const int z = blockIdx.x;
        cell_out += (size_t)z * n_cells * k * 2; cell_cnt += (size_t)z * n_cells; out += (size_t)z * (1 + 2 * (size_t)cap);
        k = k_s[z];
    }
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n_cells; c0 += 1024) {
        const int c = c0 + tid, cnt = c < n_cells ? cell_cnt[c] : 0;
        const int start = cell_scan(cnt, s_w, &s_base);
        for (int i = 0; i < cnt; i++)
            if (start + i < cap) {
                out[1 + 2 * (start + i)] = cell_out[((size_t)c * k + i) * 2];
                out[2 + 2 * (start + i)] = cell_out[((size_t)c * k + i) * 2 + 1];
            }
    }
    if (tid == 0) out[0] = s_base;
}

// What the three detection entry points share: every field of A but the avoidance list and the cell lists (single image: A.k / A.n_cur
// are the caller's), the Gaussian taps, and the checks of the LDS carve-up for `kmax`, the largest per-cell quota of the launch.
static int det_plan(slam_ctx *ctx, DetectArgs &A, const double *img, int H, int W, int pitch, size_t zs, int max_points, int radius,
                    int grid_rows, int grid_cols, int cell_size, int kmax, double sigma_mask, double min_response, size_t *lds_bytes)
{
    A.img = img; A.H = H; A.W = W; A.pitch = pitch; A.zs = zs; A.radius = radius; det_disk_table(A);
    A.grid_rows = grid_rows; A.grid_cols = grid_cols; A.cs = cell_size; A.k = 0; A.kmax = kmax; A.n_cur = 0; A.min_response = min_response;
    A.cur = nullptr; A.cur_off = nullptr; A.k_s = nullptr; A.cur_cnt = nullptr; A.cur_stride = 0; A.max_points = max_points;
    A.ntaps = 0;
    if (sigma_mask != 0) {
        ARG_TRY(ctx, 4 * (int)std::ceil(sigma_mask) + 1 <= DET_MAXTAPS);
        A.ntaps = slam_gaussian_taps(sigma_mask, A.taps);
    }
    const int hw = A.ntaps >> 1;
    const size_t n = (size_t)cell_size * cell_size;
    // LDS carve-up (4 planes of cell_size^2 doubles): byte mask at the tail of the 4th plane, blur intermediate in planes 2..4 below it
    const size_t mbytes = ((size_t)(cell_size + 2 * hw) * (cell_size + 2 * hw) + 7) & ~(size_t)7;
    ARG_TRY(ctx, mbytes <= n * 8 && (size_t)cell_size * (cell_size + 2 * hw) * 8 + mbytes <= 3 * n * 8);
    ARG_TRY(ctx, (size_t)kmax * sizeof(int) <= n * 8);
    *lds_bytes = 4 * n * sizeof(double);
    ARG_TRY(ctx, *lds_bytes <= 150 * 1024);
    // > 64 KB of dynamic LDS needs the opt-in; per device, so set it on every call (cheap host-side call)
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)detect_cells, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    return SLAM_OK;
}

int slam_detect_device(slam_ctx *ctx, const double *img_dev, int H, int W, int pitch, const double *cur_yx, int n_cur,
                       int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                       double sigma_mask, double min_response, int64_t *out_rc, int cap, int *n_out)
{
    ARG_TRY(ctx, H > 0 && W > 0 && grid_rows > 0 && grid_cols > 0 && cell_size >= 8 && radius > 0 && radius <= DET_MAXR && n_out != nullptr);
    ARG_TRY(ctx, n_cur >= 0 && (n_cur == 0 || cur_yx != nullptr));
    *n_out = 0;
    if (n_cur >= max_points) return SLAM_OK;                      // extractor.jl:64
    const int n_cells = grid_rows * grid_cols;
    const int n_detect = max_points - n_cur;
    const int k = (n_detect + n_cells - 1) / n_cells;             // ceil(Int, n_detect / n_cells)
    DetectArgs A;
    size_t lds_bytes;
    int rc = det_plan(ctx, A, img_dev, H, W, pitch, 0, max_points, radius, grid_rows, grid_cols, cell_size, k, n_cur > 0 ? sigma_mask : 0.0, min_response, &lds_bytes);
    if (rc) return rc;
    A.k = k; A.n_cur = n_cur;
    const size_t out_pairs = (size_t)n_cells * k, out_b = 8 + out_pairs * 16;
    Layout D;
    const auto o_cur = D.take<double>((size_t)n_cur * 2); const auto o_cnt = D.take<int>(n_cells); const auto o_cout = D.take<int64_t>(out_pairs * 2), o_out = D.take<int64_t>(out_b / 8);
    char *s;
    rc = slam_scratch(ctx, D.size(), (void **)&s);
    if (rc) return rc;
    double *d_cur = o_cur.at(s); int *d_cnt = o_cnt.at(s);
    int64_t *d_cout = o_cout.at(s), *d_out = o_out.at(s);
    if (n_cur > 0) HIP_TRY(ctx, hipMemcpyAsync(d_cur, cur_yx, o_cur.bytes(), hipMemcpyHostToDevice, ctx->stream));
    A.cur = d_cur; A.cell_out = d_cout; A.cell_cnt = d_cnt;
    { ProfScope span(ctx, "detect");
      hipLaunchKernelGGL(detect_cells, dim3(n_cells), dim3(DET_THREADS), lds_bytes, ctx->stream, A);
      hipLaunchKernelGGL(detect_compact, dim3(1), dim3(1024), 0, ctx->stream, d_cout, d_cnt, n_cells, k, d_out, (int)out_pairs, (const int *)nullptr); }
    HIP_TRY(ctx, hipGetLastError());
    int64_t *h_out;
    rc = slam_pinned(ctx, out_b, (void **)&h_out);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    int64_t cnt = h_out[0];
    if (cnt > cap) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_detect: %lld keypoints but cap = %d", (long long)cnt, cap);
    memcpy(out_rc, h_out + 1, (size_t)cnt * 16);
    *n_out = (int)cnt;
    return SLAM_OK;
}

extern "C" int slam_detect(slam_ctx *ctx, const double *image, int H, int W, const double *cur_yx, int n_cur,
                           int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                           double sigma_mask, double min_response, int64_t *out_rc, int cap, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr);
    ARG_TRY(ctx, image != nullptr && H > 0 && W > 0);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *d_img;
    int rc = slam_scratch2(ctx, (size_t)H * W * 8, &d_img);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_img, image, (size_t)H * W * 8, hipMemcpyHostToDevice, ctx->stream));
    return slam_detect_device(ctx, (const double *)d_img, H, W, H, cur_yx, n_cur, max_points, radius, grid_rows, grid_cols,
                              cell_size, sigma_mask, min_response, out_rc, cap, n_out);
}

extern "C" int slam_detect_pyr(slam_ctx *ctx, const slam_pyr *pyr, const double *cur_yx, int n_cur,
                               int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                               double sigma_mask, double min_response, int64_t *out_rc, int cap, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && pyr != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return slam_detect_device(ctx, pyr->plane(0, 0), pyr->H[0], pyr->W[0], pyr->P[0], cur_yx, n_cur, max_points, radius, grid_rows,
                              grid_cols, cell_size, sigma_mask, min_response, out_rc, cap, n_out);
}

// detect() for the S members of a pyramid batch in one launch (grid.y = stream).  cur_yx holds the current
// keypoints of all streams back to back, cur_off[s] .. cur_off[s+1] those of stream s; the new keypoints come
// back the same way (out_off[S+1]).  Per stream identical to slam_detect_pyr on that stream's pyramid.
extern "C" int slam_detect_batch(slam_ctx *ctx, const slam_pyr *pyr0, int S, const double *cur_yx, const int32_t *cur_off,
                                 int max_points, int radius, int grid_rows, int grid_cols, int cell_size,
                                 double sigma_mask, double min_response, int64_t *out_rc, int cap, int32_t *out_off)
{
    ARG_TRY(ctx, ctx != nullptr && pyr0 != nullptr && S >= 1 && S <= 128 && cur_off != nullptr && out_off != nullptr);
    ARG_TRY(ctx, pyr0->batch_index == 0 && pyr0->batch_size == S);
    ARG_TRY(ctx, grid_rows > 0 && grid_cols > 0 && cell_size >= 8 && radius > 0 && radius <= DET_MAXR && cap >= 0 && (cap == 0 || out_rc != nullptr));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int n_cells = grid_rows * grid_cols, n_tot = cur_off[S];
    ARG_TRY(ctx, cur_off[0] == 0 && n_tot >= 0 && (n_tot == 0 || cur_yx != nullptr));
    int ks[128], kmax = 0;
    for (int s = 0; s < S; s++) {
        const int nc = cur_off[s + 1] - cur_off[s];
        ARG_TRY(ctx, nc >= 0);
        ks[s] = nc >= max_points ? 0 : (max_points - nc + n_cells - 1) / n_cells;     // extractor.jl:64-66
        kmax = ks[s] > kmax ? ks[s] : kmax;
    }
    for (int s = 0; s <= S; s++) out_off[s] = 0;
    if (kmax == 0) return SLAM_OK;
    DetectArgs A;
    size_t lds_bytes;
    int rc = det_plan(ctx, A, pyr0->plane(0, 0), pyr0->H[0], pyr0->W[0], pyr0->P[0], pyr0->zstride, max_points, radius, grid_rows, grid_cols, cell_size, kmax,
                      sigma_mask, min_response, &lds_bytes);
    if (rc) return rc;
    // host -> device in one copy: [cur_off (S+1 ints) at 0] [k_s (S ints) at 1024] [cur (2 * n_tot doubles) at 2048]; the pinned block holds
    // these inputs and the output behind them
    const size_t pairs = (size_t)n_cells * kmax, out_b = (size_t)S * (8 + pairs * 16);
    Layout D;
    const auto o_hdr = D.take<int>(512); const auto o_cur = D.take<double>((size_t)n_tot * 2); const size_t in_b = D.size();
    const auto o_cnt = D.take<int>((size_t)S * n_cells); const auto o_cout = D.take<int64_t>((size_t)S * pairs * 2), o_out = D.take<int64_t>(out_b / 8);
    char *d, *h;
    rc = slam_scratch(ctx, D.size(), (void **)&d);
    if (rc) return rc;
    rc = slam_pinned(ctx, in_b + out_b, (void **)&h);
    if (rc) return rc;
    memcpy(o_hdr.at(h), cur_off, (size_t)(S + 1) * 4); memcpy(o_hdr.at(h) + 256, ks, (size_t)S * 4);
    if (n_tot > 0) memcpy(o_cur.at(h), cur_yx, o_cur.bytes());
    HIP_TRY(ctx, hipMemcpyAsync(d, h, o_cur.off + o_cur.bytes(), hipMemcpyHostToDevice, ctx->stream));
    A.cur_off = o_hdr.at(d); A.k_s = o_hdr.at(d) + 256; A.cur = o_cur.at(d);
    A.cell_cnt = o_cnt.at(d); A.cell_out = o_cout.at(d);
    int64_t *d_out = o_out.at(d);
    { ProfScope span(ctx, "detect");
      hipLaunchKernelGGL(detect_cells, dim3(n_cells, S), dim3(DET_THREADS), lds_bytes, ctx->stream, A);
      hipLaunchKernelGGL(detect_compact, dim3(S), dim3(1024), 0, ctx->stream, (const int64_t *)A.cell_out, (const int *)A.cell_cnt, n_cells, kmax,
                         d_out, (int)pairs, A.k_s); }
    HIP_TRY(ctx, hipGetLastError());
    int64_t *h_out = (int64_t *)(h + in_b);
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, out_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    size_t tot = 0;
    for (int s = 0; s < S; s++) tot += (size_t)h_out[(size_t)s * (1 + 2 * pairs)];
    if (tot > (size_t)cap) return slam_fail(ctx, SLAM_ERR_CAPACITY, "slam_detect_batch: %zu keypoints but cap = %d", tot, cap);
    size_t o = 0;
    for (int s = 0; s < S; s++) {
        const int64_t *hs = h_out + (size_t)s * (1 + 2 * pairs);
        memcpy(out_rc + 2 * o, hs + 1, (size_t)hs[0] * 16);
        o += (size_t)hs[0]; out_off[s + 1] = (int32_t)o;
    }
    return SLAM_OK;
}

// What slam_kpset_detect_describe reports of an unselected stream z (mask[z] == 0): info[2 z] = its id counter, info[2 z + 1] = 0 keypoints appended, and
// cnt0[z] = count[z], so that k_brief_patch finds no appended slot of it (it writes the same 0 and none of the stream's descriptor rows).  A selected
// stream's entries are detect_box_filter's and k_brief_patch's.  One thread per stream.
__global__ __launch_bounds__(64) void k_unselected_info(const uint8_t *mask, int S, const int *count, const int64_t *next_id, int *cnt0, int64_t *info)
{
    const int z = blockIdx.x * 64 + threadIdx.x;
    if (z >= S || mask[z]) return;
    cnt0[z] = count[z]; info[2 * z] = next_id[z]; info[2 * z + 1] = 0;
}

// What slam_kpset_detect and slam_kpset_detect_describe share.  kpset_detect_check: the checks both make after their null checks, in their order; kpset_detect_plan:
// det_plan on the set's current lists and the scratch of the cell lists, `extra` bytes behind them at D.extra; kpset_detect_append: the merge of the cell lists into the set.
struct KpDetect { int max_points, radius, grid_rows, grid_cols, cell_size, n_cells, kmax; DetectArgs A; size_t lds_bytes; char *extra; };
static int kpset_detect_check(slam_ctx *ctx, const slam_kpset *ks, const slam_pyr *pyr0, int max_points, int radius, int grid_rows, int grid_cols, int cell_size, KpDetect &D)
{
    ARG_TRY(ctx, pyr0->batch_index == 0 && pyr0->batch_size >= ks->S);
    ARG_TRY(ctx, grid_rows > 0 && grid_cols > 0 && cell_size >= 8 && radius > 0 && radius <= DET_MAXR && max_points > 0);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int n_cells = grid_rows * grid_cols;
    ARG_TRY(ctx, ks->v.cap >= max_points + n_cells);                // a stream below max_points may receive up to n_cells * k > max_points - n_cur keypoints
    D.max_points = max_points; D.radius = radius; D.grid_rows = grid_rows; D.grid_cols = grid_cols; D.cell_size = cell_size;
    D.n_cells = n_cells; D.kmax = (max_points + n_cells - 1) / n_cells;      // n_cur = 0
    return SLAM_OK;
}
static int kpset_detect_plan(slam_ctx *ctx, const slam_kpset *ks, const slam_pyr *pyr0, double sigma_mask, double min_response, size_t extra, KpDetect &D)
{
    int rc = det_plan(ctx, D.A, pyr0->plane(0, 0), pyr0->H[0], pyr0->W[0], pyr0->P[0], pyr0->zstride, D.max_points, D.radius, D.grid_rows, D.grid_cols, D.cell_size,
                      D.kmax, sigma_mask, min_response, &D.lds_bytes);
    if (rc) return rc;
    D.A.cur = ks->v.yx; D.A.cur_cnt = ks->v.count; D.A.cur_stride = ks->v.cap;
    Layout L;
    const auto o_cnt = L.take<int>((size_t)ks->S * D.n_cells); const auto o_cout = L.take<int64_t>((size_t)ks->S * D.n_cells * D.kmax * 2); const auto o_extra = L.take<char>(extra);
    char *d;
    rc = slam_scratch(ctx, L.size(), (void **)&d);
    if (rc) return rc;
    D.A.cell_cnt = o_cnt.at(d); D.A.cell_out = o_cout.at(d); D.extra = o_extra.at(d);
    return SLAM_OK;
}
static void kpset_detect_append(slam_ctx *ctx, slam_kpset *ks, const KpDetect &D)
{
    if (const int *sel = kpset_sel_table(ks))
        hipLaunchKernelGGL(detect_append_sel, dim3(ks->n_sel), dim3(1024), 0, ctx->stream, (const int64_t *)D.A.cell_out, (const int *)D.A.cell_cnt, D.n_cells, D.kmax,
                           D.max_points, ks->v, ks->next_id, sel);
    else
        hipLaunchKernelGGL(detect_append, dim3(ks->S), dim3(1024), 0, ctx->stream, (const int64_t *)D.A.cell_out, (const int *)D.A.cell_cnt, D.n_cells, D.kmax,
                           D.max_points, ks->v, ks->next_id);
}
// detect_cells over the streams the set's selection names (all of them without one); the caller has returned before when no stream is selected
static int kpset_detect_cells(slam_ctx *ctx, const slam_kpset *ks, const KpDetect &D)
{
    if (const int *sel = kpset_sel_table(ks)) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void *)detect_cells_sel, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));     // (as det_plan for detect_cells)
        hipLaunchKernelGGL(detect_cells_sel, dim3(D.n_cells, ks->n_sel), dim3(DET_THREADS), D.lds_bytes, ctx->stream, D.A, sel);
    } else
        hipLaunchKernelGGL(detect_cells, dim3(D.n_cells, ks->S), dim3(DET_THREADS), D.lds_bytes, ctx->stream, D.A);
    return SLAM_OK;
}

extern "C" int slam_kpset_detect(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *pyr0, int max_points, int radius, int grid_rows, int grid_cols,
                                 int cell_size, double sigma_mask, double min_response)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && pyr0 != nullptr);
    KpDetect D;
    int rc = kpset_detect_check(ctx, ks, pyr0, max_points, radius, grid_rows, grid_cols, cell_size, D);
    if (rc || kpset_none_selected(ks)) return rc;
    rc = kpset_detect_plan(ctx, ks, pyr0, sigma_mask, min_response, 0, D);
    if (rc) return rc;
    { ProfScope span(ctx, "detect");
      rc = kpset_detect_cells(ctx, ks, D);
      if (rc) return rc;
      kpset_detect_append(ctx, ks, D); }
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

// extract_keypoints! with describe (map_manager.jl:98-113) on the lists: detect_cells, the border drop, detect_append, k_brief_patch over
// the appended slots.  Enqueue-only.
extern "C" int slam_kpset_detect_describe(slam_ctx *ctx, slam_kpset *ks, const slam_pyr *pyr0, int max_points, int radius, int grid_rows, int grid_cols,
                                          int cell_size, double sigma_mask, double min_response, const int32_t *pattern, int n_bits, double sigma,
                                          int window, uint64_t *desc_dev, int64_t *info_dev, int dcap)
{
    ARG_TRY(ctx, ctx != nullptr && ks != nullptr && pyr0 != nullptr && desc_dev != nullptr && info_dev != nullptr);
    const int S = ks->S;
    KpDetect D;
    int rc = kpset_detect_check(ctx, ks, pyr0, max_points, radius, grid_rows, grid_cols, cell_size, D);
    if (rc) return rc;
    if (dcap < D.n_cells * D.kmax)
        return slam_fail(ctx, SLAM_ERR_ARG, "slam_kpset_detect_describe: dcap = %d, a key-frame may append %d keypoints per stream", dcap, D.n_cells * D.kmax);
    BriefJob J;
    rc = brief_prepare(ctx, "slam_kpset_detect_describe", pyr0->plane(0, 0), pyr0->H[0], pyr0->W[0], pyr0->P[0], pyr0->zstride, pattern, n_bits,
                       sigma, window, &J);
    if (!rc) rc = kpset_detect_plan(ctx, ks, pyr0, sigma_mask, min_response, (size_t)S * 4, D);
    if (rc) return rc;
    int *cnt0 = (int *)D.extra;
    const int *sel = kpset_sel_table(ks);
    if (sel) {                                                      // the unselected streams' report; with no stream selected that is the whole call
        hipLaunchKernelGGL(k_unselected_info, dim3((S + 63) / 64), dim3(64), 0, ctx->stream, (const uint8_t *)ks->sel_mask, S, (const int *)ks->v.count,
                           (const int64_t *)ks->next_id, cnt0, info_dev);
        HIP_TRY(ctx, hipGetLastError());
        if (kpset_none_selected(ks)) return SLAM_OK;
    }
    { ProfScope span(ctx, "detect");
      { ProfScope cells(ctx, "detect_cells");                       // (the yardstick scripts/probes/prof_describe.py quotes the describe stage against)
        rc = kpset_detect_cells(ctx, ks, D);
        if (rc) return rc; }
      if (sel)
          hipLaunchKernelGGL(detect_box_filter_sel, dim3((D.n_cells + 255) / 256, ks->n_sel), dim3(256), 0, ctx->stream, D.A.cell_out, D.A.cell_cnt, D.n_cells, D.kmax, max_points,
                             (const int *)ks->v.count, (const int64_t *)ks->next_id, pyr0->H[0], pyr0->W[0], (window + 1) / 2, cnt0, info_dev, sel);
      else
          hipLaunchKernelGGL(detect_box_filter, dim3((D.n_cells + 255) / 256, S), dim3(256), 0, ctx->stream, D.A.cell_out, D.A.cell_cnt, D.n_cells, D.kmax, max_points,
                             (const int *)ks->v.count, (const int64_t *)ks->next_id, pyr0->H[0], pyr0->W[0], (window + 1) / 2, cnt0, info_dev);
      kpset_detect_append(ctx, ks, D); }
    HIP_TRY(ctx, hipGetLastError());
    J.yx = ks->v.yx; J.cnt0 = cnt0; J.count = ks->v.count; J.cap = ks->v.cap; J.dcap = dcap; J.info = info_dev; J.out = desc_dev;
    return brief_launch(ctx, J, D.n_cells * D.kmax, S);
}
