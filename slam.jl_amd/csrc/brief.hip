// brief.hip -- BRIEF-256 descriptors (describe -> ImageFeatures.create_descriptor,
// src/extractor.jl:103-105; off by default in the reference: params.jl:69).
//
// Two full-frame separable FIR passes (Gaussian sigma = sqrt(2), `window` taps,
// replicate border) and one wave per keypoint: each lane evaluates the
// intensity-pair tests lane, lane+64, ... and a wave ballot packs 64 test
// results into one descriptor word.
//
// The device-pyramid forms (slam_describe_pyr, slam_describe_batch, slam_kpset_detect_describe in detect.hip) never form the smoothed
// frame: k_brief_patch smooths the (2 lim + 1)^2 neighbourhood of each keypoint in LDS, from the raw patch read out of the pyramid's
// level-0 plane, with the arithmetic of the two full-frame passes.
#include "common.hpp"
#include <cmath>

#define BRIEF_MAXTAPS 41
struct Taps { double w[BRIEF_MAXTAPS]; int n; };

__global__ __launch_bounds__(256) void k_fir_y(double *dst, const double *src, int H, int W, Taps t)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i % H), x = (int)(i / H), hw = t.n >> 1;
    double acc = 0.0;
    for (int j = 0; j < t.n; j++) { int yy = y + j - hw; yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy); acc += src[(size_t)yy + (size_t)x * H] * t.w[j]; }
    dst[i] = acc;
}
__global__ __launch_bounds__(256) void k_fir_x(double *dst, const double *src, int H, int W, Taps t)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i % H), x = (int)(i / H), hw = t.n >> 1;
    double acc = 0.0;
    for (int j = 0; j < t.n; j++) { int xx = x + j - hw; xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx); acc += src[(size_t)y + (size_t)xx * H] * t.w[j]; }
    dst[i] = acc;
}

__global__ __launch_bounds__(64) void k_brief(const double *sm, int H, const int64_t *rc, const int32_t *pattern, int n_bits, uint64_t *out)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const long y = rc[2 * k], x = rc[2 * k + 1];
    const int words = n_bits >> 6;
    for (int w = 0; w < words; w++) {
        const int32_t *p = pattern + 4 * (w * 64 + lane);
        const double v1 = sm[(size_t)(y - 1 + p[0]) + (size_t)(x - 1 + p[1]) * H];
        const double v2 = sm[(size_t)(y - 1 + p[2]) + (size_t)(x - 1 + p[3]) * H];
        const unsigned long long m = __ballot(v1 < v2);
        if (lane == 0) out[(size_t)k * words + w] = m;
    }
}

// ImageFeatures' BRIEF smoothing kernel: exp(-x^2 / (2 sigma^2)) over `window` taps, normalised by their sum (both describe paths)
static void brief_taps(double sigma, int window, double *w)
{
    const int hw = window >> 1;
    double s = 0;
    for (int i = 0; i < window; i++) { double x = i - hw; w[i] = std::exp(-(x * x) / (2.0 * (sigma * sigma))); s += w[i]; }
    for (int i = 0; i < window; i++) w[i] = w[i] / s;
}

// keypoints whose +-ceil(window/2) box leaves the image are dropped (1-based row, col)
static inline bool brief_in_box(int64_t y, int64_t x, int H, int W, int lim) { return !(y - lim < 1 || y + lim > H || x - lim < 1 || x + lim > W); }

// One wave per keypoint, four keypoints per workgroup; wave-private LDS regions raw (Nr x Nr) | mid (Ns x Nr) | sm (Ns x Ns), all column-major
// (row fastest), with lim = (window + 1) / 2, hw = window / 2, Ns = 2 lim + 1, Nr = Ns + 2 hw.
//   stage: raw(r, c) = image(clamp(yc - lim - hw + r), clamp(xc - lim - hw + c))            -- the replicate border of both passes
//   dim 1: mid(rs, c) = sum_j raw(rs + j, c) w[j]       (k_fir_y at row yc - lim + rs of the clamped column c)
//   dim 2: sm(rs, cs) = sum_j mid(rs, cs + j) w[j]      (k_fir_x at column xc - lim + cs; a clamped column's dim-1 result is its border value)
// acc = 0; acc += v * w[j], j ascending, uncontracted: bit for bit what k_fir_y / k_fir_x leave in the smoothed frame.  The stages hand over
// through workgroup barriers (every wave takes part, with or without a keypoint): LDS writes are not assumed visible by wave lock-step.
// Every global read is clamped into the image and every pattern offset was checked against +-lim on the host: no index depends on the
// keypoint having passed the box test.
__global__ __launch_bounds__(256) void k_brief_patch(BriefJob J)
{
    extern __shared__ double bp_lds[];
    __shared__ double s_w[BRIEF_PATCH_MAXWIN];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int window = J.window, lim = (window + 1) >> 1, hw = window >> 1, Ns = 2 * lim + 1, Nr = Ns + 2 * hw;
    const int words = J.n_bits >> 6;
    double *raw = bp_lds + (size_t)wv * (Nr * Nr + Ns * Nr + Ns * Ns), *mid = raw + Nr * Nr, *sm = mid + Ns * Nr;
    if (tid < BRIEF_PATCH_MAXWIN) {                               // (statically indexed reads of the by-value taps: no scratch copy of the struct)
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < BRIEF_PATCH_MAXWIN; j++) v = tid == j ? J.w[j] : v;
        s_w[tid] = v;
    }
    bool act = false;
    long y = 1, x = 1; int z = 0; uint64_t *out = nullptr;
    const int j = blockIdx.x * 4 + wv;
    if (J.rc) {
        act = j < J.n;
        if (act) { y = (long)J.rc[2 * (size_t)j]; x = (long)J.rc[2 * (size_t)j + 1]; z = J.member ? J.member[j] : 0; out = J.out + (size_t)j * words; }
    } else {
        z = blockIdx.y;
        const int n0 = J.cnt0[z], n1 = J.count[z];
        if (blockIdx.x == 0 && tid == 0) J.info[2 * z + 1] = n1 - n0;
        act = n0 + j < n1 && j < J.dcap;
        if (act) { const size_t q = (size_t)z * J.cap + n0 + j; y = (long)J.yx[2 * q]; x = (long)J.yx[2 * q + 1]; out = J.out + ((size_t)z * J.dcap + j) * words; }
    }
    const double *img = J.img + (size_t)z * J.zs;
    const int yc = (int)y - 1, xc = (int)x - 1, H = J.H, W = J.W;
    if (act)
        for (int e = lane; e < Nr * Nr; e += 64) {
            const int c = e / Nr, r = e - c * Nr;
            int gy = yc - lim - hw + r, gx = xc - lim - hw + c;
            gy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy); gx = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
            raw[e] = img[(size_t)gx * J.P + gy];
        }
    __syncthreads();                                              // raw patch and taps written
    if (act)
        for (int e = lane; e < Ns * Nr; e += 64) {
            const int c = e / Ns, rs = e - c * Ns;
            const double *p = raw + c * Nr + rs;
            double acc = 0.0;
            for (int t = 0; t < window; t++) acc += p[t] * s_w[t];
            mid[e] = acc;
        }
    __syncthreads();                                              // dim-1 results written
    if (act)
        for (int e = lane; e < Ns * Ns; e += 64) {
            const int cs = e / Ns, rs = e - cs * Ns;
            const double *p = mid + cs * Ns + rs;
            double acc = 0.0;
            for (int t = 0; t < window; t++) acc += p[t * Ns] * s_w[t];
            sm[e] = acc;
        }
    __syncthreads();                                              // smoothed neighbourhood written
    if (act)                                                      // (wave-uniform: the ballot sees the whole wave)
        for (int w = 0; w < words; w++) {
            const int4 p = ((const int4 *)J.pattern)[w * 64 + lane];
            const double v1 = sm[(p.y + lim) * Ns + (p.x + lim)];
            const double v2 = sm[(p.w + lim) * Ns + (p.z + lim)];
            const unsigned long long m = __ballot(v1 < v2);
            if (lane == 0) out[w] = m;
        }
}

int brief_prepare(slam_ctx *ctx, const char *who, const double *img, int H, int W, int P, size_t zs, const int32_t *pattern, int n_bits,
                  double sigma, int window, BriefJob *J)
{
    ARG_TRY(ctx, img != nullptr && pattern != nullptr && n_bits > 0 && n_bits % 64 == 0 && window > 0 && window % 2 == 1 && sigma > 0);
    if (window > BRIEF_PATCH_MAXWIN)
        return slam_fail(ctx, SLAM_ERR_ARG, "%s: window %d, the device-pyramid forms take odd windows up to %d", who, window, BRIEF_PATCH_MAXWIN);
    const int lim = (window + 1) / 2;
    for (int b = 0; b < n_bits; b++)
        for (int c = 0; c < 4; c++)
            if (pattern[4 * b + c] < -lim || pattern[4 * b + c] > lim)
                return slam_fail(ctx, SLAM_ERR_ARG, "%s: pattern offset %d outside +-%d", who, pattern[4 * b + c], lim);
    const size_t n = (size_t)n_bits * 4;
    if (ctx->brief_pat_host.size() != n || memcmp(ctx->brief_pat_host.data(), pattern, n * 4) != 0) {
        if (!ctx->brief_pat_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->brief_pat_ev, hipEventDisableTiming));
        else HIP_TRY(ctx, hipEventSynchronize(ctx->brief_pat_ev));           // the previous upload has read the pinned block (long ago)
        if (ctx->brief_pat_cap < n) {
            HIP_TRY(ctx, slam_stream_wait(ctx->stream));                      // kernels in flight read the table being replaced
            if (ctx->brief_pat_dev) (void)hipFree(ctx->brief_pat_dev);
            if (ctx->brief_pat_pin) (void)hipHostFree(ctx->brief_pat_pin);
            ctx->brief_pat_dev = nullptr; ctx->brief_pat_pin = nullptr; ctx->brief_pat_cap = 0; ctx->brief_pat_host.clear();
            const size_t cap = n < 4096 ? 4096 : n;
            HIP_TRY(ctx, hipMalloc((void **)&ctx->brief_pat_dev, cap * 4));
            HIP_TRY(ctx, hipHostMalloc((void **)&ctx->brief_pat_pin, cap * 4));
            ctx->brief_pat_cap = cap;
        }
        ctx->brief_pat_host.clear();
        memcpy(ctx->brief_pat_pin, pattern, n * 4);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->brief_pat_dev, ctx->brief_pat_pin, n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->brief_pat_ev, ctx->stream));
        ctx->brief_pat_host.assign(pattern, pattern + n);
    }
    memset(J, 0, sizeof(*J));
    J->img = img; J->H = H; J->W = W; J->P = P; J->zs = zs;
    J->pattern = ctx->brief_pat_dev; J->n_bits = n_bits; J->window = window;
    brief_taps(sigma, window, J->w);
    return SLAM_OK;
}

int brief_launch(slam_ctx *ctx, const BriefJob &J, int per_stream, int S)
{
    if (per_stream <= 0 || S <= 0) return SLAM_OK;
    const int lim = (J.window + 1) / 2, hw = J.window >> 1, Ns = 2 * lim + 1, Nr = Ns + 2 * hw;
    const size_t lds = (size_t)4 * (Nr * Nr + Ns * Nr + Ns * Ns) * sizeof(double);      // <= 56 864 bytes at window 15
    { ProfScope span(ctx, "describe");
      hipLaunchKernelGGL(k_brief_patch, dim3((per_stream + 3) / 4, S), dim3(256), lds, ctx->stream, J); }
    HIP_TRY(ctx, hipGetLastError());
    return SLAM_OK;
}

// the list forms: box test on the host (order kept), one launch over the survivors, descriptors back
static int describe_lists(slam_ctx *ctx, const char *who, const slam_pyr *pyr0, int S, bool batch, const int64_t *rc, const int32_t *off,
                          const int32_t *pattern, int n_bits, double sigma, int window, uint64_t *out_bits, int64_t *out_rc, int32_t *out_off)
{
    BriefJob J;
    // (pyr0->plane(0, 0) is that pyramid's own plane: the single form describes a batch member like any other pyramid, stride unused)
    int r = brief_prepare(ctx, who, pyr0->plane(0, 0), pyr0->H[0], pyr0->W[0], pyr0->P[0], batch ? pyr0->zstride : 0, pattern, n_bits, sigma, window, &J);
    if (r) return r;
    const int lim = (window + 1) / 2, n = off[S];
    std::vector<int64_t> keep; keep.reserve((size_t)n * 2);
    std::vector<int32_t> member; member.reserve((size_t)n);
    out_off[0] = 0;
    for (int s = 0; s < S; s++) {
        for (int k = off[s]; k < off[s + 1]; k++)
            if (brief_in_box(rc[2 * k], rc[2 * k + 1], J.H, J.W, lim)) { keep.push_back(rc[2 * k]); keep.push_back(rc[2 * k + 1]); member.push_back(s); }
        out_off[s + 1] = (int32_t)member.size();
    }
    const int m = (int)member.size();
    if (m == 0) return SLAM_OK;
    const size_t words = (size_t)n_bits / 64;
    Layout D;
    const auto o_rc = D.take<int64_t>((size_t)m * 2); const auto o_mem = D.take<int32_t>(m); const auto o_out = D.take<uint64_t>((size_t)m * words);
    char *s;
    r = slam_scratch(ctx, D.size(), (void **)&s);
    if (r) return r;
    HIP_TRY(ctx, hipMemcpyAsync(o_rc.at(s), keep.data(), o_rc.bytes(), hipMemcpyHostToDevice, ctx->stream));
    if (batch) HIP_TRY(ctx, hipMemcpyAsync(o_mem.at(s), member.data(), o_mem.bytes(), hipMemcpyHostToDevice, ctx->stream));
    J.rc = o_rc.at(s); J.member = batch ? o_mem.at(s) : nullptr; J.n = m; J.out = o_out.at(s);
    r = brief_launch(ctx, J, m, 1);
    if (r) return r;
    HIP_TRY(ctx, hipMemcpyAsync(out_bits, J.out, o_out.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));                  // (the pageable sources above are read by now as well)
    memcpy(out_rc, keep.data(), (size_t)m * 16);
    return SLAM_OK;
}

extern "C" int slam_describe_pyr(slam_ctx *ctx, const slam_pyr *pyr, const int64_t *rc, int n, const int32_t *pattern, int n_bits,
                                 double sigma, int window, uint64_t *out_bits, int64_t *out_rc, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && pyr != nullptr && n >= 0 && n_out != nullptr);
    ARG_TRY(ctx, n == 0 || (rc != nullptr && out_bits != nullptr && out_rc != nullptr));
    *n_out = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int32_t off[2] = {0, n}; int32_t out_off[2] = {0, 0};
    int r = describe_lists(ctx, "slam_describe_pyr", pyr, 1, false, rc, off, pattern, n_bits, sigma, window, out_bits, out_rc, out_off);
    if (r) return r;
    *n_out = out_off[1];
    return SLAM_OK;
}

extern "C" int slam_describe_batch(slam_ctx *ctx, const slam_pyr *pyr0, int S, const int64_t *rc, const int32_t *off, const int32_t *pattern,
                                   int n_bits, double sigma, int window, uint64_t *out_bits, int64_t *out_rc, int32_t *out_off)
{
    ARG_TRY(ctx, ctx != nullptr && pyr0 != nullptr && S >= 1 && S <= 128 && off != nullptr && out_off != nullptr);
    ARG_TRY(ctx, pyr0->batch_index == 0 && pyr0->batch_size >= S);
    ARG_TRY(ctx, off[0] == 0);
    for (int s = 0; s < S; s++) ARG_TRY(ctx, off[s + 1] >= off[s]);
    ARG_TRY(ctx, off[S] == 0 || (rc != nullptr && out_bits != nullptr && out_rc != nullptr));
    for (int s = 0; s <= S; s++) out_off[s] = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return describe_lists(ctx, "slam_describe_batch", pyr0, S, true, rc, off, pattern, n_bits, sigma, window, out_bits, out_rc, out_off);
}

extern "C" int slam_describe(slam_ctx *ctx, const double *image, int H, int W, const int64_t *rc, int n,
                             const int32_t *pattern, int n_bits, double sigma, int window,
                             uint64_t *out_bits, int64_t *out_rc, int *n_out)
{
    ARG_TRY(ctx, ctx != nullptr && image != nullptr && H > 0 && W > 0 && n >= 0 && n_out != nullptr);
    ARG_TRY(ctx, pattern != nullptr && n_bits > 0 && n_bits % 64 == 0 && window > 0 && window % 2 == 1 && window <= BRIEF_MAXTAPS && sigma > 0);
    *n_out = 0;
    if (n == 0) return SLAM_OK;
    ARG_TRY(ctx, rc != nullptr && out_bits != nullptr && out_rc != nullptr);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // keypoints whose +-ceil(window/2) box leaves the image are dropped (order kept)
    const int lim = (window + 1) / 2;
    std::vector<int64_t> keep; keep.reserve((size_t)n * 2);
    for (int k = 0; k < n; k++) {
        int64_t y = rc[2 * k], x = rc[2 * k + 1];
        if (!brief_in_box(y, x, H, W, lim)) continue;
        keep.push_back(y); keep.push_back(x);
    }
    const int m = (int)(keep.size() / 2);
    for (int b = 0; b < n_bits; b++)
        for (int c = 0; c < 4; c++)
            if (pattern[4 * b + c] < -lim || pattern[4 * b + c] > lim)
                return slam_fail(ctx, SLAM_ERR_ARG, "slam_describe: pattern offset %d outside +-%d", pattern[4 * b + c], lim);
    if (m == 0) return SLAM_OK;
    Taps t; t.n = window;
    brief_taps(sigma, window, t.w);
    const size_t N = (size_t)H * W, words = (size_t)n_bits / 64;
    Layout D;
    const auto o_a = D.take<double>(N), o_b = D.take<double>(N); const auto o_rc = D.take<int64_t>((size_t)m * 2); const auto o_pat = D.take<int32_t>((size_t)n_bits * 4); const auto o_out = D.take<uint64_t>((size_t)m * words);
    char *s;
    int r = slam_scratch(ctx, D.size(), (void **)&s);
    if (r) return r;
    double *d_a = o_a.at(s), *d_b = o_b.at(s);
    int64_t *d_rc = o_rc.at(s); int32_t *d_pat = o_pat.at(s);
    uint64_t *d_out = o_out.at(s);
    HIP_TRY(ctx, hipMemcpyAsync(d_a, image, o_a.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_rc, keep.data(), o_rc.bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_pat, pattern, o_pat.bytes(), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_fir_y, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, d_b, (const double *)d_a, H, W, t);
    hipLaunchKernelGGL(k_fir_x, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, d_a, (const double *)d_b, H, W, t);
    hipLaunchKernelGGL(k_brief, dim3(m), dim3(64), 0, ctx->stream, (const double *)d_a, H, (const int64_t *)d_rc, (const int32_t *)d_pat, n_bits, d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_bits, d_out, o_out.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, slam_stream_wait(ctx->stream));
    memcpy(out_rc, keep.data(), (size_t)m * 16);
    *n_out = m;
    return SLAM_OK;
}
