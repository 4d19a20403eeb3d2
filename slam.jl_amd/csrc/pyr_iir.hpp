// pyr_iir.hpp -- the arithmetic of the pyramid's filters (pyramid.hip), one copy of each routine.
//
// The bit-exact planes rest on a few short formulas written in exactly the reference's operation order
// (ImageFiltering._imfilter_dim!(::TriggsSdika), ImageTransformations.imresize!): the kernels differ in how they move a
// line's samples, never in these formulas, so the formulas live here and the kernels call them.  Shared by the kernels,
// the host (the stand-alone check tests/c_host/pyr_iir_check.cpp) and nothing else.
//
// `IIRCoef` is common.hpp's; a host program that cannot include common.hpp declares a struct with the same members
// (a1, a2, a3, scale, M[9], inv1masum, inv1mbsum) before this header.
#pragma once
#include <cmath>

// (both branches are built: the library by hipcc, the stand-alone check by the host compiler alone)
#if defined(__HIPCC__)
#define PYR_HD __host__ __device__ __forceinline__
#define PYR_UNROLL _Pragma("unroll")
#else
#define PYR_HD static inline
#define PYR_UNROLL
#endif

// ---- one step of the third-order recurrence ---------------------------------------------------------------------------
// iir3<false>: the reference's operation order, ((x + a1 w1) + a2 w2) + a3 w3, every product and sum rounded.
// iir3<true> and rt_step are the two contracted forms of the tolerance build (mode 3), and they are NOT the same:
//     iir3<true>  = fma(a1, w1, fma(a2, w2, fma(a3, w3, x)))   the newest state w1 enters LAST: the dependent chain from
//                                                             one step to the next is a single fma (k_cols_fused<TOL>, k_iir_seg)
//     rt_step     = fma(a3, w3, fma(a2, w2, fma(a1, w1, x)))   the newest state enters FIRST: the sum is formed in the order of
//                                                             the exact form (k_rows_tol), a chain of three
// They round differently; each kernel keeps the order it was validated with.
template <bool TOL>
PYR_HD double iir3(double x, double a1, double w1, double a2, double w2, double a3, double w3)
{
    if (TOL) return __builtin_fma(a1, w1, __builtin_fma(a2, w2, __builtin_fma(a3, w3, x)));
    return ((x + a1 * w1) + a2 * w2) + a3 * w3;
}
PYR_HD double rt_step(double x, double a1, double a2, double a3, double w1, double w2, double w3)
{
    return __builtin_fma(a3, w3, __builtin_fma(a2, w2, __builtin_fma(a1, w1, x)));
}

// ---- left border: steady state of the constant input iminus, then the first three forward samples ----------------------
PYR_HD double iir_uminus(const IIRCoef &k, double iminus) { return iminus / k.inv1masum; }
struct IirHead { double uminus, o0, o1, o2; };
template <bool TOL>
PYR_HD IirHead iir_head(const IIRCoef &k, double x0, double x1, double x2, double iminus)
{
    IirHead h;
    h.uminus = iir_uminus(k, iminus);
    h.o0 = iir3<TOL>(x0, k.a1, h.uminus, k.a2, h.uminus, k.a3, h.uminus);
    h.o1 = iir3<TOL>(x1, k.a1, h.o0, k.a2, h.uminus, k.a3, h.uminus);
    h.o2 = iir3<TOL>(x2, k.a1, h.o1, k.a2, h.o0, k.a3, h.uminus);
    return h;
}

// ---- Triggs-Sdika right border ------------------------------------------------------------------------------------------
// (f1, f2, f3) = forward values at n-1, n-2, n-3; xlast = the border value iplus.  vr0 = v[n-1]; vr1, vr2 = the virtual
// samples v[n], v[n+1].  The matrix product is ((M0 d0 + M1 d1) + M2 d2) + vplus in every build, the tolerance ones included.
struct IirBoundary { double vr0, vr1, vr2; };
PYR_HD IirBoundary iir_boundary(const IIRCoef &k, double f1, double f2, double f3, double xlast)
{
    const double uplus = xlast / k.inv1masum, vplus = uplus / k.inv1mbsum;
    const double d0 = f1 - uplus, d1 = f2 - uplus, d2 = f3 - uplus;
    IirBoundary r;
    r.vr0 = ((k.M[0] * d0 + k.M[1] * d1) + k.M[2] * d2) + vplus;
    r.vr1 = ((k.M[3] * d0 + k.M[4] * d1) + k.M[5] * d2) + vplus;
    r.vr2 = ((k.M[6] * d0 + k.M[7] * d1) + k.M[8] * d2) + vplus;
    return r;
}
// ... and the three backward values the sweep starts from: vA = v[n-1], vB = v[n-2], vC = v[n-3] (unscaled)
struct IirTail { double vA, vB, vC; };
template <bool TOL>
PYR_HD IirTail iir_tail(const IIRCoef &k, double w1, double w2, double w3, double iplus)
{
    const IirBoundary r = iir_boundary(k, w1, w2, w3, iplus);
    IirTail t;
    t.vA = r.vr0;
    t.vB = iir3<TOL>(w2, k.a1, t.vA, k.a2, r.vr1, k.a3, r.vr2);
    t.vC = iir3<TOL>(w3, k.a1, t.vB, k.a2, t.vA, k.a3, r.vr1);
    return t;
}

// ---- a whole block of N samples in registers ----------------------------------------------------------------------------
// forward: x[e] <- the recurrence from the state (f1, f2, f3) before the block; KEEP = false advances the state only.
// (Partial blocks stay spelled out in the kernels, one predicated iir3 step per sample: through a predicated form of these helpers
//  the compiler turned the steps into selects, and the skipped steps of a short block then run through the dependent chain.)
template <int N, bool KEEP>
PYR_HD void iir_block_fwd(double *x, double a1, double a2, double a3, double &f1, double &f2, double &f3)
{
    PYR_UNROLL
    for (int e = 0; e < N; e++) { const double t = iir3<false>(x[e], a1, f1, a2, f2, a3, f3); f3 = f2; f2 = f1; f1 = t; if (KEEP) x[e] = t; }
}
// backward over the forward values, right to left from the state (v1, v2, v3) right of the block: x[e] <- t * scale
template <int N>
PYR_HD void iir_block_bwd(double *x, double a1, double a2, double a3, double scale, double &v1, double &v2, double &v3)
{
    PYR_UNROLL
    for (int e = N - 1; e >= 0; e--) { const double t = iir3<false>(x[e], a1, v1, a2, v2, a3, v3); v3 = v2; v2 = v1; v1 = t; x[e] = t * scale; }
}

// ---- the checkpointed row filter (k_iir_rows_ck, k_rows_cum): pass A and the checkpoints --------------------------------
// The line's samples 3 .. n-1 are cut into blocks of CK_B; the backward sweep needs forward values on [3, n-4] = m samples in nb
// blocks.  Pass A runs the forward recurrence over the whole line reading only, and keeps the state before every block j >= 1 of
// those nb (block 0 starts from the left border's o2, o1, o0).  The kernels differ in how they address the plane and the
// checkpoint scratch, which an accessor hides:
//     io.x(c0, e)     sample c0 + e of the line (plain load)          io.x_nt(c0, e)   the same as a streaming load
//     io.ckp(j)       the line's checkpoint of block j: w1 at [0], w2 at [io.nlines], w3 at [2 io.nlines]
#define CK_B 32
struct RowCk { int n, m, nb, nfull, rem; bool have_last; };
PYR_HD RowCk rowck_plan(int n)
{
    RowCk c;
    c.n = n; c.m = n - 6; c.nb = (c.m + CK_B - 1) / CK_B;
    c.nfull = (n - 3) / CK_B;                                   // blocks of pass A that are complete
    c.rem = (n - 3) - c.nfull * CK_B;                           // samples of the trailing partial block (block nfull), prefetched like the others
    c.have_last = c.nfull == c.nb - 1;                          // after pass A `cur` already holds the inputs of pass B's first block
    return c;
}
template <class Acc>
PYR_HD void rowck_load_x(const Acc &io, const RowCk &c, int j, double *buf)   // block j = samples [3 + j CK_B, ...), CK_B of them (clamped reads: zeros past the line)
{
    const int c0 = 3 + j * CK_B, len = c.n - c0;                // samples left in the line
    if (len >= CK_B) {
        PYR_UNROLL
        for (int e = 0; e < CK_B; e++) buf[e] = io.x_nt(c0, e);
    } else {
        PYR_UNROLL
        for (int e = 0; e < CK_B; e++) buf[e] = e < len ? io.x(c0, e) : 0.0;
    }
}
template <class Acc>
PYR_HD void rowck_store(const Acc &io, int j, double g1, double g2, double g3)
{
    double *c = io.ckp(j);
    c[0] = g1; c[io.nlines] = g2; c[2 * io.nlines] = g3;
}
template <class Acc>
PYR_HD void rowck_load(const Acc &io, int j, const IirHead &h, double &g1, double &g2, double &g3)
{
    if (j > 0) { const double *c = io.ckp(j); g1 = c[0]; g2 = c[io.nlines]; g3 = c[2 * io.nlines]; }
    else { g1 = h.o2; g2 = h.o1; g3 = h.o0; }
}
// pass A: forward over i = 3 .. n-1, block by block (the next block is requested while the current one runs): the c.nfull complete
// blocks and the checkpoint of the remainder.  The caller runs the remainder's c.rem samples (left in `cur`; they absorb the 3
// trailing samples n-3 .. n-1, which only the boundary computation needs) as predicated steps of its own, like every partial
// block.  (w1, w2, w3): o2, o1, o0 on entry, the forward state before the remainder on exit.
template <class Acc>
PYR_HD void rowck_pass_a(const Acc &io, const RowCk &c, double a1, double a2, double a3, double *cur, double *nxt, double &w1, double &w2, double &w3)
{
    rowck_load_x(io, c, 0, cur);
    for (int j = 0; j < c.nfull; j++) {
        rowck_load_x(io, c, j + 1, nxt);                        // (block nfull: clamped reads, the missing samples are zeros)
        if (j > 0 && j < c.nb) rowck_store(io, j, w1, w2, w3);
        iir_block_fwd<CK_B, false>(cur, a1, a2, a3, w1, w2, w3);
        PYR_UNROLL
        for (int e = 0; e < CK_B; e++) cur[e] = nxt[e];
    }
    // remainder (< CK_B samples, in `cur`): its start may still be a checkpoint
    if (c.nfull > 0 && c.nfull < c.nb) rowck_store(io, c.nfull, w1, w2, w3);
}

// ---- imresize!: source index and weight of one axis ---------------------------------------------------------------------
// Output sample k1 (1-based) of n_dst reads the source samples i, i + 1 (1-based) of n_src with weights 1 - f, f:
// c = s k1 + o with s = n_src / n_dst, o = 0.5 - 0.5 s; i = floor(c) clamped to [1, n_src - 1]; f = c - i.
// An enlargement (s < 1) clamps c to the source first.  Only k_resize's callers can get there: the kernels that fuse imresize!
// into a filter pass go from a level to the next smaller one and say so (may_enlarge = false, a constant: the clamp folds away).
// The axis (one division) is formed once per kernel, the coordinate per output sample.
struct ResizeAxis { double s, o; int n_src; bool clamp; };
struct ResizeCoord { int i; double f; };
PYR_HD ResizeAxis resize_axis(int n_src, int n_dst, bool may_enlarge = true)
{
    ResizeAxis ax;
    ax.s = (double)n_src / (double)n_dst; ax.o = 1 - 0.5 - ax.s * (1 - 0.5);
    ax.n_src = n_src; ax.clamp = may_enlarge && ax.s < 1;
    return ax;
}
PYR_HD ResizeCoord resize_coord(const ResizeAxis &ax, int k1)
{
    double c = ax.s * k1 + ax.o;
    if (ax.clamp) c = c < 1 ? 1 : (c > ax.n_src ? ax.n_src : c);
    ResizeCoord r;
    r.i = (int)floor(c);
    if (r.i > ax.n_src - 1) r.i = ax.n_src - 1;
    if (r.i < 1) r.i = 1;
    r.f = c - r.i;
    return r;
}

// ---- tolerance mode: the segments' affine maps s -> M^k s + z ------------------------------------------------------------
#define PAR_G 8                          // segments per group of the two-level folds
// (a, b, c) <- P (a, b, c) + (za, zb, zc), three fused multiply-adds per row (mode-3 kernels only: contracted)
PYR_HD void mv3(const double *P, double &a, double &b, double &c, double za, double zb, double zc)
{
    const double n1 = __builtin_fma(P[0], a, __builtin_fma(P[1], b, __builtin_fma(P[2], c, za)));
    const double n2 = __builtin_fma(P[3], a, __builtin_fma(P[4], b, __builtin_fma(P[5], c, zb)));
    const double n3 = __builtin_fma(P[6], a, __builtin_fma(P[7], b, __builtin_fma(P[8], c, zc)));
    a = n1; b = n2; c = n3;
}

#if defined(__HIPCC__)
// Sum of the totals of the segments before segment g of the thread's line (the start of its running sum), by the same two levels:
// Zt(s) = total of segment s (written here from `total`), Gt(h) = total of group h.  Every thread calls it (two barriers inside).
template <class ZAcc, class GAcc>
__device__ __forceinline__ double seg_running_sum(int g, bool has, double total, ZAcc Zt, GAcc Gt)
{
    if (has) Zt(g) = total;
    __syncthreads();
    const int q = g % PAR_G, grp = g / PAR_G;
    double pre = 0.0;
    if (has) for (int i = 0; i < q; i++) pre = pre + Zt(grp * PAR_G + i);
    if (has && q == PAR_G - 1) Gt(grp) = pre + Zt(g);
    __syncthreads();
    double base = 0.0;
    if (has) for (int h = 0; h < grp; h++) base = base + Gt(h);
    return base + pre;
}
#endif
