// ba_math.hpp -- the arithmetic that every route of the local bundle adjustment shares, ONE copy of each formula: the LM constants and state, the
// clamped damping, the per-point solve, the products of one observation's Jacobians, and LeastSquaresOptim's step decision with the pass bookkeeping.
// The grouped single-window kernels, the pair-list fall-back, the batch kernels (vector and matrix-core builds), k_ba_window and k_pnp must agree, partly
// to the bit (tests/test_gpu_ba_batch.py, tests/test_gpu_ba_stages.py): they call these routines.  Operand order and association are part of each
// routine's contract (the library is built with -ffp-contract=off); tests/test_ba_math_host.py replays them on the host, every double compared with ==.
// Host/device like pyr_iir.hpp: no HIP call, no common.hpp -- tests/c_host/ba_math_check.cpp includes this header alone.
#pragma once
#include <cmath>

// (both branches are built: the library by hipcc, the stand-alone check by the host compiler alone)
#if defined(__HIPCC__)
#define BAM_HD __host__ __device__ __forceinline__
#define BAM_UNROLL _Pragma("unroll")
#else
#define BAM_HD static inline
#define BAM_UNROLL
#endif

#define LM_MAX_DELTA 1e16
#define LM_MIN_DELTA 1e-16
#define LM_MIN_STEP_QUALITY 1e-3
#define LM_MIN_DIAGONAL 1e-6
#define LM_MAX_DIAGONAL 1e32
#define LM_DELTA0 10.0
#define LM_XTOL 1e-8
#define LM_FTOL 1e-8

struct LMState {
    double delta, decrease_factor, ssr, trial_ssr, pred_ssr, maxdx;
    double ssr_init, ssr_pass1, ssr_final;
    int converged, accept, iters, n_outliers, chol_fail, iters_pass1, iters_pass2;
    int cur;                     // which of the two parameter buffers is the committed one: an accepted step SWAPS them (lm_decide) -- no copy
                                 // kernel per iteration (k_commit cost the iteration a launch: ~5 us of its 127)
};

// ---- damping ---------------------------------------------------------------------------------------------------------------------------------------
// LeastSquaresOptim's damping of one diagonal entry: the entry clamped to [LM_MIN_DIAGONAL, LM_MAX_DIAGONAL], times 1 / delta.  The caller adds it.
BAM_HD double lm_damp(double diag, double inv_delta) { return fmin(fmax(diag, LM_MIN_DIAGONAL), LM_MAX_DIAGONAL) * inv_delta; }

// inverse of the symmetric 3 x 3 matrix V = [V0 V1 V2; V1 V3 V4; V2 V4 V5] by cofactors; I in the same packing
BAM_HD void inv3_sym(const double V[6], double I[6])
{
    const double a = V[0], b = V[1], c = V[2], dd = V[3], e = V[4], f = V[5];
    const double A = dd * f - e * e, B = c * e - b * f, C = b * e - c * dd;
    const double det = a * A + b * B + c * C, id = 1.0 / det;
    I[0] = A * id; I[1] = B * id; I[2] = C * id;
    I[3] = (a * f - c * c) * id; I[4] = (b * c - a * e) * id; I[5] = (a * dd - b * b) * id;
}
// a map point's block: V = sum Jl'Jl (packed as above; further entries of the caller's array are not touched) gets its damping IN PLACE, Vi = V^-1
BAM_HD void point_solve(double *V, double inv_delta, double Vi[6])
{
    V[0] += lm_damp(V[0], inv_delta);
    V[3] += lm_damp(V[3], inv_delta);
    V[5] += lm_damp(V[5], inv_delta);
    inv3_sym(V, Vi);
}

// ---- one observation: Jp 2 x 6 and Jl 2 x 3, row-major; r = its residual ------------------------------------------------------------------------
// v[0..5] = Jl'Jl (packed), v[6..8] = Jl'r; every entry is (row 0 product) + (row 1 product)
BAM_HD void jl_products(const double Jl[6], const double r[2], double *v)
{
    v[0] = Jl[0] * Jl[0] + Jl[3] * Jl[3]; v[1] = Jl[0] * Jl[1] + Jl[3] * Jl[4]; v[2] = Jl[0] * Jl[2] + Jl[3] * Jl[5];
    v[3] = Jl[1] * Jl[1] + Jl[4] * Jl[4]; v[4] = Jl[1] * Jl[2] + Jl[4] * Jl[5]; v[5] = Jl[2] * Jl[2] + Jl[5] * Jl[5];
    BAM_UNROLL
    for (int k = 0; k < 3; k++) v[6 + k] = Jl[k] * r[0] + Jl[3 + k] * r[1];
}
// row a (0 .. 5) of W = Jp'Jl
BAM_HD void w_row(const double *Jp, const double *Jl, int a, double w[3])
{
    w[0] = Jp[a] * Jl[0] + Jp[6 + a] * Jl[3];
    w[1] = Jp[a] * Jl[1] + Jp[6 + a] * Jl[4];
    w[2] = Jp[a] * Jl[2] + Jp[6 + a] * Jl[5];
}
// out = Vi b for the packed symmetric Vi, each entry summed left to right (= b'Vi: the rows of W V^-1)
BAM_HD void sym3_mul(const double *Vi, const double *b, double &out0, double &out1, double &out2)
{
    out0 = Vi[0] * b[0] + Vi[1] * b[1] + Vi[2] * b[2];
    out1 = Vi[1] * b[0] + Vi[3] * b[1] + Vi[4] * b[2];
    out2 = Vi[2] * b[0] + Vi[4] * b[1] + Vi[5] * b[2];
}
// (a, b) += Jp dp: the two rows of six, entry by entry in turn
BAM_HD void jp_dot(const double *jp, const double *dp, double &a, double &b)
{
    BAM_UNROLL
    for (int k = 0; k < 6; k++) { a += jp[k] * dp[k]; b += jp[6 + k] * dp[k]; }
}
// _ba_detect_outliers! (bundle_adjustment.jl:90-111): behind the camera, or a squared reprojection error ABOVE the threshold (equality is an inlier on both)
BAM_HD bool obs_is_outlier(double z, const double r[2], double depth_eps, double repr_eps) { return z < depth_eps || (r[0] * r[0] + r[1] * r[1]) > repr_eps; }

// ---- the LM state: SP = LMState *, a pointer typed as global memory, or k_ba_window's copy in LDS ----------------------------------------------------
// start of a pass: the trust region and the counters of LeastSquaresOptim's loop (s->ssr holds the cost of the committed parameters already)
template <class SP> BAM_HD void lm_trust_reset(SP s)
{
    s->delta = LM_DELTA0; s->decrease_factor = 2.0; s->converged = 0; s->accept = 0; s->iters = 0;
}
// ... of the FIRST pass, before lm_trust_reset.  outliers = false: the sharded protocol's k_lm_start, which leaves n_outliers alone.
template <class SP> BAM_HD void lm_first_pass(SP s, bool outliers = true)
{
    s->ssr_init = s->ssr; s->chol_fail = 0;
    if (outliers) s->n_outliers = 0;
}
// end of pass 1 / pass 2
template <class SP> BAM_HD void lm_record_pass(SP s, int pass)
{
    if (pass == 1) { s->ssr_pass1 = s->ssr; s->iters_pass1 = s->iters; } else { s->ssr_final = s->ssr; s->iters_pass2 = s->iters; }
}
// LeastSquaresOptim's accept / reject of a trial step (trust-region radius update, step-quality test): t = trial cost,
// p = predicted cost, mx = max |dx|.  (pnp_lm in ba_single.hip keeps the same rule on local variables: a change here is a change there.)
template <class SP> BAM_HD void lm_decide(SP s, double t, double p, double mx)
{
    s->iters++;
    if (s->chol_fail) { s->converged = 1; s->accept = 0; return; }
    const double ssr = s->ssr;
    const double rho = (t - ssr) / (p - ssr);
    if (rho > LM_MIN_STEP_QUALITY) {
        const int x_conv = mx <= LM_XTOL;
        const int f_conv = fabs(ssr - t) / (fabs(ssr) + LM_FTOL) <= LM_FTOL;
        s->ssr = t;
        const double u = 2.0 * rho - 1.0;
        s->delta = fmin(s->delta / fmax(1.0 / 3.0, 1.0 - u * u * u), LM_MAX_DELTA);
        s->decrease_factor = 2.0;
        s->accept = 1;
        s->cur ^= 1;                                         // the trial parameters become the committed ones
        s->converged = x_conv || f_conv;
    } else {
        s->delta = fmax(s->delta / s->decrease_factor, LM_MIN_DELTA);
        s->decrease_factor *= 2.0;
        s->accept = 0;
        s->converged = mx <= LM_XTOL;
    }
}
