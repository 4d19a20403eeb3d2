// Stand-alone host replay of the local bundle adjustment's shared formulas (slam.jl_amd/csrc/ba_math.hpp), bit for bit.  Built and run by
// tests/test_ba_math_host.py (plain, and with -fsanitize=address,undefined,float-cast-overflow), which compares every printed double with a
// transcription of the routine in numpy float64.
//
// Commands on stdin, numbers as hex floats, one result line each:
//   damp <diag> <inv_delta>                         lm_damp
//   jlp <Jl 6> <r 2>                                jl_products: 9 doubles
//   psolve <inv_delta> <nobs> nobs x (<Jl 6> <r 2>) V[0..8] = the observations' jl_products summed in order, point_solve(V, inv_delta, Vi):
//                                                   V (9, damped in place), Vi (6)
//   wrow <Jp 12> <Jl 6>                             w_row for a = 0 .. 5: 18 doubles
//   sym3 <Vi 6> <b 3>                               sym3_mul: 3 doubles
//   jpdot <jp 12> <dp 6> <a> <b>                    jp_dot accumulating into (a, b): 2 doubles
//   outl <z> <r 2> <depth_eps> <repr_eps>           obs_is_outlier: 0 / 1
//   lm_set <17 fields of LMState in declaration order>     the state the next lm_* commands work on
//   lm_first <outliers 0 / 1> | lm_reset | lm_decide <t> <p> <mx> | lm_record <pass>      the routine on that state
//   every lm_* command prints the 17 fields of the state afterwards
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "ba_math.hpp"

static double num() { std::string t; if (!(std::cin >> t)) { std::printf("input ended early\n"); std::exit(2); } return std::strtod(t.c_str(), nullptr); }
static void nums(double *v, int n) { for (int i = 0; i < n; i++) v[i] = num(); }
static void put(const double *v, int n) { for (int i = 0; i < n; i++) std::printf("%a ", v[i]); std::printf("\n"); }

static LMState g_lm;
static void put_lm()
{
    const LMState &s = g_lm;
    const double v[17] = {s.delta, s.decrease_factor, s.ssr, s.trial_ssr, s.pred_ssr, s.maxdx, s.ssr_init, s.ssr_pass1, s.ssr_final,
                          (double)s.converged, (double)s.accept, (double)s.iters, (double)s.n_outliers, (double)s.chol_fail, (double)s.iters_pass1, (double)s.iters_pass2, (double)s.cur};
    put(v, 17);
}

int main()
{
    std::string c;
    while (std::cin >> c) {
        if (c == "damp") { const double d = num(), i = num(); const double v = lm_damp(d, i); put(&v, 1); }
        else if (c == "jlp") { double Jl[6], r[2], v[9]; nums(Jl, 6); nums(r, 2); jl_products(Jl, r, v); put(v, 9); }
        else if (c == "psolve") {
            const double inv_delta = num(); const int nobs = (int)num();
            double V[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Vi[6];
            for (int t = 0; t < nobs; t++) {
                double Jl[6], r[2], v[9];
                nums(Jl, 6); nums(r, 2); jl_products(Jl, r, v);
                for (int k = 0; k < 9; k++) V[k] += v[k];
            }
            point_solve(V, inv_delta, Vi);
            double o[15];
            for (int k = 0; k < 9; k++) o[k] = V[k];
            for (int k = 0; k < 6; k++) o[9 + k] = Vi[k];
            put(o, 15);
        }
        else if (c == "wrow") { double Jp[12], Jl[6], w[18]; nums(Jp, 12); nums(Jl, 6); for (int a = 0; a < 6; a++) w_row(Jp, Jl, a, w + 3 * a); put(w, 18); }
        else if (c == "sym3") { double Vi[6], b[3], o[3]; nums(Vi, 6); nums(b, 3); sym3_mul(Vi, b, o[0], o[1], o[2]); put(o, 3); }
        else if (c == "jpdot") { double jp[12], dp[6], o[2]; nums(jp, 12); nums(dp, 6); nums(o, 2); jp_dot(jp, dp, o[0], o[1]); put(o, 2); }
        else if (c == "outl") { double z = num(), r[2]; nums(r, 2); const double de = num(), re = num(); const double v = obs_is_outlier(z, r, de, re) ? 1.0 : 0.0; put(&v, 1); }
        else if (c == "lm_set") {
            double v[17]; nums(v, 17);
            LMState &s = g_lm;
            s.delta = v[0]; s.decrease_factor = v[1]; s.ssr = v[2]; s.trial_ssr = v[3]; s.pred_ssr = v[4]; s.maxdx = v[5]; s.ssr_init = v[6]; s.ssr_pass1 = v[7]; s.ssr_final = v[8];
            s.converged = (int)v[9]; s.accept = (int)v[10]; s.iters = (int)v[11]; s.n_outliers = (int)v[12]; s.chol_fail = (int)v[13]; s.iters_pass1 = (int)v[14]; s.iters_pass2 = (int)v[15]; s.cur = (int)v[16];
            put_lm();
        }
        else if (c == "lm_first") { lm_first_pass(&g_lm, num() != 0.0); put_lm(); }
        else if (c == "lm_reset") { lm_trust_reset(&g_lm); put_lm(); }
        else if (c == "lm_decide") { const double t = num(), p = num(), mx = num(); lm_decide(&g_lm, t, p, mx); put_lm(); }
        else if (c == "lm_record") { lm_record_pass(&g_lm, (int)num()); put_lm(); }
        else { std::printf("unknown command %s\n", c.c_str()); return 2; }
    }
    return 0;
}
