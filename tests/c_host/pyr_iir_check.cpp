// Stand-alone host replay of the pyramid filters' shared arithmetic (slam.jl_amd/csrc/pyr_iir.hpp), bit for bit.  Built and run by
// tests/test_pyr_iir_host.py (plain, and with -fsanitize=address,undefined), which compares every printed double with the oracle.
//
// Commands on stdin, numbers as hex floats, one result line each:
//   iir <a1 a2 a3 scale M0..M8 inv1masum inv1mbsum> <fill0> <H> <W> <H*W samples, column-major>
//        IIRGaussian of the image, dim 1 then dim 2, every line filtered with the shared routines -- once plainly (iir_head, iir3<false>
//        steps, iir_tail, the backward steps, * scale: what iir_line does) and once through the checkpointed split (RowCk: pass A over
//        the inputs with checkpoints in a host array, pass B block by block from them).  Prints the 2 * H * W results.
//   rz <may_enlarge> <Hs> <Ws> <Hd> <Wd> <Hs*Ws samples, column-major>
//        imresize! with resize_coord on both axes (k_resize's interpolation; may_enlarge = 0: the form the fused kernels use, sizes
//        that shrink only).  Prints the Hd * Wd results.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

// common.hpp's IIRCoef (that header needs the HIP runtime; the members are the contract of pyr_iir.hpp)
struct IIRCoef {
    double a1, a2, a3, scale, M[9], inv1masum, inv1mbsum;
};
#include "pyr_iir.hpp"

static double num() { std::string t; if (!(std::cin >> t)) { std::printf("input ended early\n"); std::exit(2); } return std::strtod(t.c_str(), nullptr); }

// one line, in place, the way iir_line walks it
static void line_plain(double *v, int n, long s, const IIRCoef &k, bool fill0)
{
    const double iminus = fill0 ? 0.0 : v[0], iplus = fill0 ? 0.0 : v[(long)(n - 1) * s];
    const IirHead h = iir_head<false>(k, v[0], v[s], v[2 * s], iminus);
    v[0] = h.o0; v[s] = h.o1; v[2 * s] = h.o2;
    double w3 = h.o0, w2 = h.o1, w1 = h.o2;
    for (int i = 3; i < n; i++) { const double t = iir3<false>(v[i * s], k.a1, w1, k.a2, w2, k.a3, w3); w3 = w2; w2 = w1; w1 = t; v[i * s] = t; }
    const IirTail tl = iir_tail<false>(k, w1, w2, w3, iplus);
    double v1 = tl.vC, v2 = tl.vB, v3 = tl.vA;
    v[(long)(n - 1) * s] = tl.vA * k.scale; v[(long)(n - 2) * s] = tl.vB * k.scale; v[(long)(n - 3) * s] = tl.vC * k.scale;
    for (int i = n - 4; i >= 0; i--) { const double t = iir3<false>(v[i * s], k.a1, v1, k.a2, v2, k.a3, v3); v3 = v2; v2 = v1; v1 = t; v[i * s] = t * k.scale; }
}

// RowCk's accessor over host arrays: the checkpoints of line `lineid` of `nlines` (the other lines' slots must stay untouched)
struct HostLine {
    const double *p; long s; double *ck; size_t nlines, lineid;
    double x(int c0, int e) const { return p[(long)(c0 + e) * s]; }
    double x_nt(int c0, int e) const { return x(c0, e); }
    double *ckp(int j) const { return ck + ((size_t)j * 3) * nlines + lineid; }
};

// the same line through pass A (inputs only, checkpoints) and pass B (blocks right to left, recomputed from the checkpoints)
static void line_split(const double *in, double *out, int n, long s, const IIRCoef &k, bool fill0)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const RowCk rc = rowck_plan(n);
    const size_t nlines = 3, lineid = 1;
    std::vector<double> ck((size_t)(rc.nb > 0 ? rc.nb : 1) * 3 * nlines, nan);
    const HostLine io = {in, s, ck.data(), nlines, lineid};
    const double iminus = fill0 ? 0.0 : in[0], iplus = fill0 ? 0.0 : in[(long)(n - 1) * s];
    const IirHead h = iir_head<false>(k, in[0], in[s], in[2 * s], iminus);
    double w3 = h.o0, w2 = h.o1, w1 = h.o2;
    double cur[CK_B], nxt[CK_B];
    rowck_pass_a(io, rc, k.a1, k.a2, k.a3, cur, nxt, w1, w2, w3);
    for (int e = 0; e < rc.rem; e++) { const double t = iir3<false>(cur[e], k.a1, w1, k.a2, w2, k.a3, w3); w3 = w2; w2 = w1; w1 = t; }   // the remainder, as in the kernels
    const IirTail tl = iir_tail<false>(k, w1, w2, w3, iplus);
    double v1 = tl.vC, v2 = tl.vB, v3 = tl.vA;
    std::vector<double> res((size_t)n, nan);
    res[n - 1] = tl.vA * k.scale; res[n - 2] = tl.vB * k.scale; res[n - 3] = tl.vC * k.scale;
    for (int j = rc.nb - 1; j >= 0; j--) {                        // block j covers i in [3 + j CK_B, 3 + min((j+1) CK_B, m))
        const int len = rc.m - j * CK_B < CK_B ? rc.m - j * CK_B : CK_B;
        if (!(j == rc.nb - 1 && rc.have_last)) rowck_load_x(io, rc, j, cur);      // (have_last: pass A left the block's inputs in `cur`)
        double f1, f2, f3;
        rowck_load(io, j, h, f1, f2, f3);
        if (len == CK_B) { iir_block_fwd<CK_B, true>(cur, k.a1, k.a2, k.a3, f1, f2, f3); iir_block_bwd<CK_B>(cur, k.a1, k.a2, k.a3, k.scale, v1, v2, v3); }
        else {                                                    // the partial rightmost block, a predicated step per sample as in the kernels
            for (int e = 0; e < len; e++) { const double t = iir3<false>(cur[e], k.a1, f1, k.a2, f2, k.a3, f3); f3 = f2; f2 = f1; f1 = t; cur[e] = t; }
            for (int e = len - 1; e >= 0; e--) { const double t = iir3<false>(cur[e], k.a1, v1, k.a2, v2, k.a3, v3); v3 = v2; v2 = v1; v1 = t; cur[e] = t * k.scale; }
        }
        for (int e = 0; e < len; e++) res[3 + j * CK_B + e] = cur[e];
    }
    const double o[3] = {h.o0, h.o1, h.o2};
    for (int i = n - 4 < 2 ? n - 4 : 2; i >= 0; i--) { const double t = iir3<false>(o[i], k.a1, v1, k.a2, v2, k.a3, v3); v3 = v2; v2 = v1; v1 = t; res[i] = t * k.scale; }
    for (size_t q = 0; q < ck.size(); q++)                        // only this line's slots of blocks 1 .. nb-1 were written
        if ((ck[q] == ck[q]) != (q % nlines == lineid && q / (3 * nlines) >= 1)) { std::printf("checkpoint slot %zu of n = %d\n", q, n); std::exit(3); }
    for (int i = 0; i < n; i++) out[(long)i * s] = res[i];
}

static void cmd_iir()
{
    IIRCoef k;
    k.a1 = num(); k.a2 = num(); k.a3 = num(); k.scale = num();
    for (int i = 0; i < 9; i++) k.M[i] = num();
    k.inv1masum = num(); k.inv1mbsum = num();
    const bool fill0 = num() != 0.0;
    const int H = (int)num(), W = (int)num();
    std::vector<double> a((size_t)H * W), b((size_t)H * W), t((size_t)H * W);
    for (double &v : a) v = num();
    t = a;
    for (int x = 0; x < W; x++) line_plain(a.data() + (size_t)x * H, H, 1, k, fill0);
    for (int y = 0; y < H; y++) line_plain(a.data() + y, W, H, k, fill0);
    for (int x = 0; x < W; x++) line_split(t.data() + (size_t)x * H, b.data() + (size_t)x * H, H, 1, k, fill0);
    t = b;
    for (int y = 0; y < H; y++) line_split(t.data() + y, b.data() + y, W, H, k, fill0);
    for (double v : a) std::printf("%a ", v);
    for (double v : b) std::printf("%a ", v);
    std::printf("\n");
}

static void cmd_rz()
{
    const bool may_enlarge = num() != 0.0;
    const int Hs = (int)num(), Ws = (int)num(), Hd = (int)num(), Wd = (int)num();
    std::vector<double> src((size_t)Hs * Ws);
    for (double &v : src) v = num();
    const ResizeAxis ay = resize_axis(Hs, Hd, may_enlarge), ax = resize_axis(Ws, Wd, may_enlarge);
    for (int x = 1; x <= Wd; x++)
        for (int y = 1; y <= Hd; y++) {
            const ResizeCoord ry = resize_coord(ay, y), rx = resize_coord(ax, x);
            const double *p = src.data() + (size_t)(ry.i - 1) + (size_t)(rx.i - 1) * Hs;
            const int dy = Hs > 1 ? 1 : 0; const size_t dx = Ws > 1 ? (size_t)Hs : 0;
            const double r0 = (1 - rx.f) * p[0] + rx.f * p[dx];
            const double r1 = (1 - rx.f) * p[dy] + rx.f * p[dy + dx];
            std::printf("%a ", (1 - ry.f) * r0 + ry.f * r1);
        }
    std::printf("\n");
}

int main()
{
    std::string c;
    while (std::cin >> c) {
        if (c == "iir") cmd_iir();
        else if (c == "rz") cmd_rz();
        else { std::printf("unknown command %s\n", c.c_str()); return 2; }
    }
    return 0;
}
