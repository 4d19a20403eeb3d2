/* orc_5pt_check -- stand-alone host of the oracle's five-point routines (tests/test_5pt_model_host.py builds it plain and with
 * -fsanitize=address,undefined; nothing loaded into Python runs under a sanitizer).  Compiled together with oracle/orc_5pt.c and
 * oracle/orc_tri.c.
 *
 *   orc_5pt_check IN OUT
 * IN  (doubles): T, n, thr, K (9, column-major), px1 (2 n), px2 (2 n), then T tuples of q1 (10), q2 (10)
 * OUT (doubles): per tuple ne, then per hypothesis E (9), has_pose, Rt (12), the inlier count and the mask (n, as 0 / 1)      */
#include "slam_oracle.h"
#include <stdio.h>
#include <stdlib.h>

static double *read_all(const char *path, size_t *count)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    double *d = (double *)malloc((size_t)bytes + 8);
    *count = fread(d, 8, (size_t)bytes / 8, f);
    fclose(f);
    return d;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: orc_5pt_check IN OUT\n"); return 2; }
    size_t count = 0;
    double *in = read_all(argv[1], &count);
    if (!in || count < 12) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int T = (int)in[0], n = (int)in[1];
    const double thr = in[2], *K = in + 3, *px1 = in + 12, *px2 = px1 + 2 * (size_t)n, *q = px2 + 2 * (size_t)n;
    if (T < 0 || n < 0 || count != 12 + 4 * (size_t)n + 20 * (size_t)T) { fprintf(stderr, "bad input size\n"); return 2; }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    unsigned char *mask = (unsigned char *)malloc((size_t)n + 1);
    double *row = (double *)malloc(((size_t)n + 24) * 8);
    long hyps = 0;
    for (int t = 0; t < T; t++) {
        const double *q1 = q + 20 * (size_t)t, *q2 = q1 + 10;
        double Es[90];
        const int ne = orc_five_point_solve(q1, q2, Es);
        if (ne < 0 || ne > 10) { fprintf(stderr, "tuple %d: ne = %d\n", t, ne); return 1; }
        const double dne = (double)ne;
        fwrite(&dne, 8, 1, out);
        for (int e = 0; e < ne; e++) {
            double Rt[12] = {0};
            const int ok = orc_essential_pose_cheirality(Es + 9 * e, q1, q2, Rt);
            int cnt = 0;
            for (int i = 0; i < n; i++) mask[i] = 0;
            if (ok) cnt = orc_two_view_inliers(px1, px2, n, K, K, Rt, thr, mask);
            for (int j = 0; j < 9; j++) row[j] = Es[9 * e + j];
            row[9] = (double)ok;
            for (int j = 0; j < 12; j++) row[10 + j] = Rt[j];
            row[22] = (double)cnt;
            for (int i = 0; i < n; i++) row[23 + i] = (double)mask[i];
            fwrite(row, 8, 23 + (size_t)n, out);
            hyps++;
        }
    }
    fclose(out);
    free(row); free(mask); free(in);
    printf("%d tuples, %ld hypotheses: orc_5pt OK\n", T, hyps);
    return 0;
}
