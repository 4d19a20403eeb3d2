// kf_decide_check -- the key-frame decision (csrc/kf_host.hpp: check_new_kf_required, front_end.jl:361-393) as a stand-alone host program:
// replays a table that tests/test_kf_decision_host.py exports from its numpy model, one case per line
//     cells nb_3d frames_delta local_ba_on prev_kf_nb_3d median has_prev_kf max_nb_keypoints initial_parallax required rule
// (median as a C99 hex float or "nan"), stream by stream and again as batches of up to 64 streams, and compares `required` and `rule`.
// Also: the null-argument / S < 1 refusals, a null `rule`, and the sparse-cells threshold at 1000 keypoints (0.33 * 1000 == 330.0 as doubles).
#include "kf_host.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Row { double st[KF_STATS]; int32_t fd, prev3d; uint8_t has; int ba, maxkp; double ip; int req, rule; };

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: kf_decide_check TABLE\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<Row> rows;
    char med[64];
    for (;;) {
        Row r; memset(&r, 0, sizeof r);
        double cells, nb3d; int has;
        const int k = fscanf(f, "%lf %lf %d %d %d %63s %d %d %lf %d %d", &cells, &nb3d, &r.fd, &r.ba, &r.prev3d, med, &has, &r.maxkp, &r.ip, &r.req, &r.rule);
        if (k == EOF) break;
        if (k != 11) { fprintf(stderr, "line %zu: %d fields\n", rows.size() + 1, k); return 2; }
        r.st[KF_CELLS] = cells; r.st[KF_N3D] = nb3d; r.st[KF_MEDIAN] = strcmp(med, "nan") == 0 ? NAN : strtod(med, nullptr); r.has = (uint8_t)has;
        r.st[KF_N] = 1000.0; r.st[KF_NPAR] = 900.0; r.st[KF_MEAN] = r.st[KF_MEDIAN];
        rows.push_back(r);
    }
    fclose(f);
    size_t bad = 0;
    for (size_t i = 0; i < rows.size(); i++) {                   // stream by stream
        const Row &r = rows[i];
        uint8_t req = 9, rule = 9;
        if (!kf_required(1, r.st, &r.fd, &r.prev3d, &r.has, r.maxkp, r.ip, r.ba, &req, &rule) || req != r.req || rule != r.rule) {
            if (bad++ < 10) fprintf(stderr, "row %zu: required %d rule %d, the table says %d %d\n", i, req, rule, r.req, r.rule);
        }
    }
    for (size_t i0 = 0; i0 < rows.size();) {                     // runs of rows with the same scalars, as one call of up to 64 streams
        size_t i1 = i0;
        while (i1 < rows.size() && i1 - i0 < 64 && rows[i1].ba == rows[i0].ba && rows[i1].maxkp == rows[i0].maxkp && rows[i1].ip == rows[i0].ip) i1++;
        const int S = (int)(i1 - i0);
        std::vector<double> st((size_t)S * KF_STATS); std::vector<int32_t> fd(S), p3(S); std::vector<uint8_t> has(S), req(S, 9), rule(S, 9), req2(S, 9);
        for (int s = 0; s < S; s++) { memcpy(&st[(size_t)s * KF_STATS], rows[i0 + s].st, sizeof rows[0].st); fd[s] = rows[i0 + s].fd; p3[s] = rows[i0 + s].prev3d; has[s] = rows[i0 + s].has; }
        const bool ok = kf_required(S, st.data(), fd.data(), p3.data(), has.data(), rows[i0].maxkp, rows[i0].ip, rows[i0].ba, req.data(), rule.data())
                     && kf_required(S, st.data(), fd.data(), p3.data(), has.data(), rows[i0].maxkp, rows[i0].ip, rows[i0].ba, req2.data(), nullptr);
        for (int s = 0; s < S; s++)
            if (!ok || req[s] != rows[i0 + s].req || rule[s] != rows[i0 + s].rule || req2[s] != req[s]) {
                if (bad++ < 10) fprintf(stderr, "batch row %zu: required %d rule %d, the table says %d %d\n", i0 + s, req[s], rule[s], rows[i0 + s].req, rows[i0 + s].rule);
            }
        i0 = i1;
    }
    {   // refusals write nothing
        const double st[KF_STATS] = {0}; const int32_t z = 0; const uint8_t h = 1; uint8_t req = 7;
        if (kf_required(0, st, &z, &z, &h, 1000, 20.0, 0, &req, nullptr) || kf_required(1, nullptr, &z, &z, &h, 1000, 20.0, 0, &req, nullptr)
            || kf_required(1, st, nullptr, &z, &h, 1000, 20.0, 0, &req, nullptr) || kf_required(1, st, &z, nullptr, &h, 1000, 20.0, 0, &req, nullptr)
            || kf_required(1, st, &z, &z, nullptr, 1000, 20.0, 0, &req, nullptr) || kf_required(1, st, &z, &z, &h, 1000, 20.0, 0, nullptr, nullptr) || req != 7) {
            fprintf(stderr, "a refusal case was accepted\n"); bad++;
        }
    }
    {   // at 1000 keypoints the product 0.33 * 1000 rounds to 330.0: 329 occupied cells are "sparse", 330 are not
        double st[KF_STATS] = {0}; st[KF_CELLS] = 329.0; st[KF_N3D] = 100.0;
        const int32_t fd = 5, p3 = 100; const uint8_t h = 1; uint8_t req = 9, rule = 9, req2 = 9, rule2 = 9;
        const bool a = kf_required(1, st, &fd, &p3, &h, 1000, 20.0, 0, &req, &rule);
        st[KF_CELLS] = 330.0;
        const bool b = kf_required(1, st, &fd, &p3, &h, 1000, 20.0, 0, &req2, &rule2);
        if (!a || !b || 0.33 * 1000.0 != 330.0 || req != 1 || rule != KF_RULE_SPARSE_CELLS || req2 != 0 || rule2 != KF_RULE_PARALLAX) {
            fprintf(stderr, "329 / 330 cells at 1000 keypoints: required %d %d rule %d %d\n", req, req2, rule, rule2); bad++;
        }
    }
    if (bad) { fprintf(stderr, "%zu mismatches\n", bad); return 1; }
    printf("%zu rows\nkf_decide OK\n", rows.size());
    return 0;
}
