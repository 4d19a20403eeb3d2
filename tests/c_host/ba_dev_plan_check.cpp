// ba_dev_plan_check.cpp -- csrc/ba_dev_plan.hpp as a stand-alone host program (tests/test_ba_dev_plan_host.py builds it plain and with
// -fsanitize=address,undefined and holds its output to tests/np_ba_dev_stage.py).  stdin: the number of windows, then per window "P M O", P constant
// flags, O pose ids, O point ids (1-based, grouped by ascending point id).  stdout, one line per window:
//   nfree cmax | p0 pspan (caller's order) | p0 pspan (relabelled) | the window rule | order[P] | label[P] | order with the free poses reversed [P] |
//   ksplit by cost | ksplit by observation counts
// pt_start / pfs are formed here by a plain walk (they are the kernel's to form, not the header's); everything else printed is the header's answer.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ba_dev_plan.hpp"

int main()
{
    int N;
    if (scanf("%d", &N) != 1) return 2;
    for (int w = 0; w < N; w++) {
        int P, M, O;
        if (scanf("%d %d %d", &P, &M, &O) != 3) return 2;
        std::vector<uint8_t> tc(P);
        std::vector<long long> pi(O), li(O);
        for (int p = 0; p < P; p++) { int v; if (scanf("%d", &v) != 1) return 2; tc[p] = (uint8_t)v; }
        for (int i = 0; i < O; i++) if (scanf("%lld", &pi[i]) != 1) return 2;
        for (int i = 0; i < O; i++) if (scanf("%lld", &li[i]) != 1) return 2;
        std::vector<int> start(M + 1, 0), pfs(M + 1, 0);
        for (int i = 0; i < O; i++) { start[li[i]]++; if (!tc[pi[i] - 1]) pfs[li[i]]++; }
        int cmax = 0;
        for (int j = 0; j < M; j++) { cmax = cmax > start[j + 1] ? cmax : start[j + 1]; start[j + 1] += start[j]; pfs[j + 1] += pfs[j]; }
        std::vector<int> order(P), rev(P), seq;
        const int nfree = ba_relabel_free_last(tc.data(), P, nullptr, 0, order.data());
        for (int p = P - 1; p >= 0; p--) if (!tc[p]) seq.push_back(p);
        if (ba_relabel_free_last(tc.data(), P, seq.data(), (int)seq.size(), rev.data()) != nfree) return 3;
        int p0u, su, p0, sp;
        ba_free_span(tc.data(), P, &p0u, &su);
        ba_free_span_relabelled(P, nfree, &p0, &sp);
        const bool rule = ba_window_eligible(true, M > 0 && O > 0, nfree, sp, P, O, cmax);
        printf("%d %d %d %d %d %d %d", nfree, cmax, p0u, su, p0, sp, rule ? 1 : 0);
        for (int k = 0; k < P; k++) printf(" %d", order[k]);
        for (int p = 0; p < P; p++) printf(" %d", ba_label_free_last(tc.data(), P, p));
        for (int k = 0; k < P; k++) printf(" %d", rev[k]);
        const int kc = M > 1 ? ba_ksplit_cost(M, O, [&](int k) { return start[k]; }, [&](int k) { return pfs[k]; }) : -1;
        // the device's way to the same number: count the points for which ba_ksplit_before holds
        int cnt = 0;
        const long long total = ba_ksplit_total(O, pfs[M]);
        for (int k = 0; k < M; k++) cnt += ba_ksplit_before(total, start[k], pfs[k]) ? 1 : 0;
        if (M > 1 && ba_ksplit_clamp(cnt, M) != kc) return 4;
        printf(" %d %d\n", kc, ba_ksplit_obs(M, O, [&](int k) { return start[k]; }));
    }
    return 0;
}
