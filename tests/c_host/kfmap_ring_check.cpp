// kfmap_ring_check -- a stand-alone host of csrc/kfmap_ring.hpp and csrc/layout.hpp (no HIP, no library): reads one command per line from stdin,
// integers in decimal and doubles as hex floats, and prints the routines' results, one line per command.
//   entry  id mcap                       -> kfm_entry
//   search id n ids[n]                   -> kfm_lower, kfm_find
//   ring   R r0 kfid minc tag[R] cov[R]  -> nv rank[R] asc[nv] | ncl cl[ncl] mask | wconst[R] | ncand cand[ncand] valid
//                                           (kfm_rank_slots | kfm_covmap_pick | kfm_window_const per slot | kfm_filter_candidates)
//   poses  R P order[R] first[R]         -> P order[R], after kfm_assign_poses (first[] must come back reset)
//   decide n_total n_good few ratio      -> kfm_filter_removes
//   oldest covmask tag[64]               -> kfm_oldest_covisible
//   hist   nC nP nU covmask linked max_local -> replace chain size (kfm_history_rule)
//   pairs  n pairs[2 n]                  -> kfm_pairs_one_to_one, kfm_sorted_one_to_one on the sorted ids, kfm_pair_clashes per pair
//   bind   (elem count)*                 -> per region: Layout::bind's offset in a block, take's offset on a second layout, both ends; a null base
//                                           must move no pointer
// tests/test_kfmap_ring_host.py drives it, once built plain and once with -fsanitize=address,undefined.
#include "kfmap_ring.hpp"
#include "layout.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct E16 { double v[2]; };
struct E24 { double v[3]; };

template <class T> static void bind_both(Layout &bound, Layout &null, Layout &raw, size_t count, std::vector<char> &block)
{
    T *p = nullptr, *q = (T *)block.data() + 1;                     // q: any pointer; a null base must leave it
    T *const q0 = q;
    const size_t at = raw.take(count * sizeof(T));
    if (at + count * sizeof(T) > block.size()) { fprintf(stderr, "bind: the block is too small\n"); exit(2); }
    bound.bind(p, count * sizeof(T), block.data());
    null.bind(q, count * sizeof(T), nullptr);
    if (q != q0) { fprintf(stderr, "bind: a null base moved the pointer\n"); exit(2); }
    if (count) p[count - 1] = T();                                  // the last element lies inside the block (the sanitizer build watches it)
    printf("%zu %zu %zu %zu %zu ", (size_t)((char *)p - block.data()), at, bound.size(), null.size(), raw.size());
}

int main()
{
    char *line = nullptr; size_t cap = 0;
    std::vector<char> block(1 << 20);
    while (getline(&line, &cap, stdin) > 0) {
        std::vector<std::string> tok;
        for (char *p = strtok(line, " \n"); p; p = strtok(nullptr, " \n")) tok.push_back(p);
        if (tok.empty()) continue;
        const std::string &cmd = tok[0];
        std::vector<long long> a;
        for (size_t i = 1; i < tok.size(); i++) a.push_back((long long)strtoull(tok[i].c_str(), nullptr, 0));      // (two's complement: "-1" and 2^64 - 1 both parse)
        auto need = [&](size_t n) { if (a.size() != n) { fprintf(stderr, "%s: %zu arguments, not %zu\n", cmd.c_str(), a.size(), n); exit(2); } };
        if (cmd == "entry") {
            need(2);
            printf("%llu", kfm_entry((int64_t)a[0], (int)a[1]));
        } else if (cmd == "search") {
            if (a.size() < 2) need(2);
            const int n = (int)a[1];
            need(2 + (size_t)n);
            std::vector<int64_t> ids(a.begin() + 2, a.end());      // (an empty vector's data() may be null: n = 0 reads nothing)
            printf("%d %d", kfm_lower(ids.data(), n, (int64_t)a[0]), kfm_find(ids.data(), n, (int64_t)a[0]));
        } else if (cmd == "ring") {
            if (a.size() < 4) need(4);
            const int R = (int)a[0], r0 = (int)a[1], kfid = (int)a[2], minc = (int)a[3];
            need(4 + 2 * (size_t)R);
            std::vector<int> tag(R), cov(R), rank(R, -1), asc(R, -1), cand(R, -1);
            for (int b = 0; b < R; b++) { tag[b] = (int)a[4 + b]; cov[b] = (int)a[4 + R + b]; }
            const int nv = kfm_rank_slots(tag.data(), R, rank.data(), asc.data());
            printf("%d ", nv);
            for (int b = 0; b < R; b++) printf("%d ", rank[b]);
            for (int k = 0; k < nv; k++) printf("%d ", asc[k]);
            int cl[N_COVISIBLE];
            unsigned long long mask = ~0ull, valid = ~0ull;
            const int ncl = kfm_covmap_pick(tag.data(), cov.data(), R, r0, cl, mask);
            printf("| %d ", ncl);
            for (int k = 0; k < ncl; k++) printf("%d ", cl[k]);
            printf("%llu | ", mask);
            for (int b = 0; b < R; b++) printf("%d ", (int)kfm_window_const(tag[b], mask >> b & 1, cov[b], minc));
            const int nc = kfm_filter_candidates(tag.data(), cov.data(), R, r0, kfid, cand.data(), valid);
            printf("| %d ", nc);
            for (int k = 0; k < nc; k++) printf("%d ", cand[k]);
            printf("%llu", valid);
        } else if (cmd == "poses") {
            if (a.size() < 2) need(2);
            const int R = (int)a[0];
            int P = (int)a[1];
            need(2 + 2 * (size_t)R);
            std::vector<int> order(R), first(R);
            for (int b = 0; b < R; b++) { order[b] = (int)a[2 + b]; first[b] = a[2 + R + b] < 0 ? INT_MAX : (int)a[2 + R + b]; }
            kfm_assign_poses(order.data(), first.data(), R, P);
            for (int b = 0; b < R; b++) if (order[b] != (int)a[2 + b] && first[b] != INT_MAX) { fprintf(stderr, "poses: first[%d] was not reset\n", b); exit(2); }
            printf("%d ", P);
            for (int b = 0; b < R; b++) printf("%d ", order[b]);
        } else if (cmd == "decide") {
            if (tok.size() != 5) need(4);
            printf("%d", (int)kfm_filter_removes((int)a[0], (int)a[1], (int)a[2], strtod(tok[4].c_str(), nullptr)));
        } else if (cmd == "oldest") {
            need(65);
            int tag[64];
            for (int b = 0; b < 64; b++) tag[b] = (int)a[1 + b];
            printf("%d", kfm_oldest_covisible((unsigned long long)a[0], tag));
        } else if (cmd == "hist") {
            need(6);
            bool replace = false, chain = false;
            const int size = kfm_history_rule((int)a[0], (int)a[1], (int)a[2], (unsigned long long)a[3], a[4] != 0, (int)a[5], replace, chain);
            printf("%d %d %d", (int)replace, (int)chain, size);
        } else if (cmd == "pairs") {
            if (a.size() < 1) need(1);
            const int n = (int)a[0];
            need(1 + 2 * (size_t)n);
            std::vector<int64_t> pr(a.begin() + 1, a.end()), p, q, both;
            for (int t = 0; t < n; t++) { p.push_back(pr[2 * t]); q.push_back(pr[2 * t + 1]); if (pr[2 * t] != pr[2 * t + 1]) { both.push_back(pr[2 * t]); both.push_back(pr[2 * t + 1]); } }
            std::sort(p.begin(), p.end()); std::sort(q.begin(), q.end()); std::sort(both.begin(), both.end());
            printf("%d %d ", (int)kfm_pairs_one_to_one(pr.data(), n), (int)kfm_sorted_one_to_one(p.data(), q.data(), n, both.data(), (int)both.size()));
            for (int t = 0; t < n; t++) printf("%d ", (int)kfm_pair_clashes(pr.data(), n, t));
        } else if (cmd == "bind") {
            Layout bound, null, raw;
            for (size_t i = 0; i + 1 < a.size(); i += 2) {
                const int size = (int)a[i]; const size_t count = (size_t)a[i + 1];
                if (size == 1) bind_both<unsigned char>(bound, null, raw, count, block);
                else if (size == 4) bind_both<int32_t>(bound, null, raw, count, block);
                else if (size == 8) bind_both<double>(bound, null, raw, count, block);
                else if (size == 16) bind_both<E16>(bound, null, raw, count, block);
                else if (size == 24) bind_both<E24>(bound, null, raw, count, block);
                else { fprintf(stderr, "bind: element size %d\n", size); exit(2); }
            }
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); exit(2); }
        printf("\n");
    }
    free(line);
    return 0;
}
