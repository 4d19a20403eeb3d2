// kfmap_rows_check -- the row-set routines of csrc/kfmap_ring.hpp (kfm_rows_*) as a stand-alone host program: tests/test_kfmap_rows_ring_host.py feeds it
// scripts and holds the output to the numpy model (tests/np_kfmap_rows.py).  One script per input line:
//   D  op ...      D: slots per point; two row sets, A (the surviving point) and B (prev), both empty at the start
//   p k w / P k w  kfm_rows_put of key-frame k with the row (w, w + 1, w + 2, w + 3) into A / B
//   d k / D k      kfm_rows_drop of key-frame k from A / B
//   c              kfm_rows_clear of A
//   u              kfm_rows_union of B into A, then kfm_rows_clear of B
// Output line: rows dropped by the bound, kfm_rows_count of A, then A's rows ascending by key (kfm_rows_next) as "k w" pairs; a row whose four words
// are not w .. w + 3 is printed as w = -1.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <iostream>
#include "kfmap_ring.hpp"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int D = 0;
        in >> D;
        if (D < 1 || D > KFM_MAX_ROWS) { std::printf("bad D\n"); return 1; }
        // exactly D slots each, on the heap: a routine that steps past slot D - 1 is the sanitizer's
        int32_t *ka = (int32_t *)std::calloc(D, sizeof(int32_t)), *kb = (int32_t *)std::calloc(D, sizeof(int32_t));
        uint64_t *ra = (uint64_t *)std::calloc(4 * (size_t)D, sizeof(uint64_t)), *rb = (uint64_t *)std::calloc(4 * (size_t)D, sizeof(uint64_t));
        long long dropped = 0;
        std::string op;
        while (in >> op) {
            if (op == "p" || op == "P") {
                long long k, w;
                in >> k >> w;
                const uint64_t r[4] = {(uint64_t)w, (uint64_t)w + 1, (uint64_t)w + 2, (uint64_t)w + 3};
                dropped += kfm_rows_put(op == "p" ? ka : kb, op == "p" ? ra : rb, D, (int32_t)k + 1, r);
            } else if (op == "d" || op == "D") {
                long long k;
                in >> k;
                (void)kfm_rows_drop(op == "d" ? ka : kb, D, (int32_t)k + 1);
            } else if (op == "c") kfm_rows_clear(ka, D);
            else if (op == "u") { dropped += kfm_rows_union(ka, ra, kb, rb, D); kfm_rows_clear(kb, D); }
            else { std::printf("bad op\n"); return 1; }
        }
        std::printf("%lld %d", dropped, kfm_rows_count(ka, D));
        for (int j = kfm_rows_next(ka, D, 0); j >= 0; j = kfm_rows_next(ka, D, ka[j])) {
            const uint64_t w = ra[4 * j];
            const bool whole = ra[4 * j + 1] == w + 1 && ra[4 * j + 2] == w + 2 && ra[4 * j + 3] == w + 3 && kfm_rows_find(ka, D, ka[j]) == j;
            std::printf(" %d %lld", ka[j] - 1, whole ? (long long)w : -1ll);
        }
        std::printf("\n");
        std::free(ka); std::free(kb); std::free(ra); std::free(rb);
    }
    return 0;
}
