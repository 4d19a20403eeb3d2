// compact_rank_check.cpp -- the host arithmetic of the compact right batch (csrc/kpset_select.hpp) as a stand-alone program: the rank table
// (kpset_select_rank: stream -> member of a compact batch, the inverse of kpset_select_plan's ascending table) and the stale-build check
// (kpset_select_same: the mask a batch was built for against the set's selection), at S = 1, 64, 65, 128 under the masks none, all, null, first,
// last, both alternating ones and random ones.  The rank is checked against a restatement written the other way round (the number of selected
// streams below s).  The arrays are exactly S long and heap-allocated: a write past them is a sanitizer report under -fsanitize=address,undefined.
#include "kpset_select.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0, cases = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void one(int S, const std::vector<uint8_t> *mask, const char *what)
{
    cases++;
    std::vector<int32_t> idx((size_t)S, 12345), rank((size_t)S, 54321);
    std::vector<uint8_t> norm((size_t)S, 77);
    const int n = kpset_select_plan(S, mask ? mask->data() : nullptr, idx.data(), norm.data());
    kpset_select_rank(S, idx.data(), n, rank.data());
    const int streams = kpset_select_streams(S, n);
    // the restatement: a selected stream's rank is the number of selected streams below it; an unselected stream has none
    int below = 0;
    for (int s = 0; s < S; s++) {
        const bool on = !mask || (*mask)[s] != 0;
        CHECK(rank[s] == (on ? below : -1), "S %d %s: rank[%d] = %d, want %d", S, what, s, rank[s], on ? below : -1);
        below += on;
    }
    CHECK(below == streams, "S %d %s: %d selected, %d stream slots", S, what, below, streams);
    // rank is the inverse of the ascending table, and every rank is a member of an n_sel-member batch
    for (int r = 0; r < streams; r++) CHECK(idx[r] >= 0 && idx[r] < S && rank[idx[r]] == r, "S %d %s: rank[idx[%d]] != %d", S, what, r, r);
    for (int s = 0; s < S; s++) if (rank[s] >= 0) CHECK(rank[s] < streams && idx[rank[s]] == s, "S %d %s: idx[rank[%d]] != %d", S, what, s, s);
    // the stale-build check: a mask equals itself (normalised or as given), differs from itself with any one stream flipped, and from any other S
    std::vector<uint8_t> raw((size_t)S);
    for (int s = 0; s < S; s++) raw[s] = mask ? (*mask)[s] : 1;
    CHECK(kpset_select_same(S, norm.data(), S, norm.data()), "S %d %s: a mask differs from itself", S, what);
    CHECK(kpset_select_same(S, norm.data(), S, raw.data()), "S %d %s: the normalised mask differs from the mask as given", S, what);
    for (int s = 0; s < S; s += (S > 16 ? 7 : 1)) {
        std::vector<uint8_t> other(norm);
        other[s] = other[s] ? 0 : 1;
        CHECK(!kpset_select_same(S, norm.data(), S, other.data()), "S %d %s: stream %d flipped and still the same", S, what, s);
        CHECK(!kpset_select_same(S, other.data(), S, norm.data()), "S %d %s: stream %d flipped and still the same (swapped)", S, what, s);
    }
    CHECK(!kpset_select_same(0, norm.data(), S, norm.data()), "S %d %s: a batch without a compact build passes", S, what);
    if (S > 1) CHECK(!kpset_select_same(S - 1, norm.data(), S, norm.data()), "S %d %s: a build for S - 1 streams passes", S, what);
    CHECK(!kpset_select_same(S, nullptr, S, norm.data()) && !kpset_select_same(S, norm.data(), S, nullptr), "S %d %s: a null mask passes", S, what);
}

int main()
{
    const int sizes[] = {1, 64, 65, 128};
    unsigned lcg = 12345u;
    for (int S : sizes) {
        one(S, nullptr, "null");
        std::vector<uint8_t> m((size_t)S, 0);
        one(S, &m, "none");
        for (int s = 0; s < S; s++) m[s] = (uint8_t)(s % 2 ? 1 : 255);                              // any non-zero byte selects
        one(S, &m, "all");
        { std::vector<uint8_t> q((size_t)S, 0); q[0] = 3; one(S, &q, "first"); }
        { std::vector<uint8_t> q((size_t)S, 0); q[S - 1] = 1; one(S, &q, "last"); }
        for (int par = 0; par < 2; par++) {
            std::vector<uint8_t> q((size_t)S, 0);
            for (int s = par; s < S; s += 2) q[s] = 1;
            one(S, &q, par ? "odd" : "even");
        }
        for (int k = 0; k < 8; k++) {
            std::vector<uint8_t> q((size_t)S, 0);
            for (int s = 0; s < S; s++) { lcg = lcg * 1664525u + 1013904223u; q[s] = (lcg >> 24) % 3 == 0 ? (uint8_t)(1 + (lcg >> 16) % 200) : 0; }
            one(S, &q, "random");
        }
    }
    // refusals: nothing written
    int32_t i1[1] = {0}, r1[1] = {9};
    kpset_select_rank(0, i1, 1, r1); CHECK(r1[0] == 9, "S = 0 wrote a rank");
    kpset_select_rank(1, nullptr, 1, r1); CHECK(r1[0] == 9, "a null table wrote a rank");
    kpset_select_rank(1, i1, 1, nullptr);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("%d cases\ncompact_rank OK\n", cases);
    return 0;
}
