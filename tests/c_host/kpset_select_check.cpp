// kpset_select_check.cpp -- the selection plan of slam_kpset_select (csrc/kpset_select.hpp: mask -> ascending index table, normalised mask, launch
// sizes) as a stand-alone host program: every S in {1, 3, 64, 65, 128} with a null, an empty, a full, every single-stream and both alternating
// masks, non-zero bytes other than 1 included; the table is checked against a restatement written the other way round (membership per stream).
// The arrays are exactly S long and heap-allocated, so a write past them is a sanitizer report when built with -fsanitize=address,undefined.
#include "kpset_select.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void one(int S, const std::vector<uint8_t> *mask, const char *what)
{
    cases++;
    std::vector<int32_t> idx((size_t)S, 12345);
    std::vector<uint8_t> norm((size_t)S, 77);
    const int n = kpset_select_plan(S, mask ? mask->data() : nullptr, idx.data(), norm.data());
    int want = 0;
    for (int s = 0; s < S; s++) want += !mask || (*mask)[s] != 0;
    CHECK(n == (want == S ? KPSEL_ALL : want), "S %d %s: n_sel %d, %d streams selected", S, what, n, want);
    for (int s = 0; s < S; s++) CHECK(norm[s] == (uint8_t)(!mask || (*mask)[s] != 0), "S %d %s: norm[%d] = %d", S, what, s, norm[s]);
    // every selected stream occurs exactly once, ascending; the tail is -1
    std::vector<int> seen((size_t)S, 0);
    for (int i = 0; i < want; i++) {
        CHECK(idx[i] >= 0 && idx[i] < S, "S %d %s: idx[%d] = %d", S, what, i, idx[i]);
        if (idx[i] >= 0 && idx[i] < S) seen[idx[i]]++;
        if (i > 0) CHECK(idx[i] > idx[i - 1], "S %d %s: idx not ascending at %d", S, what, i);
    }
    for (int i = want; i < S; i++) CHECK(idx[i] == -1, "S %d %s: tail idx[%d] = %d", S, what, i, idx[i]);
    for (int s = 0; s < S; s++) CHECK(seen[s] == (int)norm[s], "S %d %s: stream %d occurs %d times", S, what, s, seen[s]);
    // launch sizes
    const int streams = kpset_select_streams(S, n);
    CHECK(streams == want, "S %d %s: %d stream slots for %d selected", S, what, streams, want);
    const int cap = 1173;
    CHECK(kpset_select_bound(S, cap, n, 0) == want * cap, "S %d %s: bound without a hint", S, what);
    CHECK(kpset_select_bound(S, cap, n, 5) == (want > 0 ? 5 : 0), "S %d %s: bound with a small hint", S, what);
    CHECK(kpset_select_bound(S, cap, n, 1 << 30) == want * cap, "S %d %s: bound with a large hint", S, what);
}

int main()
{
    const int sizes[] = {1, 3, 64, 65, 128};
    for (int S : sizes) {
        one(S, nullptr, "null");
        std::vector<uint8_t> m((size_t)S, 0);
        one(S, &m, "empty");
        for (int s = 0; s < S; s++) { m[s] = (uint8_t)(1 + 37 * s); if (m[s] == 0) m[s] = 255; }    // any non-zero byte selects (1 + 37 s wraps to 0 at s = 83)
        one(S, &m, "full");
        for (int s = 0; s < S; s++) { std::vector<uint8_t> q((size_t)S, 0); q[s] = s % 2 ? 1 : 200; one(S, &q, "single"); }
        for (int par = 0; par < 2; par++) { std::vector<uint8_t> q((size_t)S, 0); for (int s = par; s < S; s += 2) q[s] = 1; one(S, &q, par ? "odd" : "even"); }
        { std::vector<uint8_t> q((size_t)S, 1); q[S - 1] = 0; if (S > 1) one(S, &q, "all but the last"); }
    }
    // refusals: nothing written
    int32_t i1[1] = {9}; uint8_t n1[1] = {9}, m1[1] = {1};
    CHECK(kpset_select_plan(0, m1, i1, n1) == KPSEL_ALL && i1[0] == 9 && n1[0] == 9, "S = 0");
    CHECK(kpset_select_plan(1, m1, nullptr, n1) == KPSEL_ALL && n1[0] == 9, "null idx");
    CHECK(kpset_select_plan(1, m1, i1, nullptr) == KPSEL_ALL && i1[0] == 9, "null norm");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("%d cases\nkpset_select OK\n", cases);
    return 0;
}
