// Stand-alone host check of where the work records live (slam.jl_amd/csrc/work_order.hpp: work_rec_stride, work_rec_per, work_rec_slot,
// work_rec_entry): every entry of a list gets a slot of its own inside the 8 x stride records, and the walk of k_kpset_match -- workgroup b
// starts at row b % 8, column b / 8 and advances by gridDim.x / 8 columns per round, valid while work_rec_entry says so -- visits exactly the
// list's entries, once each, XCD x the entries [x per, min((x + 1) per, ntot)) in order.  Built and run by tests/test_work_rec_host.py (plain,
// and with -fsanitize=address,undefined).
#include <cstdio>
#include <vector>
#include <initializer_list>
#include "work_order.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d: %s (S %d cap %d ntot %d grid %d)\n", __LINE__, #c, g_S, g_cap, g_ntot, g_grid); fails++; } } while (0)
static int g_S, g_cap, g_ntot, g_grid;

static void check_list(int S, int cap, int ntot)
{
    g_S = S; g_cap = cap; g_ntot = ntot; g_grid = 0;
    const long long slots = (long long)S * cap;
    const int stride = work_rec_stride(slots), per = work_rec_per(ntot);
    CHECK((long long)stride * WORK_XCDS >= slots && (long long)(stride - 1) * WORK_XCDS < slots);
    CHECK(per <= stride && (long long)per * WORK_XCDS >= ntot && (ntot == 0 ? per == 0 : (per - 1) * WORK_XCDS < ntot));
    // every entry a slot of its own, inside the region; the inverse finds it
    std::vector<int> owner((size_t)WORK_XCDS * stride, -1);
    for (int idx = 0; idx < ntot; idx++) {
        const int at = work_rec_slot(idx, per, stride);
        CHECK(at >= 0 && at < WORK_XCDS * stride);
        if (at < 0 || at >= WORK_XCDS * stride) continue;
        CHECK(owner[at] == -1);
        owner[at] = idx;
        CHECK(work_rec_entry(at / stride, at % stride, per, ntot) == idx);
    }
    // what every slot holds by the kernel's rule: row x, column r -> entry x per + r of XCD x's eighth, nothing elsewhere
    for (int x = 0; x < WORK_XCDS; x++)
        for (int r = 0; r < stride; r++) {
            const int lo = x * per, hi = (x + 1) * per < ntot ? (x + 1) * per : ntot;
            const int want = lo + r < hi ? lo + r : -1;
            CHECK(work_rec_entry(x, r, per, ntot) == want && owner[(size_t)x * stride + r] == want);
        }
    // the kernel's walk at launch sizes smaller than, equal to and larger than the list (multiples of 8 up to the set's capacity, as lk_grid makes them)
    const int g_eq = ((ntot + WORK_XCDS - 1) / WORK_XCDS) * WORK_XCDS, g_max = stride * WORK_XCDS;
    for (int grid : {WORK_XCDS, 2 * WORK_XCDS, g_eq - WORK_XCDS, g_eq, g_eq + WORK_XCDS, g_max}) {
        if (grid < WORK_XCDS || grid > g_max) continue;
        g_grid = grid;
        std::vector<int> seen((size_t)(ntot > 0 ? ntot : 1), 0), last(WORK_XCDS, -1);
        int visits = 0;
        const int step = grid / WORK_XCDS;
        // (rounds outermost: the order in time of one XCD's waves, as far as the launch fixes one)
        for (int round = 0; round * step < stride + step; round++)
            for (int b = 0; b < grid; b++) {
                const int x = b % WORK_XCDS, r0 = b / WORK_XCDS, r = r0 + round * step;
                if (round == 0) CHECK(x * stride + r0 < WORK_XCDS * stride);         // the first fetch is issued before ntot is known: inside the region whatever it is
                if (r >= per) continue;                                              // the kernel's loop condition
                const int e = work_rec_entry(x, r, per, ntot);
                if (e < 0) continue;                                                 // its break (every later round of this wave is invalid too)
                CHECK(work_rec_entry(x, r + step, per, ntot) < 0 || work_rec_entry(x, r + step, per, ntot) == e + step);
                CHECK(work_rec_slot(e, per, stride) == x * stride + r);
                CHECK(e >= 0 && e < ntot);
                if (e >= 0 && e < ntot) seen[e]++;
                CHECK(e > last[x]);                                                   // an XCD walks its eighth in order
                last[x] = e;
                visits++;
            }
        CHECK(visits == ntot);
        for (int idx = 0; idx < ntot; idx++) CHECK(seen[idx] == 1);
    }
}

int main()
{
    // S x cap; caps that are no multiple of 8 (and sets smaller than 8 slots) among them
    const int sets[][2] = {{1, 1}, {1, 7}, {1, 48}, {3, 48}, {9, 48}, {5, 13}, {9, 45}, {2, 67}, {128, 1073}, {128, 1072}};
    for (const auto &sc : sets) {
        const int S = sc[0], cap = sc[1], full = S * cap;
        for (int ntot : {0, 1, 7, 8, 9, 63, 64, 65, full - 1, full})
            if (ntot >= 0 && ntot <= full) check_list(S, cap, ntot);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("work_rec OK\n");
    return 0;
}
