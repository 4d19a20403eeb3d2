// Stand-alone host check of the work list's sort key (slam.jl_amd/csrc/work_order.hpp): monotone in band and row, clamped to the
// image, defined for NaN / inf / huge positions; and of the rule that picks the tracking kernels' instantiation (lk_slots, lk_window_elems:
// `work_key_check slots` prints "window slots elems" for windows 0..16).  Built and run by tests/test_work_key_host.py (plain, and with
// -fsanitize=address,undefined,float-cast-overflow: no conversion of a value an int cannot hold).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <cstring>
#include <limits>
#include "work_order.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "slots")) {
        for (int w = 0; w <= 16; w++) std::printf("%d %d %d\n", w, lk_slots(w), lk_window_elems(w));
        return 0;
    }
    const int H = 370, W = 1226;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double odd[] = {nan, -nan, inf, -inf, 1e300, -1e300, 4294967296.0, -4294967296.0, 2147483648.0, -2147483649.0, 1e19, -0.0, 0.0,
                          std::numeric_limits<double>::denorm_min(), 0.999999, 1.0, 65535.0, 65536.0, 65535.999};
    // clamping: 0 below 1, floor inside, hi from hi on; NaN -> hi
    CHECK(work_clamp_px(-5.0, H) == 0 && work_clamp_px(0.0, H) == 0 && work_clamp_px(0.99, H) == 0);
    CHECK(work_clamp_px(1.0, H) == 1 && work_clamp_px(1.99, H) == 1 && work_clamp_px(369.99, H) == 369);
    CHECK(work_clamp_px(370.0, H) == 370 && work_clamp_px(370.5, H) == 370 && work_clamp_px(1e9, H) == 370);
    CHECK(work_clamp_px((double)W, W) == (uint32_t)W && work_clamp_px(W + 0.5, W) == (uint32_t)W && work_clamp_px(W - 0.5, W) == (uint32_t)W - 1);
    CHECK(work_clamp_px(nan, H) == 370 && work_clamp_px(inf, H) == 370 && work_clamp_px(-inf, H) == 0);
    CHECK(work_clamp_px(1e300, 1 << 20) == WORK_KEY_MAX_PX && work_clamp_px(nan, 1 << 20) == WORK_KEY_MAX_PX && work_clamp_px(5.0, -3) == 0 && work_clamp_px(nan, -3) == 0);
    for (double v : odd)
        for (int hi : {0, 1, H, W, 65535, 65536, 1 << 30}) {
            const uint32_t c = work_clamp_px(v, hi);
            CHECK(c <= (uint32_t)(hi > WORK_KEY_MAX_PX ? WORK_KEY_MAX_PX : hi));
        }
    // every key of every odd position is defined and inside the image's key range
    for (int band : {1, 16, 32, 64, 5000, 0, -7})
        for (double y : odd)
            for (double x : odd) {
                const uint32_t k = work_key(y, x, H, W, band);
                CHECK((k & 0xffffu) <= (uint32_t)H && (k >> 16) <= (uint32_t)W / (uint32_t)(band < 1 ? 1 : band));
            }
    // monotone: non-decreasing in x at fixed y, in y at fixed x; the band dominates the row
    for (int band : {1, 16, 32, 64, 5000}) {
        uint32_t last = 0;
        for (double x = -3.0; x < W + 4.0; x += 0.37) { const uint32_t k = work_key(200.3, x, H, W, band); CHECK(k >= last); last = k; }
        last = 0;
        for (double y = -3.0; y < H + 4.0; y += 0.37) { const uint32_t k = work_key(y, 600.1, H, W, band); CHECK(k >= last); last = k; }
        CHECK(work_key(1.0, 2.0 * band + 1.0, H, W, band) > work_key((double)H, 2.0 * band - 0.5, H, W, band) || 2 * band >= W);
        CHECK((work_key(17.5, 100.0, H, W, band) >> 16) == 100u / (uint32_t)band && (work_key(17.5, 100.0, H, W, band) & 0xffffu) == 17u);
    }
    // same band and row -> same key (the slot index breaks the tie in the kernel)
    CHECK(work_key(50.2, 33.0, H, W, 32) == work_key(50.9, 63.9, H, W, 32) && work_key(50.2, 31.9, H, W, 32) != work_key(50.2, 32.0, H, W, 32));
    // a band wider than the image is a pure row order, a 1-px band a pure column order
    CHECK(work_key(10.0, 1200.0, H, W, 5000) < work_key(11.0, 3.0, H, W, 5000) && work_key(300.0, 7.0, H, W, 1) < work_key(2.0, 8.0, H, W, 1));
    // the instantiation rule: the smallest of 3 / 6 / 9 slots per lane whose 64 lanes hold the window; the kernel's `cached`
    // (lk_window_elems(w) <= 64 * LK_MAXE, LK_MAXE = lk_slots(w)) holds exactly up to window 11
    for (int w = 0; w <= 16; w++) {
        const int ne = lk_window_elems(w), n = lk_slots(w);
        CHECK(ne == (2 * w + 1) * (2 * w + 1) && (n == 3 || n == 6 || n == 9));
        CHECK(n == 9 || ne <= 64 * n);                               // a 3- / 6-slot kernel always holds its window
        CHECK(n == 3 || ne > 64 * (n - 3));                          // and no smaller one would
        CHECK((ne <= 64 * n) == (w <= 11));
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("work_key OK\n");
    return 0;
}
