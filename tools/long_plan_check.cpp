// dev / test: the cutting rule for recordings of any length (csrc/qv_long_plan.h) -- host only, no GPU.
//
//     c++ -std=c++17 -fsanitize=address,undefined tools/long_plan_check.cpp -o long_plan_check
//     ./long_plan_check frames     n / 1280 + 1 against the forward's own frame arithmetic for n = 0 .. 200,000
//     ./long_plan_check grid       the plan's invariants over a grid of (n, Kw, M), and every plan printed for comparison
//                                  with a restatement of the rule
//     ./long_plan_check refused    the bad-argument cases
//
// Exit status 0 when every check holds; tests/test_long_plan_host.py builds and runs it.
#include "../offline-tarteel_amd/csrc/qv_long_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {

// qv_frames_for_samples (qv_capi.hip): STFT with center = True and hop 160, then three convolutions k3 s2 p1
int32_t forward_frames(int64_t n) {
    int64_t t = n / 160 + 1;
    for (int i = 0; i < 3; ++i) t = (t + 2 - 3) / 2 + 1;
    return (int32_t)t;
}

int frames() {
    for (int64_t n = 0; n <= 200000; ++n) CHECK(qv_long_frames(n) == forward_frames(n));
    printf("frames hold\n");
    return 0;
}

int grid() {
    const int kws[] = {1, 2, 3, 5, 37, 125, 762};
    long plans = 0;
    for (int kw : kws) {
        const int window = kw * QV_LONG_HOP;
        std::vector<int> ms = {-1, 0, 1, (kw - 1) / 2, kw / 4, 6, 18, 50};
        for (int m : ms) {
            if (m > (kw - 1) / 2) continue;
            std::vector<int64_t> ns = {0, 1, 399, 400, 1279, 1280, 1281, window - 1, window, window + 1, window + 399, window + 400,
                                       window + 1279, window + 1280, window + 1281, 2LL * window, 2LL * window + 1, 3LL * window - 1,
                                       7LL * window + 640, 130000, 211000, 1000003, (int64_t)QV_LONG_HOP * QV_LONG_FRAME_CAP - 1};
            if (m >= 0)
                for (int k = 1; k <= 4; ++k)   // on, just before and just behind the lengths at which one more window is needed
                    for (int d = -1; d <= 1; ++d) ns.push_back((int64_t)QV_LONG_HOP * (k * (kw - 2 * m) + kw) + d);
            for (int64_t n : ns) {
                if (n < 0) continue;
                // max_samples between the window and the next multiple: window_samples = 0 must find the same window
                for (int pass = 0; pass < 2; ++pass) {
                    QvLongPlan p;
                    CHECK(qv_long_plan_make(n, window + (pass ? 1279 : 0), pass ? 0 : window, m, &p) == QV_LONG_OK);
                    const int M = p.m, H = p.h;
                    CHECK(p.kw == kw && H == kw - 2 * M && H >= 1 && M >= 0 && p.t_total == n / QV_LONG_HOP + 1 && p.n_windows >= 1);
                    if (m >= 0) CHECK(M == m);
                    else CHECK(M == (kw / 4 < 50 ? kw / 4 : 50));
                    if (n <= window) CHECK(p.n_windows == 1);
                    else {   // the smallest nw whose windows reach the end
                        CHECK(p.n_windows >= 2);
                        CHECK((int64_t)QV_LONG_HOP * ((int64_t)(p.n_windows - 1) * H + kw) >= n);
                        CHECK((int64_t)QV_LONG_HOP * ((int64_t)(p.n_windows - 2) * H + kw) < n);
                    }
                    int32_t expect_lo = 0;
                    for (int w = 0; w < p.n_windows; ++w) {
                        const int32_t lo = qv_long_lo(p, w), hi = qv_long_hi(p, w), len = qv_long_len(p, w), fr = qv_long_window_frames(p, w);
                        CHECK(lo == expect_lo && hi > lo);                         // the ranges tile [0, T) ...
                        expect_lo = hi;
                        CHECK(qv_long_start(p, w) % QV_LONG_HOP == 0 && qv_long_start(p, w) + len <= n && len >= 0 && len <= window);
                        CHECK(w == p.n_windows - 1 ? qv_long_start(p, w) + len == n : len == window);
                        CHECK(lo - w * H >= 0 && hi - w * H <= fr);                // ... and every owned frame is a valid frame of its window
                        CHECK(qv_long_fwd_len(p, w) >= len && qv_long_frames(qv_long_fwd_len(p, w)) == fr && qv_long_fwd_len(p, w) <= window);
                        if (w > 0 || n >= QV_LONG_MIN_SAMPLES) CHECK(qv_long_fwd_len(p, w) >= QV_LONG_MIN_SAMPLES);
                        if (w == p.n_windows - 1) {
                            CHECK(fr + w * H == p.t_total);                        // last-window frames + start offset = T
                            if (w > 0) CHECK(len > 2 * M * QV_LONG_HOP && hi - lo >= M + 1);
                        }
                    }
                    CHECK(expect_lo == p.t_total);
                    if (!pass) printf("plan %lld %d %d: %d %d %d %d\n", (long long)n, window, m, p.n_windows, p.t_total, p.kw, p.m);
                    ++plans;
                }
            }
        }
    }
    printf("grid holds %ld\n", plans);
    return 0;
}

int refused() {
    QvLongPlan p;
    const int W = 37 * QV_LONG_HOP;
    CHECK(qv_long_plan_make(100000, 48000, W, 6, &p) == QV_LONG_OK);
    CHECK(qv_long_plan_make(-1, 48000, W, 6, &p) == QV_LONG_BAD_ARG);                  // negative length
    CHECK(qv_long_plan_make(100000, 48000, W + 1, 6, &p) == QV_LONG_BAD_ARG);          // not a multiple of 1280
    CHECK(qv_long_plan_make(100000, 48000, 1000, 6, &p) == QV_LONG_BAD_ARG);
    CHECK(qv_long_plan_make(100000, 48000, W + QV_LONG_HOP, 6, &p) == QV_LONG_BAD_ARG);   // above max_samples
    CHECK(qv_long_plan_make(100000, 48000, -QV_LONG_HOP, 6, &p) == QV_LONG_BAD_ARG);
    CHECK(qv_long_plan_make(100000, 1279, 0, 0, &p) == QV_LONG_BAD_ARG);               // no room for one frame
    CHECK(qv_long_plan_make(100000, 48000, W, 18, &p) == QV_LONG_OK && p.h == 1);      // H = 1 is the last that is accepted
    CHECK(qv_long_plan_make(100000, 48000, W, 19, &p) == QV_LONG_BAD_ARG);             // H < 1
    CHECK(qv_long_plan_make(100000, 48000, 2 * QV_LONG_HOP, 1, &p) == QV_LONG_BAD_ARG);   // H = 0
    CHECK(qv_long_plan_make(100000, 48000, W, -2, &p) == QV_LONG_BAD_ARG);
    CHECK(qv_long_plan_make(100000, 48000, W, 0x7fffffff, &p) == QV_LONG_BAD_ARG);     // (no overflow in 2 M)
    const int64_t top = (int64_t)QV_LONG_HOP * QV_LONG_FRAME_CAP;
    CHECK(qv_long_plan_make(top - 1, 48000, W, 6, &p) == QV_LONG_OK && p.t_total == QV_LONG_FRAME_CAP);
    CHECK(qv_long_plan_make(top, 48000, W, 6, &p) == QV_LONG_TOO_LONG);
    CHECK(qv_long_plan_make(INT64_MAX, 48000, W, 6, &p) == QV_LONG_TOO_LONG);
    CHECK(qv_long_plan_make(top, 48000, W, 19, &p) == QV_LONG_BAD_ARG);                // a bad margin is reported before the length
    printf("refusals hold\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "frames")) return frames();
    if (argc == 2 && !strcmp(argv[1], "grid")) return grid();
    if (argc == 2 && !strcmp(argv[1], "refused")) return refused();
    fprintf(stderr, "usage: long_plan_check frames|grid|refused\n");
    return 2;
}
