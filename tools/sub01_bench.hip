// sub01_bench.hip -- conv.0 + ReLU + conv.2 of the f16 front end on their own: k_sub01 (fused, c0 through LDS) in its
// variants against the two-kernel path (k_conv0 + k_dwconv2d, c0 through HBM) on random log-mel features, B utterances of
// Tm mel frames each (default: 64 x 1,001, the headline batch, then 64 x 3,001, the 30 s one).  HIP-event averages over
// back-to-back launches and a byte compare of c1 for every variant:
//   refetch 8 / 16   k_sub01<false>: the mel rows of a tile are fetched, normalised and stored once per channel group
//   resident 1 .. 4  k_sub01<true>: the run's normalised mel rows stay in LDS
//   product          launch_sub01, i.e. what qv_sub01_run_tiles picks for the shape
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops \
//         -I offline-tarteel_amd/csrc -I include tools/sub01_bench.hip -o tools/sub01_bench
//   tools/sub01_bench [iters] [B] [Tm]
// Built with -DQV_SUB01_STAMPS (-o tools/sub01_bench_stamps) the kernel also records where wave 0 of one block in the
// middle of the grid spends its clock (see SUB_STAMP in qv_frontend.hip) and the tool prints each phase's share; the times
// of that build are not the product's.
#include "../offline-tarteel_amd/csrc/qv_frontend.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int run_shape(int B, int Tm, int iters) {
    const int T1 = (Tm - 1) / 2 + 1, T2 = (T1 - 1) / 2 + 1, n_tiles = (T2 + SUB_TT - 1) / SUB_TT;
    const size_t nf = (size_t)B * Tm * QV_NMEL, n0 = (size_t)B * T1 * 40 * QV_SUBC, n1 = (size_t)B * T2 * 20 * QV_SUBC;
    std::vector<float> hf(nf), hw0(9 * QV_SUBC), hb0(QV_SUBC), hw1(9 * QV_SUBC), hb1(QV_SUBC);
    srand(1);
    auto rnd = [] { return (rand() % 2001 - 1000) / 1000.0f; };
    for (auto &x : hf) x = -8.f + 6.f * rnd();              // (log-mel features: any finite values do)
    for (auto &x : hw0) x = rnd() * 0.5f;
    for (auto &x : hb0) x = rnd() * 0.1f;
    for (auto &x : hw1) x = rnd() * 0.3f;
    for (auto &x : hb1) x = rnd() * 0.1f;
    std::vector<int32_t> hn(B, (Tm - 1) * 160), hlm(B, Tm), hl1(B, T1);
    float *feats, *w0, *b0, *w1, *b1;
    half_t *c0, *c1a, *c1b;
    double *stats;
    int32_t *ns, *lm, *l1;
    CK(hipMalloc(&feats, nf * 4)); CK(hipMalloc(&c0, n0 * 2)); CK(hipMalloc(&c1a, n1 * 2)); CK(hipMalloc(&c1b, n1 * 2));
    CK(hipMalloc(&w0, 9 * QV_SUBC * 4)); CK(hipMalloc(&b0, QV_SUBC * 4)); CK(hipMalloc(&w1, 9 * QV_SUBC * 4)); CK(hipMalloc(&b1, QV_SUBC * 4));
    CK(hipMalloc(&stats, qv_melstats_doubles(B) * 8));
    CK(hipMalloc(&ns, B * 4)); CK(hipMalloc(&lm, B * 4)); CK(hipMalloc(&l1, B * 4));
    CK(hipMemcpy(feats, hf.data(), nf * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w0, hw0.data(), 9 * QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(b0, hb0.data(), QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w1, hw1.data(), 9 * QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(b1, hb1.data(), QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(ns, hn.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(lm, hlm.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(l1, hl1.data(), B * 4, hipMemcpyHostToDevice));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    // the statistics the normalisation reads, as the forward forms them
    hipLaunchKernelGGL(k_melstats, dim3(MS_CHUNKS, B), dim3(320), 0, s, feats, ns, Tm, stats + (size_t)B * 2 * QV_NMEL);
    hipLaunchKernelGGL(k_melstats_sum, dim3(B), dim3(2 * QV_NMEL), 0, s, stats + (size_t)B * 2 * QV_NMEL, stats);
    CK(hipStreamSynchronize(s));

    auto pair = [&] {
        launch_conv0(feats, Tm, lm, stats, w0, b0, c0, T1, B, s);
        launch_dwconv2d(c0, T1, 40, l1, w1, b1, c1a, T2, 20, B, s);
    };
    auto fused = [&](bool resident, int run) {
        const dim3 grid(1, (n_tiles + run - 1) / run, B);
        if (resident)
            hipLaunchKernelGGL(k_sub01<true>, grid, dim3(256), 0, s, feats, Tm, lm, stats, w0, b0, l1, w1, b1, c1b, T2, run);
        else
            hipLaunchKernelGGL(k_sub01<false>, grid, dim3(256), 0, s, feats, Tm, lm, stats, w0, b0, l1, w1, b1, c1b, T2, run);
    };
    struct Variant { const char *name; int resident, run; };     // resident < 0: launch_sub01
    const Variant variants[] = {{"pair", 0, 0}, {"refetch 8", 0, 8}, {"refetch 16", 0, 16}, {"refetch 4", 0, 4}, {"resident 1", 1, 1},
                                {"resident 2", 1, 2}, {"resident 4", 1, 4}, {"product", -1, 0}};
    std::vector<half_t> ha(n1), hb(n1);
    size_t bad_total = 0;
    printf("B %d x %d mel frames (%d c1 frames, %d tiles; the product picks a run of %d):\n", B, Tm, T2, n_tiles, qv_sub01_run_tiles(B, T2));
    for (const Variant &v : variants) {
        auto go = [&] { v.run == 0 && v.resident == 0 ? pair() : v.resident < 0 ? launch_sub01(feats, Tm, lm, stats, w0, b0, l1, w1, b1, c1b, T2, B, s) : fused(v.resident, v.run); };
        if (v.run || v.resident) CK(hipMemsetAsync(c1b, 0xff, n1 * 2, s));
        for (int i = 0; i < 5; ++i) go();
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) go();
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        CK(hipGetLastError());
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (!(v.run || v.resident)) {
            CK(hipMemcpy(ha.data(), c1a, n1 * 2, hipMemcpyDeviceToHost));
            printf("  %-11s %8.1f us (k_conv0 + k_dwconv2d)\n", v.name, ms * 1000 / iters);
            continue;
        }
        CK(hipMemcpy(hb.data(), c1b, n1 * 2, hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (size_t i = 0; i < n1; ++i) bad += memcmp(&ha[i], &hb[i], 2) != 0;
        bad_total += bad;
        printf("  %-11s %8.1f us; c1 halves that differ from the pair's: %zu of %zu", v.name, ms * 1000 / iters, bad, n1);
#ifdef QV_SUB01_STAMPS
        unsigned long long st[6];
        CK(hipMemcpyFromSymbol(st, HIP_SYMBOL(qv_sub01_stamps), sizeof(st)));
        double sum = 0;
        for (int p = 0; p < 6; ++p) sum += (double)st[p];
        printf("; wave clocks %.0f: prologue %.1f %%, conv0 %.1f %%, barrier %.1f %%, depthwise %.1f %%, mel store %.1f %%, barrier %.1f %%",
               sum, 100 * st[0] / sum, 100 * st[1] / sum, 100 * st[2] / sum, 100 * st[3] / sum, 100 * st[4] / sum, 100 * st[5] / sum);
#endif
        printf("\n");
    }
    for (void *p : {(void *)feats, (void *)c0, (void *)c1a, (void *)c1b, (void *)w0, (void *)b0, (void *)w1, (void *)b1, (void *)stats,
                    (void *)ns, (void *)lm, (void *)l1})
        CK(hipFree(p));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipStreamDestroy(s));
    return bad_total ? 2 : 0;
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 50;
    if (argc > 3) return run_shape(atoi(argv[2]), atoi(argv[3]), iters);
    int rc = run_shape(64, 1001, iters);
    if (rc == 1) return rc;             // a HIP error: nothing more is started
    const int rc2 = run_shape(64, 3001, iters);
    return rc ? rc : rc2;
}
