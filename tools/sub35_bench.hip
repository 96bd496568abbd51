// sub35_bench.hip -- conv.3 + ReLU + conv.5 of the f16 front end on their own: the pair the forward used to launch
// (k_gemm256<f16_relu> + k_dwconv2d, c1p through HBM, c2 dense) against k_sub35 (c2 packed) on random c1, B utterances of
// T2 c1 frames each (default: 64 x 251, the headline batch, then 64 x 751, the 30 s one).  HIP-event averages over
// back-to-back launches and a byte compare of c2.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I offline-tarteel_amd/csrc -I include \
//         tools/sub35_bench.hip -o tools/sub35_bench
//   tools/sub35_bench [iters] [B] [T2]
#include "../offline-tarteel_amd/csrc/qv_frontend.hip"
#include "../offline-tarteel_amd/csrc/qv_gemm256.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int run_shape(int B, int T2, int iters) {
    const int T3 = (T2 - 1) / 2 + 1;
    const size_t n1 = (size_t)B * T2 * 20 * QV_SUBC, n2 = (size_t)B * T3 * 10 * QV_SUBC;
    std::vector<half_t> hc1(n1), hw3((size_t)QV_SUBC * QV_SUBC);
    std::vector<float> hb3(QV_SUBC), hw5(9 * QV_SUBC), hb5(QV_SUBC);
    srand(1);
    auto rnd = [] { return (rand() % 2001 - 1000) / 1000.0f; };
    for (auto &x : hc1) x = (half_t)fabsf(rnd());          // (c1 is a ReLU-free depthwise output; any finite values do)
    for (auto &x : hw3) x = (half_t)(rnd() * 0.1f);
    for (auto &x : hb3) x = rnd() * 0.1f;
    for (auto &x : hw5) x = rnd() * 0.3f;
    for (auto &x : hb5) x = rnd() * 0.1f;
    std::vector<int32_t> hl2(B, T2), hl3(B, T3), hoff(B);
    for (int b = 0; b < B; ++b) hoff[b] = b * T3;
    half_t *c1, *c1p, *c2a, *c2b, *w3;
    float *b3, *w5, *b5;
    int32_t *l2, *l3, *off, *row_map;
    CK(hipMalloc(&c1, n1 * 2)); CK(hipMalloc(&c1p, n1 * 2)); CK(hipMalloc(&c2a, n2 * 2)); CK(hipMalloc(&c2b, n2 * 2));
    CK(hipMalloc(&w3, hw3.size() * 2)); CK(hipMalloc(&b3, QV_SUBC * 4)); CK(hipMalloc(&w5, 9 * QV_SUBC * 4)); CK(hipMalloc(&b5, QV_SUBC * 4));
    CK(hipMalloc(&l2, B * 4)); CK(hipMalloc(&l3, B * 4)); CK(hipMalloc(&off, B * 4)); CK(hipMalloc(&row_map, (size_t)B * T3 * 4));
    CK(hipMemcpy(c1, hc1.data(), n1 * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(w3, hw3.data(), hw3.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(b3, hb3.data(), QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w5, hw5.data(), 9 * QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(b5, hb5.data(), QV_SUBC * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(l2, hl2.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(l3, hl3.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(off, hoff.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemset(c2a, 0, n2 * 2)); CK(hipMemset(c2b, 0xff, n2 * 2));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    GemmArgs g = {};
    g.alpha = 1.f;
    g.A = c1; g.W = w3; g.bias = b3; g.out = c1p;
    g.M = B * T2 * 20; g.N = QV_SUBC; g.K = QV_SUBC; g.lda = QV_SUBC; g.ldw = QV_SUBC; g.ldo = QV_SUBC;
    auto pair = [&] {
        launch_gemm256(EPI_F16_RELU, g, s, 256);
        launch_dwconv2d(c1p, T2, 20, l2, w5, b5, c2a, T3, 10, B, s);
    };
    auto fused = [&] { launch_sub35(c1, T2, w3, b3, w5, b5, l2, l3, off, c2b, row_map, T3, B, s); };
    float ms_pair = 0.f, ms_fused = 0.f;
    for (int which = 0; which < 2; ++which) {
        for (int i = 0; i < 10; ++i) which ? fused() : pair();
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) which ? fused() : pair();
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        CK(hipGetLastError());
        CK(hipEventElapsedTime(which ? &ms_fused : &ms_pair, e0, e1));
    }
    std::vector<half_t> ha(n2), hb(n2);
    std::vector<int32_t> hmap((size_t)B * T3);
    CK(hipMemcpy(ha.data(), c2a, n2 * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), c2b, n2 * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hmap.data(), row_map, hmap.size() * 4, hipMemcpyDeviceToHost));
    size_t bad = 0, bad_map = 0;
    for (size_t i = 0; i < n2; ++i) bad += memcmp(&ha[i], &hb[i], 2) != 0;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T3; ++t) bad_map += hmap[(size_t)b * T3 + t] != ((b << 16) | t);
    printf("B %d x %d c1 frames (%d c2 frames, run %d steps): pair %.1f us (k_gemm256<f16_relu> + k_dwconv2d), k_sub35 %.1f us; "
           "c2 halves that differ: %zu of %zu, row_map entries wrong: %zu\n",
           B, T2, T3, qv_sub35_run_frames(B, T3) / S35_TC, ms_pair * 1000 / iters, ms_fused * 1000 / iters, bad, n2, bad_map);
    for (void *p : {(void *)c1, (void *)c1p, (void *)c2a, (void *)c2b, (void *)w3, (void *)b3, (void *)w5, (void *)b5, (void *)l2,
                    (void *)l3, (void *)off, (void *)row_map})
        CK(hipFree(p));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipStreamDestroy(s));
    return (bad || bad_map) ? 2 : 0;
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 100;
    if (argc > 3) return run_shape(atoi(argv[2]), atoi(argv[3]), iters);
    int rc = run_shape(64, 251, iters);
    if (rc == 1) return rc;             // a HIP error: nothing more is started
    const int rc2 = run_shape(64, 751, iters);
    return rc ? rc : rc2;
}
