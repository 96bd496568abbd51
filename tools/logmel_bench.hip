// logmel_bench.hip -- the log-mel kernel on its own: k_logmel_reg<0> (one wave per frame) against k_logmel_run<F> (a wave
// walks a run of F frames) on random audio, B clips of N samples (default 64 x 160,000, the headline batch).  HIP-event
// averages over back-to-back launches and a byte compare of the features.  F is the build's QV_LOGMEL_RUN:
//   for F in 2 4 8; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Xclang -target-feature -Xclang \
//         -packed-fp32-ops -DQV_LOGMEL_RUN=$F -I offline-tarteel_amd/csrc -I include tools/logmel_bench.hip -o tools/logmel_bench_f$F; done
//   tools/logmel_bench_f4 [iters] [B] [N]
// The tables are made here (Hann(400) centred in 512, exp(-2 pi i m / 512), 80 triangular filters on the HTK mel scale up
// to 8 kHz): the shapes of the product's tables, which is what the time depends on; the compare needs no particular values.
#include "../offline-tarteel_amd/csrc/qv_frontend.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 100, B = argc > 2 ? atoi(argv[2]) : 64, N = argc > 3 ? atoi(argv[3]) : 160000;
    const int tm = N / 160 + 1;
    const double pi = 3.14159265358979323846;
    std::vector<float> hwin(512, 0.f), hw(32 * QV_NMEL, 0.f), ha((size_t)B * N);
    std::vector<float2> htw(256);
    std::vector<int32_t> hlo(QV_NMEL), hcnt(QV_NMEL), hn(B, N);
    for (int i = 0; i < 400; ++i) hwin[56 + i] = (float)(0.5 - 0.5 * cos(2 * pi * i / 399));
    for (int m = 0; m < 256; ++m) htw[m] = make_float2((float)cos(2 * pi * m / 512), (float)-sin(2 * pi * m / 512));
    auto mel = [](double f) { return 2595.0 * log10(1.0 + f / 700.0); };
    auto bin = [&](double m) { return (700.0 * (pow(10.0, m / 2595.0) - 1.0)) / 8000.0 * 256.0; };
    for (int m = 0; m < QV_NMEL; ++m) {
        const double lo = bin(mel(8000.0) * m / (QV_NMEL + 1)), c = bin(mel(8000.0) * (m + 1) / (QV_NMEL + 1)),
                     hi = bin(mel(8000.0) * (m + 2) / (QV_NMEL + 1));
        int k0 = (int)floor(lo) + 1, k1 = (int)ceil(hi) - 1;
        if (k1 < k0) k1 = k0;
        if (k1 - k0 + 1 > 32) k1 = k0 + 31;
        if (k1 > 256) k1 = 256;
        hlo[m] = k0;
        hcnt[m] = k1 - k0 + 1;
        for (int k = k0; k <= k1; ++k) {
            const double v = k <= c ? (k - lo) / (c - lo) : (hi - k) / (hi - c);
            hw[(k - k0) * QV_NMEL + m] = (float)(v > 0 ? v : 0);
        }
    }
    srand(1);
    for (auto &x : ha) x = (rand() % 2001 - 1000) / 4000.0f;
    float *audio, *win, *w, *fa, *fb;
    float2 *tw;
    int32_t *lo, *cnt, *ns;
    const size_t nf = (size_t)B * tm * QV_NMEL;
    CK(hipMalloc(&audio, ha.size() * 4)); CK(hipMalloc(&win, 512 * 4)); CK(hipMalloc(&w, hw.size() * 4)); CK(hipMalloc(&tw, 256 * 8));
    CK(hipMalloc(&lo, QV_NMEL * 4)); CK(hipMalloc(&cnt, QV_NMEL * 4)); CK(hipMalloc(&ns, B * 4));
    CK(hipMalloc(&fa, nf * 4)); CK(hipMalloc(&fb, nf * 4));
    CK(hipMemcpy(audio, ha.data(), ha.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(win, hwin.data(), 512 * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(tw, htw.data(), 256 * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(lo, hlo.data(), QV_NMEL * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(cnt, hcnt.data(), QV_NMEL * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(ns, hn.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemset(fa, 0, nf * 4)); CK(hipMemset(fb, 0xff, nf * 4));
    const FrontendTab ft = {win, tw, lo, cnt, w};
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float ms[2] = {0.f, 0.f};
    for (int which = 0; which < 2; ++which) {
        auto go = [&] {
            if (which) hipLaunchKernelGGL(lmv::k_logmel_run<QV_LOGMEL_RUN>, dim3((tm + 4 * QV_LOGMEL_RUN - 1) / (4 * QV_LOGMEL_RUN), B), dim3(256), 0, s, audio, (int64_t)N, ns, ft, fb, tm);
            else hipLaunchKernelGGL(lmv::k_logmel_reg<0>, dim3((tm + 3) / 4, B), dim3(256), 0, s, audio, (int64_t)N, ns, ft, fa, tm);
        };
        for (int i = 0; i < 10; ++i) go();
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) go();
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        CK(hipGetLastError());
        CK(hipEventElapsedTime(&ms[which], e0, e1));
    }
    std::vector<float> ga(nf), gb(nf);
    CK(hipMemcpy(ga.data(), fa, nf * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(gb.data(), fb, nf * 4, hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < nf; ++i) bad += memcmp(&ga[i], &gb[i], 4) != 0;
    printf("B %d x %d samples (%d frames): k_logmel_reg<0> %.1f us, k_logmel_run<%d> %.1f us; features that differ: %zu of %zu\n", B, N, tm,
           ms[0] * 1000 / iters, QV_LOGMEL_RUN, ms[1] * 1000 / iters, bad, nf);
    return bad ? 2 : 0;
}
