// qv_gemm.hip -- fused-epilogue f16 GEMM on v_mfma_f32_32x32x16_f16 (see qv_kernels.h).
//
// C[M,N] = epilogue(A[M,K] * W[N,K]^T + bias).  128 x BN x 64 tiles (BN = 128 or 64), 512 threads: 4 consumer waves
// (2 x 2, fragment reads + MFMA + epilogue) and 4 loader waves (register-staged MUBUF loads into a 2-stage LDS
// ring by default; direct global->LDS loads with 2..4 stages under QVERSE_GEMM_LD=0).  The large shapes run on the
// 256 x 256-tile kernel of qv_gemm256.hip instead (launch_gemm's plan, bottom of this file); both kernels produce
// bit-identical results.  The epilogue goes back through LDS so that every
// global store is a full 16-byte lane-contiguous row segment (a wave writes 4 whole tile rows per
// instruction); storing straight from the MFMA accumulator layout (one row per lane) cost more
// time than the whole K loop.

#include "qv_kernels.h"
#include "qv_gemm_epilogue.h"
#include "qv_launch_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

namespace {

typedef const __attribute__((address_space(1))) void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

__device__ __forceinline__ void glds16(const void *g, void *l) {
    // direct global->LDS, 16 B per lane; LDS destination = wave-uniform base + lane * 16
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}

}  // namespace

// Wave specialisation: 512 threads.  Waves 0..3 (one per SIMD) are CONSUMERS: fragment reads from LDS
// and MFMAs only (2 x 2 layout, 64 x BN/2 each), then the epilogue.  Waves 4..7 are LOADERS: they only
// issue the direct global->LDS loads of the stage NST - 1 K-steps ahead.  A wave that does both pays
// the issue time of its 8 loads (hundreds of cycles per K-step) in front of its 16 MFMAs; split, the
// loads issue under the partner wave's MFMAs (tools/gemm_exp.hip: 7-17 % per GEMM at these shapes).
//
// LD selects how the loader waves move a K-step's operands into LDS:
//   LD = 0  direct global->LDS loads (global_load_lds_dwordx4), NST LDS stages, counted vmcnt
//   LD = 1  REGISTER staging through MUBUF: buffer_load_dwordx4 into VGPRs (a loader wave holds no
//           accumulators, so it has ~100 VGPRs to spare) and ds_write_b128 into a 2-stage LDS ring; the
//           prefetch depth (two K-steps) lives in registers, not in LDS.  Why (tools/stage_bench.hip, 4 loader
//           + 4 MFMA waves per CU): while a SIMD's matrix pipe runs back-to-back MFMAs, the FLAT-encoded
//           loads of its other waves (global_load_lds_dwordx4 AND global_load_dwordx4 -- their 64-bit
//           address goes through the VALU) hardly issue at all: 2 MB per CU took 86 / 74 us under 61 us of
//           dense MFMAs against 27 / 17 us alone, i.e. the loads ran AFTER the MFMAs.  Buffer loads (SGPR
//           descriptor + 32-bit offset, no VALU pass) are not blocked: 18.8 us under the same MFMA load
//           (53 B/clk/CU), and the MFMA waves lose < 2 %.
template <int EPI, int BN, int WQ, int NST, int LD>
__global__ __launch_bounds__(512, 4) void k_gemm(GemmArgs g) {
#include "qv_gemm_body.inc"
}

// Round 6 (advisor): the whole library is built WITHOUT packed-FP32 code generation (offline-tarteel_amd/build.py: the
// v_pk_*_f32 class is what the cross-kernel disturbance of DESIGN.md 4.1 corrupts) -- the GEMM translation units included.
// Two instantiations of the 128-wide kernel (W8A16, register-staged loaders, two stages: GLU and residual epilogue, the
// pointwise convolutions of precision 1) do not fit the 128-VGPR budget of their 512-thread block without the packed forms
// (7 spilled registers, and a spill's scratch traffic would break the loaders' hand-counted vmcnt).  They alone keep the
// feature, as their own kernel symbol: tests/test_capi_load.py allows v_pk_*_f32 in k_gemm_pk<...> and nowhere else, and
// the interference probe runs them as victims (tests/test_gpu_interference.py).
template <int EPI, int BN, int WQ, int NST, int LD>
__global__ __launch_bounds__(512, 4) __attribute__((target("packed-fp32-ops"))) void k_gemm_pk(GemmArgs g) {
#include "qv_gemm_body.inc"
}

template <int EPI, int BN, int WQ, int NST, int LD>
constexpr bool gemm_needs_pk() { return WQ == 8 && BN == 128 && NST == 2 && LD == 1 && (EPI == EPI_GLU || EPI == EPI_RESID); }

template <int EPI, int BN, int WQ, int NST, int LD = 0>
static void launch_one(const GemmArgs &g, hipStream_t s) {
    constexpr bool W4 = WQ == 4, W8 = WQ == 8;
    dim3 grid(g.N / BN, (g.M + 127) / 128);
    size_t lds = W4 ? NST * ((128 * 64 * 2) + (BN * 32)) + (size_t)BN * (g.K / 128) * 4
                    : W8 ? NST * ((128 * 64 * 2) + (BN * 64)) : NST * ((128 * 64 * 2) + (BN * 64 * 2));
    size_t epi = qv_epi::out_is_f32(EPI) ? (size_t)128 * (BN + 4) * 4 : (size_t)128 * (BN + 8) * 2;
    if (WQ == 88) epi = (size_t)128 * ((EPI == EPI_GLU ? BN / 2 : BN) + 4) * 4 + 128 * 3 * 4;   // f32 staging + per-row range keys and owners
    if (epi > lds) lds = epi;
    // more than 64 KB of dynamic LDS is opted into, once per instantiation and only where needed
    if (lds > 64 * 1024) {
        static size_t allowed = 0;
        if (lds > allowed) {
            if constexpr (gemm_needs_pk<EPI, BN, WQ, NST, LD>())
                (void)hipFuncSetAttribute((const void *)k_gemm_pk<EPI, BN, WQ, NST, LD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            else
                (void)hipFuncSetAttribute((const void *)k_gemm<EPI, BN, WQ, NST, LD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            allowed = lds;
        }
    }
    if constexpr (gemm_needs_pk<EPI, BN, WQ, NST, LD>()) hipLaunchKernelGGL((k_gemm_pk<EPI, BN, WQ, NST, LD>), grid, dim3(512), lds, s, g);
    else hipLaunchKernelGGL((k_gemm<EPI, BN, WQ, NST, LD>), grid, dim3(512), lds, s, g);
}

// tile width BN in {64, 128} and LDS stage count NST in {2, 3, 4} (see launch_gemm)
template <int EPI, int WQ>
static void launch_shape(const GemmArgs &g, hipStream_t s, bool narrow, int nst) {
    if constexpr (WQ == 8) {
        // int8 weights (the two pointwise-convolution shapes) only exist with register-staged loaders: their direct-to-LDS
        // variants (QVERSE_GEMM_LD=0) needed 4-12 spilled VGPRs at the 128-register budget, i.e. scratch traffic inside a
        // loop whose vmcnt waits are counted by hand (tests/test_capi_load.py keeps the binary free of such kernels)
        launch_one<EPI, 128, 8, 2, 1>(g, s);
    } else if (nst == 0) {   // register-staged loaders (2-stage LDS ring)
        if (narrow) launch_one<EPI, 64, WQ, 2, 1>(g, s);
        else launch_one<EPI, 128, WQ, 2, 1>(g, s);
    } else if (narrow) {
        if (nst == 2) launch_one<EPI, 64, WQ, 2>(g, s);
        else launch_one<EPI, 64, WQ, 3>(g, s);
    } else {
        if (nst == 2) launch_one<EPI, 128, WQ, 2>(g, s);
        else if (nst == 3) launch_one<EPI, 128, WQ, 3>(g, s);
        else launch_one<EPI, 128, WQ, 4>(g, s);
    }
}

// ---- measurement hook: HIP-event timing of every GEMM launch, per (epilogue, tile) class ----
namespace {
struct GemmProf {
    bool on = false;
    std::vector<hipEvent_t> ev;   // pairs
    std::vector<int> cls;
    std::vector<double> flops;
} g_prof;
}  // namespace

bool qv_gemm_prof_on() { return g_prof.on; }

void qv_gemm_prof_enable(bool on) {
    g_prof.on = on;
    g_prof.cls.clear();
    g_prof.flops.clear();
}

// call after the stream has been synchronised; accumulates into ms[21], flops[21], n[21]
// (class = epilogue * 3 + tile: 0 = 64-wide, 1 = 128-wide, 2 = 256 x 256)
void qv_gemm_prof_collect(double *ms, double *flops, int *n) {
    for (int i = 0; i < 21; ++i) { ms[i] = 0; flops[i] = 0; n[i] = 0; }
    for (size_t i = 0; i < g_prof.cls.size(); ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) continue;
        ms[g_prof.cls[i]] += t;
        flops[g_prof.cls[i]] += g_prof.flops[i];
        n[g_prof.cls[i]] += 1;
    }
    g_prof.cls.clear();
    g_prof.flops.clear();
}

// the 128-wide path of a (weights, epilogue) pair of the table (qv_gemm_epilogue.h): its shape rules, then the instantiation
// gemm_kernel (qv_launch_plan.h) names
struct Launch128 {
    const GemmArgs &g;
    hipStream_t s;
    GemmKernel k;
    template <int EPI, int WQ>
    bool operator()() const {
        if constexpr (WQ == 88) {
            // 128-wide tiles, register-staged loaders
            if (g.N % 128 != 0 || !g.wsum || !g.mm_in) abort();
            launch_one<EPI, 128, 88, 2, 1>(g, s);
        } else if constexpr (WQ == 8) {
            if (k.bn != 128 || g.N % 128 != 0) abort();
            launch_shape<EPI, 8>(g, s, false, k.nst);
        } else {
            launch_shape<EPI, WQ>(g, s, k.bn == 64, k.ld == 1 ? 0 : k.nst);
        }
        return true;
    }
};

// what the tile policy (gemm_plan, qv_launch_plan.h) reads of a call
static GemmShape gemm_shape(int epi, const GemmArgs &g) {
    return {g.M, g.N, g.K, g.Wq ? GEMM_W_INT4 : g.Wi8 ? GEMM_W_A8W8 : g.W8 ? GEMM_W_INT8 : GEMM_W_F16, g.bias != nullptr, epi == EPI_GLU, g.in_flight};
}

// "k_gemm256<f16_swish>" / "k_gemm<resid,128>": the kernel launch_gemm picks for this call (measurement reports).  A pipeline
// that is not the default's register staging shows: "k_gemm<resid,128,lds3>" = direct global->LDS loads, 3 stages.
const char *qv_gemm_kernel_name(int epi, const GemmArgs &g, const QvSwitches &sw) {
    static thread_local char buf[64];
    const char *name = gemm_epi_name(epi);
    const GemmShape sh = gemm_shape(epi, g);
    const GemmPlan p = gemm_plan(sh, sw);
    const GemmKernel k = gemm_kernel(sh, p);
    if (g.Wi8) snprintf(buf, sizeof buf, p.wide ? (p.bm == 192 ? "k_gemm256<%s,a8w8,192>" : "k_gemm256<%s,a8w8>") : "k_gemm<%s,128,a8w8>", name);
    else if (p.wide) snprintf(buf, sizeof buf, p.bm == 192 ? "k_gemm256<%s,192>" : "k_gemm256<%s>", name);
    else if (k.ld == 0) snprintf(buf, sizeof buf, "k_gemm<%s,%d,lds%d>", name, k.bn, k.nst);
    else snprintf(buf, sizeof buf, "k_gemm<%s,%d>", name, k.bn);
    return buf;
}

void launch_gemm(int epi, const GemmArgs &g, hipStream_t s, const QvSwitches &sw) {
    if (g.K % 64 != 0 || g.N % 64 != 0 || (g.Wq && g.K % 128 != 0)) {
        fprintf(stderr, "launch_gemm: unsupported shape N=%d K=%d\n", g.N, g.K);
        abort();
    }
    const GemmShape sh = gemm_shape(epi, g);
    const GemmPlan p = gemm_plan(sh, sw);
    const GemmKernel k = gemm_kernel(sh, p);
    auto go = [&] {
        if (p.wide && launch_gemm256(epi, g, s, p.bm)) return;
        if (!gemm_for_pair(g, epi, Launch128{g, s, k})) abort();   // no kernel for this (weights, epilogue) pair
    };
    if (!g_prof.on) { go(); return; }
    size_t i = g_prof.cls.size();
    while (g_prof.ev.size() < 2 * (i + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { go(); return; }
        g_prof.ev.push_back(e);
    }
    (void)hipEventRecord(g_prof.ev[2 * i], s);
    go();
    (void)hipEventRecord(g_prof.ev[2 * i + 1], s);
    g_prof.cls.push_back((epi == EPI_F32_RELU ? EPI_F16_RELU : epi) * 3 + (p.wide ? 2 : k.bn == 64 ? 0 : 1));   // (21 classes in the ABI)
    g_prof.flops.push_back(2.0 * (double)g.M * (double)g.N * (double)g.K * (g.Wi8 ? 2.0 : 1.0));
}
