// qv_gemm_epilogue.h -- everything the GEMM tile kernels must agree on BIT FOR BIT, defined once: k_gemm / k_gemm_pk
// (qv_gemm_body.inc), k_gemm256 (qv_gemm256.hip) and the measured-only k_gemm256q (tools/gemm256q.h) produce identical
// outputs because they run the same K order into the same accumulator layout and then THESE value functions.  What a kernel
// keeps for itself is how a tile is staged through LDS and read back, its buffer descriptors and its FOLD reduction.
// Also here: the one table of (weights, epilogue) pairs that exist, which both launchers instantiate from (bottom).
//
// Accumulator layout (operands swapped, D^T = W A^T): register quad q of a 32 x 32 fragment holds 4 CONSECUTIVE output
// columns, 8 * q + 4 * (lane >> 5) + 0..3, of tile row lane & 31.  The functions that run a packed activation (swish4 /
// sigmoid4) take a fragment and q, i.e. one such quad; the others take one value, and the kernel's own loop over a quad
// names the elements (with these shapes the kernels' instruction streams are the hand-written ones').
#pragma once

#include "qv_kernels.h"
#include "qv_gemm_dequant.h"
#include "qv_ort.h"

#include <utility>

// dev tools only (tools/gemm_trace.hip, tools/gemm256_trace.hip): ablation bits and time stamps; `g`, `tid`, `lane` in scope.
// A kernel's trace record layout is its own: it passes the element index (QV_BLOCK = the launch-order block id).
#define QV_BLOCK ((size_t)(blockIdx.y * gridDim.x + blockIdx.x))
#ifdef QV_GEMM_TRACE
#define QV_ABL(bit) (g.abl & (bit))
#define QV_PHASE(slot) do { if (g.phase && tid == 0) g.phase[QV_BLOCK * 4 + (slot)] = wall_clock64(); } while (0)
#define QV_TRACE_AT(cond, elem) do { if (g.trace && lane == 0 && (cond)) g.trace[elem] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define QV_ABL(bit) false
#define QV_PHASE(slot) do { } while (0)
#define QV_TRACE_AT(cond, elem) do { } while (0)
#endif

namespace qv_epi {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// the output is float32 (staged as floats), not f16
constexpr bool out_is_f32(int epi) { return epi == EPI_RESID || epi == EPI_F32; }

// XCD-aware tile order (bijective for any tile count): consecutive workgroup ids land on different XCDs (id % 8); each XCD
// gets a contiguous run of tiles, which share A row panels in its private L2
__device__ __forceinline__ int xcd_tile(int wg, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = wg & 7, idx = wg >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// EPI_F32 / EPI_RESID, one staged value: alpha * (acc [* scl] + bias); the residual's old quad is added at read-back
template <bool W8>
__device__ __forceinline__ float val_f32(float acc, float scl, float alpha, float bias) {
    float x = acc;
    if (W8) x *= scl;
    return alpha * (x + bias);
}
__device__ __forceinline__ void add_resid(f32x4 &v, const f32x4 &old) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += old[e];
}

// EPI_F16 / EPI_F16_SWISH / EPI_F16_RELU / the q, k columns of EPI_QKV: half(act(acc + bias))
template <int EPI, class ACC>
__device__ __forceinline__ half4 val_f16(const ACC &acc, int q, const f32x4 &bias) {
    half4 o;
    f32x4 xv;
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] = acc[q * 4 + e] + bias[e];
    if (EPI == EPI_F16_SWISH) xv = swish4(xv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = xv[e];
        if (EPI == EPI_F16_RELU) x = x > 0.f ? x : 0.f;
        o[e] = (half_t)x;
    }
    return o;
}

// EPI_GLU, f16 / W8A16: half((a [* sa] + ba) * sigmoid(gt [* sg] + bg)); a = value quad, gt = gate quad
template <bool W8, class ACC>
__device__ __forceinline__ half4 val_glu(const ACC &a, const ACC &gt, int q, const f32x4 &sa, const f32x4 &sg, const f32x4 &ba, const f32x4 &bg) {
    half4 o;
    f32x4 av, gv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        av[e] = a[q * 4 + e];
        gv[e] = gt[q * 4 + e];
        if (W8) { av[e] *= sa[e]; gv[e] *= sg[e]; }
        av[e] += ba[e];
        gv[e] += bg[e];
    }
    const f32x4 sgm = sigmoid4(gv);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (half_t)(av[e] * sgm[e]);
    return o;
}

// ---- A8W8 (QV_PREC_ORT_MIXED, qv_ort.h): int32 accumulator -> float32, per-utterance activation scale, bias, activation.
//   v = float(acc + (128 - zp_x[u]) * wsum[n]) * (s_x[u] * s_w) + bias[n]
// The int32 sum is < 2^24 in magnitude (K <= 512 products of |255| x |127|), so the conversion is exact and v carries
// exactly the two roundings the reference's Cast -> Mul -> Add chain has.
template <int EPI>
struct A8W8 {
    static constexpr bool GLU = EPI == EPI_GLU, OUT16 = EPI == EPI_F16_RELU;
    static constexpr bool RELU = EPI == EPI_F16_RELU || EPI == EPI_F32_RELU;
    static constexpr bool FOLD = EPI == EPI_GLU || EPI == EPI_F32_RELU;   // the output feeds another quantiser: track its range
};

// the utterance a row belongs to (its quantisation parameters and its range slot); valid = the row is inside its length
__device__ __forceinline__ int row_owner(const GemmArgs &g, int grow, bool &valid) {
    valid = true;
    if (g.row_map) return g.row_map[grow] >> 16;
    const int u = grow / g.rows_per_utt;
    valid = (grow - u * g.rows_per_utt) / g.f_per_t < g.len[u];
    return u;
}

// s_x[u] * s_w and 128 - zp_x[u] of utterance u
__device__ __forceinline__ void a8w8_row_param(const GemmArgs &g, int u, float &srow, int &zc) {
    const QParam p = dql_param(g.mm_in + QV_MM_STRIDE * u);
    srow = p.scale * g.w_scale;
    zc = 128 - (int)p.zp;
}

// running range of a row's outputs (feeds mm_fold / mm_fold_keys)
__device__ __forceinline__ void track(float v, float &mn, float &mx) {
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
}

// one A8W8 value (the kernels run sigmoid4 over a quad of gate values themselves: GLU = value * sigmoid(gate))
template <bool RELU>
__device__ __forceinline__ float val_a8w8(int acc, int zc, int wsum, float srow, float bias) {
    float v = (float)(acc + zc * wsum) * srow + bias;
    if (RELU) v = v > 0.f ? v : 0.f;
    return v;
}

// EPI_RESID read-back of the A8W8 kernels
__device__ __forceinline__ float a8w8_resid(float old, float alpha, float v) { return old + alpha * v; }

// ---- EPI_QKV, V columns: stored TRANSPOSED, Vt[b][h * 64 + d][t].  A thread owns the frame pair (r0, r0 + 1) of one d row;
// bt = (utterance << 16 | frame) of a row, -1 = no such row.
__device__ __forceinline__ half_t val_v(float a, float bias) { return (half_t)(a + bias); }
// element of Vt that row bt's value of d row `drow` goes to
__device__ __forceinline__ size_t vt_index(const GemmArgs &g, int bt, size_t drow) {
    return ((size_t)(bt >> 16) * QV_D + drow) * g.t_pad + (bt & 0xFFFF);
}

}  // namespace qv_epi

// ---- the (weights, epilogue) pairs that exist, once.  launch_gemm (128-wide tiles) and launch_gemm256 are functors over this
// table: f.template operator()<EPI, WQ>() launches the pair's kernel under the functor's own shape rules and returns whether
// it did.  WQ: 0 = f16 weights, 4 = W4A16, 8 = W8A16, 88 = A8W8.  false = no such pair (or the functor declined).
inline const char *gemm_epi_name(int epi) {
    static const char *const NAME[8] = {"f16", "f16_swish", "f16_relu", "glu", "resid", "f32", "qkv", "f32_relu"};   // (the EPI_ enum's order)
    return NAME[epi];
}
template <int WQ, class F, int... EPIS>
bool gemm_for_epi(int epi, F &&f, std::integer_sequence<int, EPIS...>) {
    return ((epi == EPIS && f.template operator()<EPIS, WQ>()) || ...);
}
template <class F>
bool gemm_for_pair(const GemmArgs &g, int epi, F &&f) {
    using std::integer_sequence;
    // A8W8 (QV_PREC_ORT_MIXED): the GEMM-shaped convolutions
    if (g.Wi8) return gemm_for_epi<88>(epi, f, integer_sequence<int, EPI_GLU, EPI_RESID, EPI_F32, EPI_F32_RELU, EPI_F16_RELU>{});
    // int4 weights: the Linear layers only (FFN, QKV, attention out, linear_pos)
    if (g.Wq) return gemm_for_epi<4>(epi, f, integer_sequence<int, EPI_F16, EPI_F16_SWISH, EPI_RESID, EPI_QKV>{});
    // int8 weights: the pointwise convolutions of the conv module
    if (g.W8) return gemm_for_epi<8>(epi, f, integer_sequence<int, EPI_GLU, EPI_RESID>{});
    return gemm_for_epi<0>(epi, f, integer_sequence<int, EPI_F16, EPI_F16_SWISH, EPI_F16_RELU, EPI_RESID, EPI_F32, EPI_QKV, EPI_GLU>{});
}
