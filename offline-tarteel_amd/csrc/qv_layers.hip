// qv_layers.hip -- the encoder's row kernels: LayerNorm, f16 / f32 conversion, the conv module's depthwise conv,
// log-softmax.  All of them are HBM-bound elementwise or small-reduction kernels.  The front end is qv_frontend.hip, the
// rel-pos attention qv_attention.hip, the audio ingest qv_ingest.hip.

#include "qv_layers.h"

#include "qv_dev_util.h"

#include <math.h>

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

// ------------------------------------------------------------------ LayerNorm ----------
// one wave per row of 512: f32 in -> f16 out (GEMM operand).  Two-pass variance in registers (ln_row_p, qv_dev_util.h).
// One wave normalises LN_ROWS consecutive rows: all their loads (and the parameters) are in flight
// before the first reduction, and a wave lives for LN_ROWS rows instead of one.
#ifndef LN_ROWS
#define LN_ROWS 2
#endif
__global__ __launch_bounds__(256) void k_layernorm(const float *__restrict__ x, const float *__restrict__ gam,
                                                   const float *__restrict__ bet, half_t *__restrict__ y, int M) {
    const int row0 = (xcd_order(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * LN_ROWS, lane = threadIdx.x & 63;
    if (row0 >= M) return;
    // (its own copy of ln_load_rows, qv_dev_util.h: through the shared loader this kernel allocates one VGPR more)
    f32x4 a[LN_ROWS], c[LN_ROWS];
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) {
        const int row = row0 + r < M ? row0 + r : M - 1;
        const float *p = x + (size_t)row * QV_D + lane * 8;
        a[r] = *(const f32x4 *)p; c[r] = *(const f32x4 *)(p + 4);
    }
    const LnParam pr = ln_param(gam, bet, lane);
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) {
        if (row0 + r >= M) break;
        float v[8] = {a[r][0], a[r][1], a[r][2], a[r][3], c[r][0], c[r][1], c[r][2], c[r][3]}, o[8];
        ln_row_p(v, pr, o);
        half8 h;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = (half_t)o[i];
        *(half8 *)(y + (size_t)(row0 + r) * QV_D + lane * 8) = h;
    }
}

// x <- LN_out(x) (f32, in place: the next layer's residual stream), y <- LN_next(x) (f16); with g2 == nullptr and y set
// (last layer) y is the f16 copy of LN_out(x) itself: the CTC head's operand, no separate conversion pass
__global__ __launch_bounds__(256) void k_layernorm2(float *__restrict__ x, const float *__restrict__ g1, const float *__restrict__ b1,
                                                    const float *__restrict__ g2, const float *__restrict__ b2,
                                                    half_t *__restrict__ y, int M) {
    const int row0 = (xcd_order(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * LN_ROWS, lane = threadIdx.x & 63;
    if (row0 >= M) return;
    float v[LN_ROWS][8];
    ln_load_rows<LN_ROWS>(x, row0, M, lane, v);
    const LnParam p1 = ln_param(g1, b1, lane);
    LnParam p2 = p1;
    const bool second = y && g2;
    if (second) p2 = ln_param(g2, b2, lane);
#pragma unroll
    for (int r = 0; r < LN_ROWS; ++r) {
        if (row0 + r >= M) break;
        float o[8], o2[8];
        ln_row_p(v[r], p1, o);
        store_c8(x + (size_t)(row0 + r) * QV_D + lane * 8, o);
        if (y) {
            if (second) ln_row_p(o, p2, o2);
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o2[i] = o[i];
            }
            half8 h;
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = (half_t)o2[i];
            *(half8 *)(y + (size_t)(row0 + r) * QV_D + lane * 8) = h;
        }
    }
}

// f32 -> f16 copy of the final encoder output (CTC head operand)
__global__ void k_to_half(const float *__restrict__ x, half_t *__restrict__ y, size_t n8) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    f32x4 a = *(const f32x4 *)(x + i * 8), c = *(const f32x4 *)(x + i * 8 + 4);
    half8 h = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3], (half_t)c[0], (half_t)c[1], (half_t)c[2], (half_t)c[3]};
    *(half8 *)(y + i * 8) = h;
}

// f16 -> f32 (debug taps)
__global__ void k_to_float(const half_t *__restrict__ x, float *__restrict__ y, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (float)x[i];
}

// ------------------------------------------------------------------ conv module --------
// depthwise Conv1d(512, k=9, pad 4) + folded BatchNorm + Swish on f16 [M][512]; input frames
// t >= len[b] read as zero (the reference zeroes padded frames after GLU).  A lane owns 8
// channels (weights [9][512] tap-major in registers) and slides over DW_TT consecutive frames,
// so each input row is loaded once per DW_TT outputs instead of 9 times.
#define DW_TT 4
__global__ __launch_bounds__(256) void k_dwconv1d(const half_t *__restrict__ x, const float *__restrict__ wt /*[9][512]*/,
                                                  const float *__restrict__ bias, const int32_t *__restrict__ len,
                                                  const int32_t *__restrict__ row_off, half_t *__restrict__ y) {
    // blocks in (utterance, frame chunk) order, XCD k takes the k-th eighth of them (xcd_order)
    const int wg = xcd_order(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    const int b = wg / gridDim.x, t0 = ((wg - b * gridDim.x) * 4 + (threadIdx.x >> 6)) * DW_TT, lane = threadIdx.x & 63;
    const int T = len[b], c0 = lane * 8;
    if (t0 >= T) return;
    const size_t row0 = (size_t)row_off[b];   // packed rows of utterance b
    float w[9][8], bs[8];
    load_taps9_c8(wt, QV_D, c0, w);
    load_c8(bias + c0, bs);
    float acc[DW_TT][8];
#pragma unroll
    for (int j = 0; j < DW_TT; ++j)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[j][c] = bs[c];
#pragma unroll
    for (int i = 0; i < DW_TT + 8; ++i) {
        int tt = t0 - 4 + i;
        if (tt < 0 || tt >= T) continue;
        half8 v = *(const half8 *)(x + (row0 + tt) * QV_D + c0);
        float vf[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) vf[c] = (float)v[c];
#pragma unroll
        for (int j = 0; j < DW_TT; ++j) {
            int k = i - j;  // tap index: tt = (t0 + j) + k - 4
            if (k < 0 || k > 8) continue;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[j][c] = __builtin_fmaf(w[k][c], vf[c], acc[j][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < DW_TT; ++j) {
        if (t0 + j >= T) break;
        half8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (half_t)(acc[j][c] * sigmoidf_(acc[j][c]));
        *(half8 *)(y + (row0 + t0 + j) * QV_D + c0) = o;
    }
}

// ------------------------------------------------------------------ log-softmax --------
// logits f32 [M][ld] (first 1025 valid) -> log-probs f32 [B][t_max][1025]; one wave per row.
__global__ __launch_bounds__(256) void k_logsoftmax(const float *__restrict__ logits, int ld, float *__restrict__ out, int M,
                                                    const int32_t *__restrict__ row_map, int t_out) {
    int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    // packed row -> (utterance, frame); the caller's log-prob tensor is dense [B][t_out][1025]
    const int bt = row_map[row];
    const size_t orow = (size_t)(bt >> 16) * t_out + (bt & 0xFFFF);
    const float *p = logits + (size_t)row * ld;
    float v[17];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        int c = lane + 64 * i;
        v[i] = c < 1025 ? p[c] : -INFINITY;
        mx = fmaxf(mx, v[i]);
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 17; ++i) s += (lane + 64 * i < 1025) ? expf(v[i] - mx) : 0.f;
    float lse = mx + logf(wave_sum(s));
    float *o = out + orow * 1025;
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        int c = lane + 64 * i;
        if (c < 1025) o[c] = v[i] - lse;
    }
}

// rows t >= T[b] of the caller's dense [B][t_out][1025] tensor: zeros (qv_forward's contract -- onnxruntime hands the
// reference exactly [1, T, 1025], mixed/run.py:59-63; a padded batch tensor must not expose uninitialised memory)
__global__ __launch_bounds__(256) void k_zero_pad_rows(float *__restrict__ out, const int32_t *__restrict__ len, int t_out) {
    const int b = blockIdx.y, t = len[b] + blockIdx.x;
    if (t >= t_out) return;
    float *o = out + ((size_t)b * t_out + t) * 1025;
    for (int c = threadIdx.x; c < 1025; c += 256) o[c] = 0.f;
}

}  // namespace

// ====================================================================== launchers ======

void launch_layernorm(const float *x, const float *g, const float *b, half_t *y, int M, hipStream_t s) {
    hipLaunchKernelGGL(k_layernorm, dim3((M + 4 * LN_ROWS - 1) / (4 * LN_ROWS)), dim3(256), 0, s, x, g, b, y, M);
}

void launch_layernorm2(float *x, const float *g1, const float *b1, const float *g2, const float *b2, half_t *y, int M,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_layernorm2, dim3((M + 4 * LN_ROWS - 1) / (4 * LN_ROWS)), dim3(256), 0, s, x, g1, b1, g2, b2, y, M);
}

void launch_to_half(const float *x, half_t *y, size_t n, hipStream_t s) {
    size_t n8 = n / 8;
    hipLaunchKernelGGL(k_to_half, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, y, n8);
}

void launch_to_float(const half_t *x, float *y, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_to_float, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
}

void launch_dwconv1d(const half_t *x, const float *w, const float *bias, const int32_t *len, const int32_t *row_off, half_t *y,
                     int t_max, int batch, hipStream_t s) {
    hipLaunchKernelGGL(k_dwconv1d, dim3((t_max + 4 * DW_TT - 1) / (4 * DW_TT), batch), dim3(256), 0, s, x, w, bias, len, row_off,
                       y);
}

void launch_logsoftmax(const float *logits, int ld, float *out, int M, const int32_t *row_map, int t_out, hipStream_t s) {
    hipLaunchKernelGGL(k_logsoftmax, dim3((M + 3) / 4), dim3(256), 0, s, logits, ld, out, M, row_map, t_out);
}

void launch_zero_pad_rows(float *out, const int32_t *len, int t_out, int t_min, int batch, hipStream_t s) {
    if (t_out <= t_min) return;   // every utterance fills the tensor
    hipLaunchKernelGGL(k_zero_pad_rows, dim3(t_out - t_min, batch), dim3(256), 0, s, out, len, t_out);
}
