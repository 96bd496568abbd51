// qv_wpack_host.h -- host-side packers for the quantised weight layouts the GEMM kernels read (GemmArgs in qv_kernels.h:
// Wq / wscale for W4A16, W8 / w8scale for W8A16).  HIP-free (the standard library only): the half type H of the int4 scale
// table is the including file's (_Float16 in the library).  qv_model_prep_host.h and qv_capi.hip are the callers.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

// code q (0..15) of weight (n, kk) into the W4A16 image: [N/64][K/64][64 rows][32 B], one 64 x 64 tile of nibbles 2 KB
// contiguous; inside a row the 4-byte chunk c of 8 codes sits at c ^ ((n >> 2) & 7), and k = 2p -> nibble p, k = 2p + 1 ->
// nibble p + 4 of its chunk (dequant8 in qv_gemm_dequant.h unpacks two codes per OR)
inline void qv_w4_put(uint8_t *q_out, int n, int kk, int nk, int q) {
    const int kt = kk >> 6, c = (kk & 63) >> 3, e = kk & 7;
    const int nib = (e >> 1) + 4 * (e & 1);
    const int pos = c ^ ((n >> 2) & 7);
    const size_t byte = ((size_t)(n >> 6) * nk + kt) * 2048 + (size_t)(n & 63) * 32 + pos * 4 + (nib >> 1);
    if (nib & 1) q_out[byte] = (uint8_t)((q_out[byte] & 0x0F) | (q << 4));
    else q_out[byte] = (uint8_t)((q_out[byte] & 0xF0) | q);
}

// Symmetric block-128 int4 (w: [N][K] f32 row-major; N % 64 == 0, K % 128 == 0): per row and per 128 consecutive k,
// scale = v / -8 where v is the element of largest magnitude (first one on ties), q = clamp(floor(w / scale + 8.5), 0, 15),
// w' = (q - 8) * half(scale).  oracle/fastconformer_ref.py:quant_dequant_int4 mirrors this exactly.
template <class H>
void qv_pack_w4(const float *w, int N, int K, uint8_t *q_out, H *scale_out) {
    const int nk = K / 64, nkb = K / 128;
    for (int n = 0; n < N; ++n) {
        const float *row = w + (size_t)n * K;
        for (int kb = 0; kb < nkb; ++kb) {
            float vmax = 0.f, amax = -1.f;
            for (int k = 0; k < 128; ++k) {
                float a = fabsf(row[kb * 128 + k]);
                if (a > amax) { amax = a; vmax = row[kb * 128 + k]; }
            }
            float scale = vmax / -8.0f;
            float rs = scale != 0.f ? 1.0f / scale : 0.f;
            scale_out[((size_t)kb * N + n) * 2] = (H)scale;
            scale_out[((size_t)kb * N + n) * 2 + 1] = (H)(1024.f + 8.f);  // symmetric: zero point 8
            for (int k = 0; k < 128; ++k) {
                float t = row[kb * 128 + k] * rs + 8.0f;
                int q = (int)floorf(t + 0.5f);
                qv_w4_put(q_out, n, kb * 128 + k, nk, q < 0 ? 0 : q > 15 ? 15 : q);
            }
        }
    }
}

// The same device layout from a grid that is GIVEN (a weight file converted from the reference's quantised ONNX carries
// MatMulNBits' own block scales and zero points, tools/convert_weights.py; scale, zp: [N][K/128]): w[n][k] = (q - zp[n][kb]) *
// scale[n][kb] holds exactly in float32, so q = rint(w / scale + zp) returns the file's integer verbatim.  The device then
// multiplies by half(scale) -- the file's float32 scale rounded once, 2^-11 = 4.9e-4 relative at most -- and subtracts the
// file's zero point (asymmetric blocks included: the {scale, 1024 + zp} pair format always carried one).  Returns the number
// of elements that cannot be represented this way (0 for a consistent file): a recovered q that is not an integer in [0, 15]
// to 1e-3, and every element of a block whose zero point is not an integer in [0, 15] (half(1024 + zp) would round it) or
// whose scale leaves the normal range of f16 (it would be flushed or overflow on the device).  The caller keeps the
// dequantised f16 path for such a tensor (tools/convert_weights.py) instead of running it on a grid the file does not have.
template <class H>
int64_t qv_pack_w4_given(const float *w, int N, int K, const float *scale, const float *zp, uint8_t *q_out, H *scale_out) {
    const int nk = K / 64, nkb = K / 128;
    int64_t bad = 0;
    for (int n = 0; n < N; ++n) {
        const float *row = w + (size_t)n * K;
        for (int kb = 0; kb < nkb; ++kb) {
            const float sc = scale[(size_t)n * nkb + kb], z = zp[(size_t)n * nkb + kb];
            scale_out[((size_t)kb * N + n) * 2] = (H)sc;
            scale_out[((size_t)kb * N + n) * 2 + 1] = (H)(1024.f + z);
            const float asc = fabsf(sc);
            if (z != nearbyintf(z) || z < 0.f || z > 15.f || (sc != 0.f && (asc < 6.103515625e-05f || asc > 65504.f))) bad += 128;
            for (int k = 0; k < 128; ++k) {
                const float t = sc != 0.f ? row[kb * 128 + k] / sc + z : z;
                int q = (int)nearbyintf(t);
                if (fabsf(t - (float)q) > 1e-3f || q < 0 || q > 15) ++bad;
                qv_w4_put(q_out, n, kb * 128 + k, nk, q < 0 ? 0 : q > 15 ? 15 : q);
            }
        }
    }
    return bad;
}

// Per-row symmetric int8 (N % 64 == 0, K % 64 == 0): scale = max|w| / 127 (1 for an all-zero row), q = clamp(floor(w / scale
// + 0.5), -127, 127), stored as q + 128 in [N/64][K/64][64 rows][64 B] with the 8-byte chunk c of a row at c ^ ((n >> 2) & 7).
// oracle/fastconformer_ref.py:quant_dequant_int8 mirrors this exactly.
inline void qv_pack_w8(const float *w, int N, int K, uint8_t *q_out, float *scale_out) {
    const int nk = K / 64;
    for (int n = 0; n < N; ++n) {
        const float *row = w + (size_t)n * K;
        float amax = 0.f;
        for (int k = 0; k < K; ++k) amax = fmaxf(amax, fabsf(row[k]));
        const float scale = amax > 0.f ? amax / 127.0f : 1.0f;
        scale_out[n] = scale;
        for (int k = 0; k < K; ++k) {
            float t = row[k] / scale;
            int q = (int)floorf(t + 0.5f);
            q = q < -127 ? -127 : q > 127 ? 127 : q;
            const int kt = k >> 6, c = (k & 63) >> 3;
            const size_t byte = ((size_t)(n >> 6) * nk + kt) * 4096 + (size_t)(n & 63) * 64 + ((c ^ ((n >> 2) & 7)) << 3) + (k & 7);
            q_out[byte] = (uint8_t)(q + 128);
        }
    }
}
