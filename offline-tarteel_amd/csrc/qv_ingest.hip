// qv_ingest.hip -- audio ingest, ahead of any forward: the polyphase resampler and the channel mix-down.  Only the audio
// entry points launch these kernels (launchers declared in qv_layers.h).

#include "qv_layers.h"

// ---------------------------------------------------------------- a15: polyphase resampler ----
// scipy.signal.upfirdn's float32 inner loop, one output sample per thread (tta/run.py:60-71 reaches
// it through resample_poly).  hflip[t][j] = h[t + up * (P - 1 - j)] (zero beyond n_taps) is built
// on the host, so a thread walks x forwards and its phase row forwards, exactly scipy's order;
// out-of-range inputs are skipped like scipy's index clamping does, not added as zeros.
namespace {
// output sample m (counted from the start of the whole output) of a row of n_in samples: the one definition of the FIR's
// arithmetic.  x_at(i) is input sample i of the row, taps the [up][P] per-phase filter; either may sit in global memory or LDS.
template <typename X>
__device__ __forceinline__ float upfirdn_sample(int64_t m, int64_t n_in, const float *taps, int P, int up, int down, X x_at) {
    const int64_t pos = m * down;
    const int64_t xi = pos / up;
    const int t = (int)(pos - xi * up);
    const float *h = taps + (size_t)t * P;
    const int64_t first = xi - (P - 1);
    const int j0 = first < 0 ? (int)(-first) : 0;
    const int64_t last = xi < n_in - 1 ? xi : n_in - 1;   // last valid input index
    float acc = 0.f;
    for (int64_t i = first + j0; i <= last; ++i) acc = __fadd_rn(acc, __fmul_rn(x_at(i), h[i - first]));
    return acc;
}

__global__ __launch_bounds__(256) void k_upfirdn(const float *__restrict__ x, int64_t n_in, const float *__restrict__ hflip,
                                                 int P, int up, int down, int64_t m0, int64_t n_out, float *__restrict__ y) {
    int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= n_out) return;
    y[m] = upfirdn_sample(m0 + m, n_in, hflip, P, up, down, [&](int64_t i) { return x[i]; });
}
// The same FIR for a BATCH of rows in one launch (round 6: the TTA wrapper's 0.9x / 1.1x copies of every gated clip, the
// 44.1 / 48 kHz -> 16 kHz ingest of audio.load_audio_device): output row r reads source row src[r] (or r) of x, n_in[r]
// samples long, writes ceil(n_in[r] * up / down) samples and zeroes the rest of its pitch -- the engine's [B, N]
// zero-padded input layout.  Per output sample the arithmetic is k_upfirdn's, term for term.
__global__ __launch_bounds__(256) void k_upfirdn_rows_direct(const float *__restrict__ x, int64_t x_pitch, const int32_t *__restrict__ src,
                                                             const int64_t *__restrict__ n_in_rows, const float *__restrict__ hflip,
                                                             int P, int up, int down, int64_t m0, float *__restrict__ y, int64_t y_pitch) {
    const int r = blockIdx.y;
    const int64_t n_in = n_in_rows[r];
    const int64_t n_out = (n_in * up + down - 1) / down;
    const float *xr = x + (size_t)(src ? src[r] : r) * x_pitch;
    float *yr = y + (size_t)r * y_pitch;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < y_pitch; m += (int64_t)gridDim.x * 256) {
        if (m >= n_out) { yr[m] = 0.f; continue; }
        yr[m] = upfirdn_sample(m0 + m, n_in, hflip, P, up, down, [&](int64_t i) { return xr[i]; });
    }
}

// ... and with the operands staged in LDS: the 256 outputs of a block read one window of x (256 * down / up + P samples) and
// the whole per-phase filter (up * P taps); from global memory every thread walked its P taps with two dependent loads per
// product (809 us per launch for 64 clips x 33 s in the TTA profile of round 6).  Same products, same order, same bits.
__global__ __launch_bounds__(256) void k_upfirdn_rows(const float *__restrict__ x, int64_t x_pitch, const int32_t *__restrict__ src,
                                                      const int64_t *__restrict__ n_in_rows, const float *__restrict__ hflip,
                                                      int P, int up, int down, int64_t m0, float *__restrict__ y, int64_t y_pitch, int xspan) {
    extern __shared__ __attribute__((aligned(16))) float sm_up[];
    float *sh = sm_up, *sx = sm_up + up * P;
    const int r = blockIdx.y, tid = threadIdx.x;
    const int64_t n_in = n_in_rows[r];
    const int64_t n_out = (n_in * up + down - 1) / down;
    const float *xr = x + (size_t)(src ? src[r] : r) * x_pitch;
    float *yr = y + (size_t)r * y_pitch;
    for (int i = tid; i < up * P; i += 256) sh[i] = hflip[i];
    for (int64_t mb = (int64_t)blockIdx.x * 256; mb < y_pitch; mb += (int64_t)gridDim.x * 256) {
        const int64_t m = mb + tid;
        if (mb >= n_out) {                                   // (uniform: the whole block is in the zero padding)
            if (m < y_pitch) yr[m] = 0.f;
            continue;
        }
        const int64_t m_hi = mb + 255 < n_out - 1 ? mb + 255 : n_out - 1;
        int64_t x_lo = ((m0 + mb) * down) / up - (P - 1), x_hi = ((m0 + m_hi) * down) / up;
        x_lo = x_lo < 0 ? 0 : x_lo;
        x_hi = x_hi < n_in - 1 ? x_hi : n_in - 1;
        __syncthreads();                                     // the previous window has been consumed (and the taps are in place)
        for (int64_t i = x_lo + tid; i <= x_hi; i += 256) sx[i - x_lo] = xr[i];
        __syncthreads();
        if (m >= y_pitch) continue;
        if (m >= n_out) { yr[m] = 0.f; continue; }
        yr[m] = upfirdn_sample(m0 + m, n_in, sh, P, up, down, [&](int64_t i) { return sx[i - x_lo]; });
    }
}

// interleaved [frames][channels] float32 -> mono: numpy's float32 mean over the channel axis, what audio._read_wav / the
// reference's soundfile fallback do (shared/audio.py:13-15): one division of the frame's sum by the channel count, the sum
// taken in the order of numpy's float32 add-reduce along a contiguous axis.  Below 8 channels that is left to right from
// +0 (so a frame of -0.0 gives +0.0, as numpy's does).  From 8 channels up (and to 128: the entry point stops at 64) it
// keeps eight running sums r[k] = x[k], r[k] += x[8 i + k] over the whole groups of eight, joins them as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and adds the channels % 8 tail one by one; the +0 goes in last, where
// it changes nothing but the sign of a zero.
__global__ __launch_bounds__(256) void k_mixdown(const float *__restrict__ x, int64_t x_pitch, const int64_t *__restrict__ n_frames,
                                                 int channels, float *__restrict__ y, int64_t y_pitch) {
    const int r = blockIdx.y;
    const int64_t n = n_frames[r];
    const float *xr = x + (size_t)r * x_pitch;
    float *yr = y + (size_t)r * y_pitch;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float *f = xr + i * channels;
        float acc = 0.f;
        if (channels < 8) {
            for (int c = 0; c < channels; ++c) acc = __fadd_rn(acc, f[c]);
        } else {
            float s[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] = f[k];
            int c = 8;
            for (; c + 8 <= channels; c += 8)
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] = __fadd_rn(s[k], f[c + k]);
            float t = __fadd_rn(__fadd_rn(__fadd_rn(s[0], s[1]), __fadd_rn(s[2], s[3])),
                                __fadd_rn(__fadd_rn(s[4], s[5]), __fadd_rn(s[6], s[7])));
            for (; c < channels; ++c) t = __fadd_rn(t, f[c]);
            acc = __fadd_rn(t, 0.f);
        }
        yr[i] = __fdiv_rn(acc, (float)channels);
    }
}
}  // namespace

void launch_upfirdn_rows(const float *x, int64_t x_pitch, const int32_t *src, const int64_t *n_in_rows, int rows, const float *hflip,
                         int P, int up, int down, int64_t m0, float *y, int64_t y_pitch, hipStream_t s) {
    if (rows <= 0 || y_pitch <= 0) return;
    const int64_t bx = (y_pitch + 255) / 256;
    // window of x a block of 256 outputs reads (+ 2: the two floor divisions at its ends) and the filter, in LDS when they fit
    const int64_t xspan = (256 * (int64_t)down) / up + P + 2;
    const size_t lds = ((size_t)up * P + (size_t)xspan) * sizeof(float);
    if (lds <= 60 * 1024)
        hipLaunchKernelGGL(k_upfirdn_rows, dim3((unsigned)(bx < 4096 ? bx : 4096), rows), dim3(256), lds, s, x, x_pitch, src, n_in_rows, hflip, P, up,
                           down, m0, y, y_pitch, (int)xspan);
    else
        hipLaunchKernelGGL(k_upfirdn_rows_direct, dim3((unsigned)(bx < 4096 ? bx : 4096), rows), dim3(256), 0, s, x, x_pitch, src, n_in_rows, hflip,
                           P, up, down, m0, y, y_pitch);
}

void launch_mixdown(const float *x, int64_t x_pitch, const int64_t *n_frames, int rows, int channels, float *y, int64_t y_pitch,
                    int64_t max_frames, hipStream_t s) {
    if (rows <= 0 || max_frames <= 0) return;
    const int64_t bx = (max_frames + 255) / 256;
    hipLaunchKernelGGL(k_mixdown, dim3((unsigned)(bx < 4096 ? bx : 4096), rows), dim3(256), 0, s, x, x_pitch, n_frames, channels, y, y_pitch);
}

void launch_upfirdn(const float *x, int64_t n_in, const float *hflip, int P, int up, int down, int64_t m0, int64_t n_out,
                    float *y, hipStream_t s) {
    if (n_out <= 0) return;
    hipLaunchKernelGGL(k_upfirdn, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, x, n_in, hflip, P, up, down, m0,
                       n_out, y);
}
