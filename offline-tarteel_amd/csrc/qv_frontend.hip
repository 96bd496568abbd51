// qv_frontend.hip -- the front end of the FastConformer forward: log-mel features and their statistics, the strided conv
// subsampling (conv.0 to conv.5) and the packing of its rows.  HBM/LDS-bound kernels, conv.0 and conv.3 on the matrix pipe;
// the encoder's row kernels are qv_layers.hip.

#include "qv_layers.h"

#include "qv_dev_util.h"
#include "qv_launch_plan.h"
#include "qv_logmel_reg.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------ front-end ----------
// One wave per STFT frame: pre-emphasis + reflect padding + Hann window on load; the 512 real
// samples are packed as 256 complex ones (z[n] = x[2n] + i x[2n+1]), transformed with a 256-point
// radix-2 Stockham FFT in LDS (8 passes, 2 butterflies per lane per pass) and unpacked to the 257
// bins of the real transform; power spectrum, sparse mel projection (each filter touches <= 32
// bins), log(x + 2^-24).
__global__ __launch_bounds__(256) void k_logmel(const float *__restrict__ audio, int64_t n_max,
                                                const int32_t *__restrict__ n_samples, const FrontendTab ft,
                                                float *__restrict__ feats, int tm_max) {
    __shared__ float2 buf[4][2][256];
    __shared__ float pw[4][264];
    __shared__ float2 tw[256];   // the twiddle table: every FFT pass fetched its factors from global memory (waves parked 79 %)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y, t = blockIdx.x * 4 + wave;
    const int n = n_samples[b];
    const int tm = n / 160 + 1;
    tw[threadIdx.x] = ft.twiddle[threadIdx.x];
    __syncthreads();
    if (t >= tm) return;  // frames past the utterance are zeroed by the normalisation kernel
    const float *x = audio + (size_t)b * n_max;
    float2 *A = buf[wave][0], *Bf = buf[wave][1];
    auto sample = [&](int i) {
        int s = t * 160 - 256 + i;
        if (s < 0) s = -s;
        if (s >= n) s = 2 * (n - 1) - s;
        s = s < 0 ? 0 : s;
        float y = x[s] - (s > 0 ? 0.97f * x[s - 1] : 0.f);
        return y * ft.window[i];
    };
    for (int i = lane; i < 256; i += 64) A[i] = make_float2(sample(2 * i), sample(2 * i + 1));
    // Stockham autosort, radix 2, N = 256: pass p (len = 1 << p): out[j*2*len + k] , out[... + len]
    float2 *src = A, *dst = Bf;
    for (int p = 0; p < 8; ++p) {
        int len = 1 << p;  // half-size of the butterflies produced so far
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < 128; i += 64) {
            int k = i & (len - 1), j = i >> p;  // j: group, k: index within group
            float2 u = src[j * len + k], v = src[j * len + k + 128];
            // twiddle w = exp(-2 pi i * k / (2 len)) from the 512-point table
            float2 w = tw[k * (256 >> p)];
            float2 vw = make_float2(__builtin_fmaf(v.x, w.x, -(v.y * w.y)), __builtin_fmaf(v.x, w.y, v.y * w.x));
            dst[j * 2 * len + k] = make_float2(u.x + vw.x, u.y + vw.y);
            dst[j * 2 * len + k + len] = make_float2(u.x - vw.x, u.y - vw.y);
        }
        float2 *tmp = src; src = dst; dst = tmp;
    }
    __builtin_amdgcn_wave_barrier();
    // X[k] = E[k] - i W^k O[k],  E = (Z[k] + conj Z[256-k]) / 2,  O = (Z[k] - conj Z[256-k]) / 2,  W = exp(-2 pi i / 512)
    for (int k = lane; k < 257; k += 64) {
        float2 X;
        if (k == 0 || k == 256) {
            float2 z0 = src[0];
            X = make_float2(k == 0 ? z0.x + z0.y : z0.x - z0.y, 0.f);
        } else {
            float2 zk = src[k], zc = src[256 - k];
            float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
            float2 O = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y + zc.y));
            float2 w = tw[k];
            float2 P = make_float2(__builtin_fmaf(w.x, O.x, -(w.y * O.y)), __builtin_fmaf(w.x, O.y, w.y * O.x));
            X = make_float2(E.x + P.y, E.y - P.x);
        }
        float mag = sqrtf(X.x * X.x + X.y * X.y);
        pw[wave][k] = mag * mag;
    }
    __builtin_amdgcn_wave_barrier();
    float *out = feats + ((size_t)b * tm_max + t) * QV_NMEL;
    for (int m = lane; m < QV_NMEL; m += 64) {
        int lo = ft.mel_lo[m], cnt = ft.mel_cnt[m];
        const float *w = ft.mel_w + m;        // tap-major [32][80]
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) acc += w[k * QV_NMEL] * pw[wave][lo + k];
        out[m] = logf(acc + 5.9604644775390625e-08f);
    }
}

// per-feature sum / sum of squares over the valid frames (f64 accumulation); the normalisation itself is applied by conv0
// while it loads its input rows, so the features make no extra round trip through HBM.
// Each of the MS_CHUNKS blocks of an utterance writes its partial sums and k_melstats_sum adds them in chunk order.  (Until
// round 4 the blocks added their partials to the result with f64 atomics, i.e. in whatever order they finished: the last
// bit of a sum then depends on what else the GPU is running.  This was the SECOND, independent source of run-to-run
// differences found while chasing the 38-of-1,500 soak mismatches of round 4; the first and larger one was the packed-FP32
// hazard in k_logmel's unpack step that round 5 pinned down -- build.py, tests/test_gpu_interference.py.)
#define MS_CHUNKS 16
__global__ __launch_bounds__(320) void k_melstats(const float *__restrict__ feats, const int32_t *__restrict__ n_samples,
                                                  int tm_max, double *__restrict__ part /*[B][MS_CHUNKS][80][2]*/) {
    __shared__ double p1[4][QV_NMEL], p2[4][QV_NMEL];
    const int b = blockIdx.y, f = threadIdx.x % QV_NMEL, g = threadIdx.x / QV_NMEL;  // 4 time groups
    const int tm = n_samples[b] / 160 + 1;
    const int per = (tm + MS_CHUNKS - 1) / MS_CHUNKS, t0 = blockIdx.x * per, t1 = min(tm, t0 + per);
    const float *x = feats + (size_t)b * tm_max * QV_NMEL;
    double s1 = 0.0, s2 = 0.0;
    for (int t = t0 + g; t < t1; t += 4) { double v = x[t * QV_NMEL + f]; s1 += v; s2 += v * v; }
    p1[g][f] = s1;
    p2[g][f] = s2;
    __syncthreads();
    if (g == 0) {     // an empty chunk writes zeros
        double *o = part + (((size_t)b * MS_CHUNKS + blockIdx.x) * QV_NMEL + f) * 2;
        o[0] = p1[0][f] + p1[1][f] + p1[2][f] + p1[3][f];
        o[1] = p2[0][f] + p2[1][f] + p2[2][f] + p2[3][f];
    }
}
__global__ __launch_bounds__(2 * QV_NMEL) void k_melstats_sum(const double *__restrict__ part, double *__restrict__ acc /*[B][80][2]*/) {
    const int b = blockIdx.x, i = threadIdx.x;      // i = feature * 2 + {sum, sum of squares}
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < MS_CHUNKS; ++c) s += part[((size_t)b * MS_CHUNKS + c) * (2 * QV_NMEL) + i];
    acc[(size_t)b * 2 * QV_NMEL + i] = s;
}

// materialise the normalised features (only for the debug tap / parity tests)
__global__ __launch_bounds__(320) void k_melapply(const float *__restrict__ feats, const int32_t *__restrict__ n_samples,
                                                  int tm_max, const double *__restrict__ acc, float *__restrict__ out) {
    const int b = blockIdx.y, f = threadIdx.x % QV_NMEL, g = threadIdx.x / QV_NMEL;
    const int tm = n_samples[b] / 160 + 1;
    float mean, rstd;
    mel_mean_rstd(acc, b, f, tm, mean, rstd);
    for (int t = blockIdx.x * 4 + g; t < tm_max; t += gridDim.x * 4) {
        size_t i = ((size_t)b * tm_max + t) * QV_NMEL + f;
        out[i] = t < tm ? (feats[i] - mean) * rstd : 0.f;
    }
}

// ------------------------------------------------------------------ subsampling --------
// conv0: Conv2d(1->256, 3x3, s2, p1) + ReLU on [B][Tm][80] -> channels-last f16 [B][T1][40][256].
// Round 4: on the f32 matrix pipe.  As 9 FMAs per output on the VALU this layer was 6 GFLOP per batch at 17 % of the
// packed-FMA peak, issue-bound (k_sub01: 36 packed FMAs + ~30 address / LDS instructions per position and thread).
// It is a [channels] x [9 taps] x [positions] product: v_mfma_f32_32x32x2_f32 takes two taps per instruction, so a
// 32-channel x 32-position tile is five of them (the tenth tap is zero) with the bias as the initial accumulator --
// float32 operands and accumulation like before, only the summation order inside the instruction is the hardware's.
// A operand: lane (l31 = channel, hi = tap parity) holds w[2j + hi][channel]; B operand: lane (l31 = position, hi)
// holds the input sample of tap 2j + hi at that position; D register r of lane (l31 = position, hi) is channel
// (r & 3) + 8 (r >> 2) + 4 hi.  conv0_taps / conv0_tile are shared by the fused kernel and the two-kernel cross-check
// path, which therefore still agree bit for bit.
__device__ __forceinline__ void conv0_weights(const float *__restrict__ wt /*[9][256]*/, const float *__restrict__ bias, int ch0,
                                              int l31, int hi, float wa[5], float bc[16]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) wa[j] = 2 * j + hi < 9 ? wt[(2 * j + hi) * QV_SUBC + ch0 + l31] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) bc[r] = bias[ch0 + (r & 3) + 8 * (r >> 2) + 4 * hi];
}
// (conv0_tap_offsets / conv0_taps, the B operand fetch, live in qv_dev_util.h: precision 2's front end uses them too)
__device__ __forceinline__ f32x16 conv0_tile(const float wa[5], const float bc[16], const float xb[5]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bc[r];
#pragma unroll
    for (int j = 0; j < 5; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j], xb[j], acc, 0, 0, 0);
    return acc;
}

// ReLU + conversion of a D tile's 16 registers: convert first (round to nearest even, v_cvt_pk_f16_f32), then clamp the
// f16 BITS as signed integers (a negative float is a negative int16; one v_pk_max_i16 per two channels).
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ half4 conv0_relu4(const f32x16 &acc, int q) {
    const float4_t v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    const half4 h = __builtin_convertvector(v, half4);
    short4_t b = __builtin_bit_cast(short4_t, h);
    b = __builtin_elementwise_max(b, (short4_t){0, 0, 0, 0});
    return __builtin_bit_cast(half4, b);
}

// two-kernel path (QVERSE_SUB_UNFUSED=1, the cross-check of k_sub01): block = one output row t1; the 3 input rows sit in
// LDS; wave w owns channel tiles 2w and 2w + 1, both position tiles (40 positions = 32 + 8).
__global__ __launch_bounds__(256) void k_conv0(const float *__restrict__ feats, int tm_max, const int32_t *__restrict__ len_in,
                                               const double *__restrict__ stats, const float *__restrict__ wt /*[9][256]*/,
                                               const float *__restrict__ bias, half_t *__restrict__ out, int t1_max) {
    __shared__ float rows[3][QV_NMEL + 2];
    __shared__ float mean_s[QV_NMEL], rstd_s[QV_NMEL];
    const int b = blockIdx.z, t1 = blockIdx.y, tid = threadIdx.x;
    const int tin = len_in[b];
    const float *x = feats + (size_t)b * tm_max * QV_NMEL;
    if (tid < QV_NMEL) mel_mean_rstd(stats, b, tid, tin, mean_s[tid], rstd_s[tid]);
    __syncthreads();
    stage_mel_rows<3>(rows, x, 2 * t1 - 1, tin, mean_s, rstd_s, [](float v) { return v; });
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    int koff[5];
    conv0_tap_offsets(hi, koff);
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int ch0 = (2 * wave + ct) * 32;
        float wa[5], bc[16];
        conv0_weights(wt, bias, ch0, l31, hi, wa, bc);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int f1 = pt * 32 + l31, f1c = f1 < 40 ? f1 : 39;
            float xb[5];
            conv0_taps(&rows[0][0], 0, f1c, koff, xb);
            const f32x16 acc = conv0_tile(wa, bc, xb);
            if (f1 < 40) {
                half_t *o = out + (((size_t)b * t1_max + t1) * 40 + f1) * QV_SUBC + ch0 + 4 * hi;
#pragma unroll
                for (int q = 0; q < 4; ++q) *(half4 *)(o + 8 * q) = conv0_relu4(acc, q);
            }
        }
    }
}

// depthwise Conv2d(256, 3x3, s2, p1, groups=256) on channels-last f16; rows t >= len_in[b] read as 0.
// Same ownership as conv0: 8 channels per thread, weights [9][256] in registers.
#define DW2_TT 4
__global__ __launch_bounds__(256) void k_dwconv2d(const half_t *__restrict__ in, int tin_max, int fin,
                                                  const int32_t *__restrict__ len_in, const float *__restrict__ wt,
                                                  const float *__restrict__ bias, half_t *__restrict__ out, int tout_max,
                                                  int fout) {
    // a block owns DW2_TT consecutive output frames: the 80 weights a thread fetches serve DW2_TT x fout / 8 outputs
    // instead of fout / 8 (they were most of the block's L2 traffic), and with fout = 10 the 8 position slots of a
    // channel group are all busy (40 positions / 8) instead of 10 of 16
    const int b = blockIdx.z, to0 = blockIdx.y * DW2_TT, tid = threadIdx.x;
    const int tin = len_in[b];
    const int c0 = (tid & 31) * 8, fl = tid >> 5;
    float w[9][8], bs[8];
    load_taps9_c8(wt, QV_SUBC, c0, w);
    load_c8(bias + c0, bs);
    for (int p = fl; p < DW2_TT * fout; p += 8) {
        const int to = to0 + p / fout, fo = p % fout;
        if (to >= tout_max) break;
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = bs[c];
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
            int t = 2 * to - 1 + dt;
            if (t < 0 || t >= tin) continue;
#pragma unroll
            for (int df = 0; df < 3; ++df) {
                int f = 2 * fo - 1 + df;
                if (f < 0 || f >= fin) continue;
                half8 v = *(const half8 *)(in + (((size_t)b * tin_max + t) * fin + f) * QV_SUBC + c0);
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = __builtin_fmaf(w[dt * 3 + df][c], (float)v[c], acc[c]);
            }
        }
        half8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (half_t)acc[c];
        *(half8 *)(out + (((size_t)b * tout_max + to) * fout + fo) * QV_SUBC + c0) = o;
    }
}

// conv0 + ReLU + first depthwise conv in one kernel: the [B][T1][40][256] activation (657 MB at
// B = 64 x 10 s) never goes to HBM.  A block walks a RUN of consecutive tiles of one utterance (a tile = 4 output frames
// = 8 new conv0 rows + the row before them), 64 channels at a time: conv0 of the 8 new rows goes through the f32 matrix
// pipe into an LDS tile as f16 (same rounding as the two-kernel path), the depthwise 3x3/s2 reads it from there.
//   * loop order "channel group outer, tiles inner": a group's weights of both convolutions are fetched once and stay in
//     registers for the whole run (21 conv0 values per lane: a wave owns ONE 32-channel half; 40 depthwise values per
//     thread: 4 channels), and the statistics -> mean / rstd are formed once per block
//   * no halo inside a run: the last conv0 row of a tile is the first of the next one; the wave that computes it stores
//     it twice (tile row 8 and the other one of two halo rows), so nothing is recomputed or copied.  A step is then
//     8 x 40 = 320 positions = exactly 10 position tiles of 32 = 20 (position tile, channel half) units, five per wave;
//     only the first step of a pass also computes the halo row (one more unit per wave)
//   * rows outside [0, len1) -- the depthwise conv's zero padding -- are written as zeros by the conv0 epilogue itself
//   * depthwise stage: 80 positions x 16 four-channel chunks = 1,280 items, five per thread
//   * the 19 mel rows of the next step are requested before the current step's products and normalised into the other
//     row buffer behind its depthwise stage
//   * RESIDENT (runs of at most SUB_RES_RUN tiles): the normalised mel rows of the WHOLE run stay in LDS (16 run + 3 rows;
//     tile k reads rows 16 k .. 16 k + 18).  The prologue fills them, all loads in flight at once; the four passes fetch,
//     normalise and store nothing.  Without it every mel row of a run is loaded, normalised and stored four times.  LDS: 54,592 (tile +
//     halo) + 640 + 67 x 328 = 77,208 bytes at a run of 4; a run of 5 would need 82,456 -- hence the cap, and the
//     two-buffer variant stays for the longer runs QV_KV_SUB_RUN can force.  The same values from the same operations
//     reach conv0 either way.
// Every output element is formed by the same instructions on the same operands whatever the run length (and as in the
// two-kernel path): the run length only decides which block forms it.
// LDS tile: position p (row * 40 + f) owns 64 channels at a pitch of 136 bytes.  The conv0 epilogue stores 8 bytes per
// lane for 32 consecutive positions: 32 x 136 bytes touch every bank pair once.  The depthwise stage reads 8 bytes per
// lane, 16 lanes per position; lanes 0-15 / 16-31 of a half-wave read output frames tl / tl + 1, whose inputs lie
// 80 positions = 42.5 x 256 bytes apart: the two 128-byte pieces fall on the two halves of the 64 banks.  The second halo
// row starts at a multiple of 256 bytes for the same reason.
// (SUB_TT = 4 c1 frames per tile, SUB_MAX_RUN, SUB_RES_RUN: qv_limits.h)
#define SUB_R1 (2 * SUB_TT + 1)     // c0 rows per tile
#define SUB_RM (2 * SUB_R1 + 1)     // mel rows per tile
#define SUB_MSTEP (4 * SUB_TT)       // mel rows from a tile to the next
#define SUB_CG 64                   // channels per pass
#define SUB_PP 68                   // halves per position of the LDS tile (136 bytes)
#define SUB_HALO1 24576             // halves: the second halo row (49,152 bytes = 192 x 256, behind rows 0 .. 8)
#define SUB_MEL_PER_THREAD ((SUB_RM * QV_NMEL + 255) / 256)
// QV_SUB01_STAMPS (tools/sub01_bench only, never the product build): wave 0 of one block in the middle of the grid adds up
// its clock between the phase boundaries -- 0 prologue, 1 conv0 units (with a pass's weight fetch), 2 the barrier behind
// them, 3 depthwise stage, 4 mel store, 5 the barrier behind it -- and leaves the sums in a buffer nothing else reads.
// The stamps' waits forbid overlaps the product kernel has: read the shares, not the length.
#ifdef QV_SUB01_STAMPS
__device__ unsigned long long qv_sub01_stamps[6];
__device__ __forceinline__ unsigned long long sub_clock() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define SUB_STAMP_BEGIN unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_last = sub_clock()
#define SUB_STAMP(p) do { const unsigned long long t_ = sub_clock(); st_acc[p] += t_ - st_last; st_last = t_; } while (0)
#define SUB_STAMP_END do { if (blockIdx.y == gridDim.y / 2 && blockIdx.z == gridDim.z / 2 && threadIdx.x == 0) \
    for (int p_ = 0; p_ < 6; ++p_) qv_sub01_stamps[p_] = st_acc[p_]; } while (0)
#else
#define SUB_STAMP_BEGIN
#define SUB_STAMP(p)
#define SUB_STAMP_END
#endif
template <bool RESIDENT>
__global__ __launch_bounds__(256) void k_sub01(const float *__restrict__ feats, int tm_max, const int32_t *__restrict__ len_mel,
                                               const double *__restrict__ stats, const float *__restrict__ w0t,
                                               const float *__restrict__ b0, const int32_t *__restrict__ len1,
                                               const float *__restrict__ w1t, const float *__restrict__ b1,
                                               half_t *__restrict__ out, int t2_max, int run) {
    constexpr int N_ROWS = RESIDENT ? SUB_MSTEP * SUB_RES_RUN + 3 : 2 * SUB_RM;   // the run's rows, or two buffers of a tile's
    __shared__ __attribute__((aligned(16))) float rows[N_ROWS][QV_NMEL + 2];
    __shared__ float mean_s[QV_NMEL], rstd_s[QV_NMEL];
    __shared__ __attribute__((aligned(256))) half_t tile[SUB_HALO1 + 40 * SUB_PP];
    static_assert(SUB_HALO1 >= SUB_R1 * 40 * SUB_PP && (SUB_HALO1 * 2) % 256 == 0, "k_sub01: the second halo row lies behind the tile");
    // ~68 KB of static LDS: gfx950 only (160 KB per CU, two blocks resident); every other target stops at 64 KB per block
    static_assert(sizeof(rows) + sizeof(tile) + sizeof(mean_s) + sizeof(rstd_s) <= 80 * 1024,
                  "k_sub01: two blocks per CU need <= 80 KB of LDS each");
    SUB_STAMP_BEGIN;
    const int b = blockIdx.z, tid = threadIdx.x;
    const int n_tiles = (t2_max + SUB_TT - 1) / SUB_TT;
    const int tile0 = blockIdx.y * run;                                     // first tile of the run
    const int nk = n_tiles - tile0 < run ? n_tiles - tile0 : run;           // tiles this block walks (>= 1 by the grid)
    const int tin = len_mel[b], l1 = len1[b];
    const float *x = feats + (size_t)b * tm_max * QV_NMEL;
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int ct = wave & 1, pt0 = wave >> 1;           // conv0 stage: the wave's channel half, its position tiles pt0 + 2 i
    // depthwise stage: 4 channels; frame tlb + 2 (wave >> 1) of the tile, positions fq .. fq + 4
    const int c4 = (tid & 15) * 4, tlb = (tid >> 4) & 1, th = wave >> 1, fq = ((tid >> 5) & 3) * 5;
    int koff[5];
    conv0_tap_offsets(hi, koff);
    // the mel rows of tile `tl`: row r is mel frame 16 tl - 3 + r.  Requested here, normalised and stored by mel_store
    // (normalisation as in k_conv0: frames past the utterance and the conv padding read as 0)
    float pf[SUB_MEL_PER_THREAD];
    auto mel_fetch = [&](int tl) {
#pragma unroll
        for (int i = 0; i < SUB_MEL_PER_THREAD; ++i) {
            // (always a load from inside the utterance: no branch around it; mel_store drops what lies outside)
            const int e = min(tid + 256 * i, SUB_RM * QV_NMEL - 1), r = e / QV_NMEL, f = e - r * QV_NMEL;
            const int t = min(max(16 * tl - 3 + r, 0), tin - 1);
            pf[i] = x[t * QV_NMEL + f];
        }
    };
    auto mel_store = [&](int tl, int buf) {
#pragma unroll
        for (int i = 0; i < SUB_MEL_PER_THREAD; ++i) {
            const int e = tid + 256 * i, r = e / QV_NMEL, f = e - r * QV_NMEL, t = 16 * tl - 3 + r;
            if (e < SUB_RM * QV_NMEL) rows[buf * SUB_RM + r][f + 1] = (t >= 0 && t < tin) ? (pf[i] - mean_s[f]) * rstd_s[f] : 0.f;
        }
    };
    if (RESIDENT) {
        // all 16 nk + 3 rows of the run at once: every load is issued before the statistics, one wait, then the stores
        constexpr int PER_THREAD = (N_ROWS * QV_NMEL + 255) / 256;
        const int n_el = (SUB_MSTEP * nk + 3) * QV_NMEL;
        float pr[PER_THREAD];
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const int e = min(tid + 256 * i, n_el - 1), r = e / QV_NMEL, f = e - r * QV_NMEL;
            const int t = min(max(16 * tile0 - 3 + r, 0), tin - 1);
            pr[i] = x[t * QV_NMEL + f];
        }
        if (tid < QV_NMEL) mel_mean_rstd(stats, b, tid, tin, mean_s[tid], rstd_s[tid]);
        for (int i = tid; i < 2 * N_ROWS; i += 256) rows[i >> 1][i & 1 ? QV_NMEL + 1 : 0] = 0.f;      // the padding columns
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const int e = tid + 256 * i, r = e / QV_NMEL, f = e - r * QV_NMEL, t = 16 * tile0 - 3 + r;
            if (e < n_el) rows[r][f + 1] = (t >= 0 && t < tin) ? (pr[i] - mean_s[f]) * rstd_s[f] : 0.f;
        }
    } else {
        mel_fetch(tile0);
        if (tid < QV_NMEL) mel_mean_rstd(stats, b, tid, tin, mean_s[tid], rstd_s[tid]);
        for (int i = tid; i < 2 * N_ROWS; i += 256) rows[i >> 1][i & 1 ? QV_NMEL + 1 : 0] = 0.f;      // the padding columns
        __syncthreads();
        mel_store(tile0, 0);
    }
    __syncthreads();
    SUB_STAMP(0);
    int it = 0;                     // steps done: step `it` reads its tile's rows (RESIDENT) / row buffer it & 1
    for (int cg = 0; cg < QV_SUBC; cg += SUB_CG) {
        float wa[5], bc[16];
        conv0_weights(w0t, b0, cg + 32 * ct, l31, hi, wa, bc);
        float w[9][4], bs[4];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const f32x4 v = *(const f32x4 *)(w1t + k * QV_SUBC + cg + c4);
#pragma unroll
            for (int c = 0; c < 4; ++c) w[k][c] = v[c];
        }
        {
            const f32x4 v = *(const f32x4 *)(b1 + cg + c4);
#pragma unroll
            for (int c = 0; c < 4; ++c) bs[c] = v[c];
        }
        for (int k = 0; k < nk; ++k, ++it) {
            const int tl0 = tile0 + k;
            const int t1_0 = 2 * SUB_TT * tl0 - 1;          // the halo row; the new rows are t1_0 + 1 .. t1_0 + 8
            const float *rw = &rows[RESIDENT ? SUB_MSTEP * k : (it & 1) * SUB_RM][0];
            // the next step's mel rows (the first tile again behind the last step of a pass); RESIDENT: they are there
            const int nxt = k + 1 < nk ? tl0 + 1 : tile0;
            const bool more = !RESIDENT && (k + 1 < nk || cg + SUB_CG < QV_SUBC);
            if (more) mel_fetch(nxt);
            // ---- conv0 + ReLU into the LDS tile on the f32 matrix pipe
            if (k == 0) {           // the halo row of the run: 40 positions, wave = (position tile pt0, channel half ct)
                const int f1 = pt0 * 32 + l31, f1c = f1 < 40 ? f1 : 39;
                float xb[5];
                conv0_taps(rw, 0, f1c, koff, xb);
                const f32x16 acc = conv0_tile(wa, bc, xb);
                if (f1 < 40) {
                    half_t *trow = tile + f1 * SUB_PP + 32 * ct + 4 * hi;
                    const bool zero = t1_0 < 0 || t1_0 >= l1;
#pragma unroll
                    for (int q = 0; q < 4; ++q) *(half4 *)(trow + 8 * q) = zero ? half4{0, 0, 0, 0} : conv0_relu4(acc, q);
                }
            }
            half_t *const halo_w = tile + ((k + 1) & 1 ? SUB_HALO1 : 0);       // where the NEXT step finds its halo row
            const half_t *const halo_r = tile + (k & 1 ? SUB_HALO1 : 0);
            {
                // unit i: new positions (pt0 + 2 i) * 32 + l31 of 320, new row r = tile row r + 1.  The products of unit
                // i + 1 are issued in front of unit i's conversion and stores
                float xb[5];
                conv0_taps(rw, 2 * (pt0 * 32 + l31 >= 40 ? 2 : 1), (pt0 * 32 + l31) % 40, koff, xb);
                f32x16 acc = conv0_tile(wa, bc, xb);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int n = (pt0 + 2 * i) * 32 + l31, r = n / 40, f1 = n - r * 40;
                    f32x16 nacc = acc;
                    if (i + 1 < 5) {
                        const int n2 = n + 64, r2 = n2 / 40;
                        conv0_taps(rw, 2 * (r2 + 1), n2 - r2 * 40, koff, xb);
                        nacc = conv0_tile(wa, bc, xb);
                    }
                    half_t *trow = tile + (n + 40) * SUB_PP + 32 * ct + 4 * hi;
                    const bool zero = t1_0 + 1 + r >= l1;           // (t1_0 + 1 + r >= 0 always)
                    half4 h[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) h[q] = zero ? half4{0, 0, 0, 0} : conv0_relu4(acc, q);
#pragma unroll
                    for (int q = 0; q < 4; ++q) *(half4 *)(trow + 8 * q) = h[q];
                    if (i == 4 && r == 2 * SUB_TT - 1) {            // the tile's last row is the next step's halo row
                        half_t *hrow = halo_w + f1 * SUB_PP + 32 * ct + 4 * hi;
#pragma unroll
                        for (int q = 0; q < 4; ++q) *(half4 *)(hrow + 8 * q) = h[q];
                    }
                    acc = nacc;
                }
            }
            SUB_STAMP(1);
            __syncthreads();            // conv0 done: the tile is complete
            SUB_STAMP(2);
            // ---- depthwise 3x3 stride 2 over the tile: all nine reads of an item are issued, then its 36 FMAs; the tap
            // left of the first position (f = -1) reads position 0 instead and its FMAs are dropped
            {
                const int tl = tlb + 2 * th, t2 = SUB_TT * tl0 + tl;
                const half_t *rb[3];
#pragma unroll
                for (int dt = 0; dt < 3; ++dt)
                    rb[dt] = (dt == 0 && tl == 0 ? halo_r : tile + (2 * tl + dt) * 40 * SUB_PP) + c4 + (2 * fq - 1) * SUB_PP;
                half_t *o = out + (((size_t)b * t2_max + (t2 < t2_max ? t2 : t2_max - 1)) * 20 + fq) * QV_SUBC + cg + c4;
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const bool edge = i == 0 && fq == 0;
                    half4 v[3][3];
#pragma unroll
                    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
                        for (int df = 0; df < 3; ++df)
                            v[dt][df] = *(const half4 *)(rb[dt] + (2 * i + (i == 0 && df == 0 && edge ? 1 : df)) * SUB_PP);
                    float acc[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = bs[c];
#pragma unroll
                    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
                        for (int df = 0; df < 3; ++df)
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                const float a = __builtin_fmaf(w[dt * 3 + df][c], (float)v[dt][df][c], acc[c]);
                                acc[c] = (i == 0 && df == 0 && edge) ? acc[c] : a;
                            }
                    half4 h;
#pragma unroll
                    for (int c = 0; c < 4; ++c) h[c] = (half_t)acc[c];
                    if (t2 < t2_max) *(half4 *)(o + i * QV_SUBC) = h;
                }
            }
            SUB_STAMP(3);
            if (more) mel_store(nxt, (it + 1) & 1);
            SUB_STAMP(4);
            __syncthreads();            // the depthwise stage has left the tile; the next step's mel rows are in LDS
            SUB_STAMP(5);
        }
    }
    SUB_STAMP_END;
}

// dense [B][t_max][row_elems] -> packed [sum of len][row_elems]: utterance b's valid frames become
// rows row_off[b] .. row_off[b] + len[b] - 1 (from here on padding frames do not exist).  Also
// records each packed row's owner, row_map[row] = utterance << 16 | frame, for the kernels that
// have to go back from a row to its utterance (V transpose in the QKV epilogue, log-softmax).
__global__ void k_pack_rows(const half_t *__restrict__ x, int t_max, int row_elems, const int32_t *__restrict__ len,
                            const int32_t *__restrict__ row_off, half_t *__restrict__ y, int32_t *__restrict__ row_map) {
    const int b = blockIdx.z, t = blockIdx.y;
    if (t >= len[b]) return;
    const half_t *p = x + ((size_t)b * t_max + t) * row_elems;
    half_t *q = y + ((size_t)row_off[b] + t) * row_elems;
    if (threadIdx.x == 0) row_map[row_off[b] + t] = (b << 16) | t;
    for (int i = threadIdx.x * 8; i < row_elems; i += blockDim.x * 8) *(half8 *)(q + i) = *(const half8 *)(p + i);
}

// conv.3 (pointwise 256 -> 256) + ReLU + conv.5 (depthwise 3x3 / s2) in one kernel: the [B][T2][20][256] activation
// between them (c1p, 164.5 MB at B = 64 x 10 s) never goes to HBM, and c2 comes out PACKED (frame t3 < len3[b] of
// utterance b at rows (off[b] + t3) * 10 .. + 9), with row_map beside it: no k_pack_rows, no work on padding frames.
// A block of eight waves owns one utterance and a run of consecutive c2 frames and walks it S35_TC frames a step:
//   * a step's 2 S35_TC new c1 frames are 120 consecutive rows of c1 = one 128-row GEMM tile (8 rows of padding whose
//     products are dropped).  They go global -> registers (MUBUF buffer_load_dwordx4, one step ahead, in flight under
//     the products and the depthwise stage of the step before) -> LDS in the GEMM kernels' swizzled image (four
//     64-deep K-tiles of 128-byte rows, chunk c of row r at c ^ ((r >> 1) & 7)).  Rows past the utterance's buffer
//     read as zero through the descriptor's bounds check; nothing below reads what is computed from them.
//   * wave w owns output channels 32 w .. 32 w + 31 and keeps ITS [32 x 256] slice of conv.3's weights in registers for
//     the whole run (16 MFMA operand fragments = 64 VGPRs): weights are fetched once per block and never staged.
//   * c1p of the step -- (half_t) relu(acc + bias), acc from mfma_f32_32x32x16_f16(W fragment, A fragment, acc) over
//     K = 0, 16, .. 240 from zero: the instructions and the order of k_gemm / k_gemm256 with EPI_F16_RELU -- is written
//     into an LDS tile as f16.  Its last frame is the next step's first: the epilogue stores it twice (tile and the
//     other one of two halo slots); only a run's first step computes the frame in front of it.
//   * the depthwise stage reads the tile: thread = 4 channels (lane) x positions wave, wave + 8, ..; sum from the bias,
//     fmaf per tap, dt outer / df inner, as k_dwconv2d.  Taps outside the utterance or the frequency axis are DROPPED
//     by selects (the row / the tap was formed from clamped addresses), never multiplied by zero; the only branch is
//     the store guard.
// Every output element is formed by the same instructions on the same operands whatever the run length.
// (S35_TC = 3 c2 frames per step, S35_MAX_RUN: qv_limits.h)
#define S35_ROWS (2 * S35_TC * 20)                  // new c1 rows per step (of a 128-row GEMM tile)
#define S35_PITCH 260                               // halves per c1p row of the LDS tile (520 bytes: 32 rows x 8-byte stores touch every bank pair once)
#define S35_A_BYTES (128 * 256 * 2)                 // the A tile
#define S35_HALO (S35_ROWS * S35_PITCH)             // halves: the two halo slots (20 rows each) lie behind the new rows
#define S35_LDS (S35_A_BYTES + (S35_ROWS + 40) * S35_PITCH * 2)
static_assert(S35_ROWS <= 128 && S35_LDS <= 160 * 1024, "k_sub35: one block per CU, 160 KB of LDS");
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512, 1) void k_sub35(const half_t *__restrict__ c1, int t2_max, const half_t *__restrict__ w3,
                                                  const float *__restrict__ b3, const float *__restrict__ w5,
                                                  const float *__restrict__ b5, const int32_t *__restrict__ len2,
                                                  const int32_t *__restrict__ len3, const int32_t *__restrict__ row_off,
                                                  half_t *__restrict__ out, int32_t *__restrict__ row_map, int run) {
    extern __shared__ __attribute__((aligned(256))) unsigned char s35[];
    unsigned char *const sA = s35;
    half_t *const tile = (half_t *)(s35 + S35_A_BYTES);
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int l2 = len2[b], l3 = len3[b], ob = row_off[b];
    const int t3_first = blockIdx.y * run * S35_TC;
    if (t3_first >= l3) return;                     // (block-uniform) the run lies in the utterance's padding
    const int t3_end = l3 < t3_first + run * S35_TC ? l3 : t3_first + run * S35_TC;
    const int nsteps = (t3_end - t3_first + S35_TC - 1) / S35_TC;

    // ---- conv.3's weights and bias of the wave's 32 channels; conv.5's of the thread's 4
    half8 wf[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) wf[ks] = *(const half8 *)(w3 + (size_t)(wave * 32 + l31) * QV_SUBC + ks * 16 + hi * 8);
    f32x4 bq[4];    // accumulator register r is channel 32 wave + 8 (r >> 2) + 4 hi + (r & 3)
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[q] = *(const f32x4 *)(b3 + wave * 32 + 8 * q + 4 * hi);
    const int c4 = lane * 4;
    float w[9][4], bs[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const f32x4 v = *(const f32x4 *)(w5 + k * QV_SUBC + c4);
#pragma unroll
        for (int c = 0; c < 4; ++c) w[k][c] = v[c];
    }
    {
        const f32x4 v = *(const f32x4 *)(b5 + c4);
#pragma unroll
        for (int c = 0; c < 4; ++c) bs[c] = v[c];
    }

    // ---- staging: piece (g, kt) of this thread = tile row 16 wave + 8 g + (lane >> 3), 16-byte chunk lane & 7 of K-tile kt
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(c1 + (size_t)b * t2_max * 20 * QV_SUBC), 0,
                                                                        t2_max * 20 * QV_SUBC * 2, 0x00020000);
    u32x4_t ra[8];
    int dstA[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int row = wave * 16 + g * 8 + (lane >> 3), c = lane & 7;
        dstA[g] = row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
    }
    auto fetch = [&](int row0) {    // the 128 c1 rows from row0 (>= 0) of the utterance on
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int voff = (row0 + wave * 16 + g * 8 + (lane >> 3)) * (QV_SUBC * 2) + (lane & 7) * 16;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) ra[g * 4 + kt] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, kt * 128, 0);
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) *(u32x4_t *)(sA + kt * (128 * 128) + dstA[g]) = ra[g * 4 + kt];
    };
    // ---- products of tile rows 64 fp .. 64 fp + 63, ReLU, f16.  Row R < n_rows goes to dst + R * pitch; a row of the
    // step's last frame also to the halo slot `halo_w` (nullptr: none)
    auto mm_pair = [&](int fp, half_t *dst, int n_rows, half_t *halo_w) {
        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int c = (ks & 3) * 2 + hi;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = fp * 64 + i * 32 + l31;
                const half8 af = *(const half8 *)(sA + (ks >> 2) * (128 * 128) + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], af, acc[i], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int R = fp * 64 + i * 32 + l31;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = acc[i][q * 4 + e] + bq[q][e];
                    x = x > 0.f ? x : 0.f;
                    o[e] = (half_t)x;
                }
                const int col = wave * 32 + 8 * q + 4 * hi;
                if (R < n_rows) *(half4 *)(dst + R * S35_PITCH + col) = o;
                if (halo_w && R >= S35_ROWS - 20 && R < S35_ROWS) *(half4 *)(halo_w + (R - (S35_ROWS - 20)) * S35_PITCH + col) = o;
            }
        }
    };

    const int row_first = 2 * t3_first * 20;        // first new c1 row of the run
    if (t3_first > 0) {
        // the frame in front of the run -> halo slot 0
        fetch(row_first - 20);
        put();
        __syncthreads();
        fetch(row_first);
        mm_pair(0, tile + S35_HALO, 20, nullptr);
        __syncthreads();
    } else {
        fetch(row_first);   // (frame -1 does not exist: the taps on it are dropped)
    }
    for (int k = 0; k < nsteps; ++k) {
        half_t *const halo_r = tile + S35_HALO + (k & 1) * 20 * S35_PITCH;
        half_t *const halo_w = tile + S35_HALO + ((k + 1) & 1) * 20 * S35_PITCH;
        put();
        __syncthreads();        // the step's rows are in LDS; the depthwise stage of the step before has left the tile
        if (k + 1 < nsteps) fetch(row_first + (k + 1) * S35_ROWS);
        mm_pair(0, tile, S35_ROWS, nullptr);
        mm_pair(1, tile, S35_ROWS, halo_w);
        __syncthreads();        // the tile is complete; the A tile is free
        // ---- depthwise 3x3 stride 2 over the tile
        const int t3_0 = t3_first + k * S35_TC;
        if (tid < S35_TC && t3_0 + tid < l3) row_map[ob + t3_0 + tid] = (b << 16) | (t3_0 + tid);
#pragma unroll
        for (int i = 0; i < (S35_TC * 10 + 7) / 8; ++i) {
            const int p_raw = wave + 8 * i, p = p_raw < S35_TC * 10 ? p_raw : S35_TC * 10 - 1;
            const int tl = p / 10, fo = p - tl * 10, t3 = t3_0 + tl;
            const bool edge = fo == 0, skip0 = t3 == 0, skip2 = 2 * t3 + 1 >= l2;
            const half_t *rb[3];
            rb[0] = (tl == 0 ? halo_r : tile + (2 * tl - 1) * 20 * S35_PITCH) + c4;
            rb[1] = tile + (2 * tl) * 20 * S35_PITCH + c4;
            rb[2] = tile + (2 * tl + 1) * 20 * S35_PITCH + c4;
            half4 v[3][3];
#pragma unroll
            for (int dt = 0; dt < 3; ++dt)
#pragma unroll
                for (int df = 0; df < 3; ++df)
                    v[dt][df] = *(const half4 *)(rb[dt] + (2 * fo - 1 + (df == 0 && edge ? 1 : df)) * S35_PITCH);
            float acc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = bs[c];
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) {
                float a[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) a[c] = acc[c];
#pragma unroll
                for (int df = 0; df < 3; ++df)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float x = __builtin_fmaf(w[dt * 3 + df][c], (float)v[dt][df][c], a[c]);
                        a[c] = (df == 0 && edge) ? a[c] : x;
                    }
                const bool skip = dt == 0 ? skip0 : dt == 2 ? skip2 : false;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = skip ? acc[c] : a[c];
            }
            half4 h;
#pragma unroll
            for (int c = 0; c < 4; ++c) h[c] = (half_t)acc[c];
            if (p_raw < S35_TC * 10 && t3 < l3) *(half4 *)(out + ((size_t)(ob + t3) * 10 + fo) * QV_SUBC + c4) = h;
        }
    }
}

// packed rows (or, row_off == nullptr, dense f16 rows) -> the dense f32 view [B][t_max][row_elems] of a debug tap (frames
// >= len[b] are left alone: the caller zeroed them)
__global__ void k_unpack_rows_f32(const half_t *__restrict__ x, int t_max, int row_elems, const int32_t *__restrict__ len,
                                  const int32_t *__restrict__ row_off, float *__restrict__ y) {
    const int b = blockIdx.z, t = blockIdx.y;
    if (t >= len[b]) return;
    const half_t *p = x + (row_off ? (size_t)row_off[b] + t : (size_t)b * t_max + t) * row_elems;
    float *q = y + ((size_t)b * t_max + t) * row_elems;
    for (int i = threadIdx.x; i < row_elems; i += blockDim.x) q[i] = (float)p[i];
}

}  // namespace

// ====================================================================== launchers ======

// stats: [batch][80][2] results, followed by room for the [batch][MS_CHUNKS][80][2] partial sums (qv_melstats_doubles)
size_t qv_melstats_doubles(size_t max_batch) { return max_batch * 2 * QV_NMEL * (1 + MS_CHUNKS); }

void launch_logmel(const float *audio, int64_t n_max, const int32_t *n_samples, const FrontendTab &ft, float *feats,
                   int tm_max, double *stats, int batch, hipStream_t s, const QvSwitches &sw) {
    double *part = stats + (size_t)batch * 2 * QV_NMEL;
    const int variant = sw[QV_KV_LOGMEL];
    if (variant == 2)
        hipLaunchKernelGGL(lmv::k_logmel_run<QV_LOGMEL_RUN>, dim3((tm_max + 4 * QV_LOGMEL_RUN - 1) / (4 * QV_LOGMEL_RUN), batch), dim3(256), 0, s, audio, n_max, n_samples, ft, feats, tm_max);
    else if (variant == 1)
        hipLaunchKernelGGL(lmv::k_logmel_reg<0>, dim3((tm_max + 3) / 4, batch), dim3(256), 0, s, audio, n_max, n_samples, ft, feats, tm_max);
    else
        hipLaunchKernelGGL(k_logmel, dim3((tm_max + 3) / 4, batch), dim3(256), 0, s, audio, n_max, n_samples, ft, feats, tm_max);
    hipLaunchKernelGGL(k_melstats, dim3(MS_CHUNKS, batch), dim3(320), 0, s, feats, n_samples, tm_max, part);
    hipLaunchKernelGGL(k_melstats_sum, dim3(batch), dim3(2 * QV_NMEL), 0, s, part, stats);
}

void launch_melapply(const float *feats, const int32_t *n_samples, int tm_max, const double *stats, float *out, int batch,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_melapply, dim3(64, batch), dim3(320), 0, s, feats, n_samples, tm_max, stats, out);
}

void launch_conv0(const float *feats, int tm_max, const int32_t *len_in, const double *stats, const float *w,
                  const float *bias, half_t *out, int t1_max, int batch, hipStream_t s) {
    hipLaunchKernelGGL(k_conv0, dim3(1, t1_max, batch), dim3(256), 0, s, feats, tm_max, len_in, stats, w, bias, out, t1_max);
}

int qv_sub01_run_tiles(int batch, int t2_max, const QvSwitches &sw) { return sub01_run_tiles(batch, t2_max, sw); }

void launch_sub01(const float *feats, int tm_max, const int32_t *len_mel, const double *stats, const float *w0,
                  const float *b0, const int32_t *len1, const float *w1, const float *b1, half_t *out, int t2_max, int batch,
                  hipStream_t s, const QvSwitches &sw) {
    const int n_tiles = (t2_max + SUB_TT - 1) / SUB_TT, run = sub01_run_tiles(batch, t2_max, sw);
    const dim3 grid(1, (n_tiles + run - 1) / run, batch);
    if (run <= SUB_RES_RUN)
        hipLaunchKernelGGL(k_sub01<true>, grid, dim3(256), 0, s, feats, tm_max, len_mel, stats, w0, b0, len1, w1, b1, out, t2_max, run);
    else
        hipLaunchKernelGGL(k_sub01<false>, grid, dim3(256), 0, s, feats, tm_max, len_mel, stats, w0, b0, len1, w1, b1, out, t2_max, run);
}

void launch_dwconv2d(const half_t *in, int tin_max, int fin, const int32_t *len_in, const float *w, const float *bias,
                     half_t *out, int tout_max, int fout, int batch, hipStream_t s) {
    hipLaunchKernelGGL(k_dwconv2d, dim3(1, (tout_max + DW2_TT - 1) / DW2_TT, batch), dim3(256), 0, s, in, tin_max, fin, len_in, w,
                       bias, out, tout_max, fout);
}

void launch_pack_rows(const half_t *x, int t_max, int row_elems, const int32_t *len, const int32_t *row_off, half_t *y,
                      int32_t *row_map, int batch, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_rows, dim3(1, t_max, batch), dim3(256), 0, s, x, t_max, row_elems, len, row_off, y, row_map);
}

int qv_sub35_run_frames(int batch, int t3_max, const QvSwitches &sw) { return sub35_run_steps(batch, t3_max, sw) * S35_TC; }

// 145 KB of dynamic LDS: opted into once, outside any stream capture (qv_model_create calls this; launch_sub35 for the tools)
void qv_sub35_init() {
    static const int once = [] {
        (void)hipFuncSetAttribute((const void *)k_sub35, hipFuncAttributeMaxDynamicSharedMemorySize, S35_LDS);
        return 0;
    }();
    (void)once;
}

void launch_sub35(const half_t *c1, int t2_max, const half_t *w3, const float *b3, const float *w5, const float *b5,
                  const int32_t *len2, const int32_t *len3, const int32_t *row_off, half_t *out, int32_t *row_map, int t3_max,
                  int batch, hipStream_t s, const QvSwitches &sw) {
    qv_sub35_init();
    const int n_steps = (t3_max + S35_TC - 1) / S35_TC, run = sub35_run_steps(batch, t3_max, sw);
    hipLaunchKernelGGL(k_sub35, dim3(1, (n_steps + run - 1) / run, batch), dim3(512), S35_LDS, s, c1, t2_max, w3, b3, w5, b5, len2,
                       len3, row_off, out, row_map, run);
}

void launch_unpack_rows_f32(const half_t *x, int t_max, int row_elems, const int32_t *len, const int32_t *row_off, float *y,
                            int batch, hipStream_t s) {
    hipLaunchKernelGGL(k_unpack_rows_f32, dim3(1, t_max, batch), dim3(256), 0, s, x, t_max, row_elems, len, row_off, y);
}

