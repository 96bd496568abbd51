// qv_greedy.h -- the greedy frame path, one definition for every kernel that walks it: the per-frame argmax (k_decode in
// both compilations of qv_match_body.inc, k_transcribe, k_long_frames), the collapse of runs of equal frame ids into tokens
// (k_transcribe, k_long_collapse), the two reductions over the tokens' log-probs, and the (score desc, key asc) ordering of
// the stable top-k selections (qv_postlogits.hip, qv_nbest.hip).  No state; every float reported is a value of the input or
// the result of the IEEE operations spelled out here, so the kernels that share a helper report the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qv_limits.h"   // QV_VOCAB, QV_BLANK (through the public header)

// Hand-off between the lanes of ONE wave through LDS or global memory: the wave's own memory operations have to be complete,
// which workgroup-scope release / acquire fences around a wave barrier give -- no block barrier.
#define QV_WSYNC()                                                  \
    do {                                                            \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      \
        __builtin_amdgcn_wave_barrier();                            \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");      \
    } while (0)

// (score desc, key asc): the ordering of every stable "sorted(..., reverse=True)" emulation, under IEEE > / == on doubles
// (no bit-pattern keys: -0.0 and +0.0 tie as they do in Python)
template <typename K>
static __device__ __forceinline__ bool better(double s, K k, double s2, K k2) {
    return s > s2 || (s == s2 && k < k2);
}

// argmax of one row of QV_VOCAB log-probs over a wave, numpy semantics (the first maximum; ties go to the smaller index).
// The 17 loads of the row are all requested before the first comparison: a frame's argmax is one memory latency, not
// seventeen.  best / bi are valid in every lane.
static __device__ __forceinline__ void frame_argmax(const float *row, int lane, float &best, int &bi) {
    float x[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) x[i] = lane + 64 * i < QV_VOCAB ? row[lane + 64 * i] : -INFINITY;
    best = x[0];
    bi = lane;
#pragma unroll
    for (int i = 1; i < 17; ++i)
        if (x[i] > best) { best = x[i]; bi = lane + 64 * i; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float b2 = __shfl_xor(best, o);
        int i2 = __shfl_xor(bi, o);
        if (b2 > best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
    }
}

// Runs of equal frame ids over the frames [base0, base1) of an utterance of T frames, 64 frames at a time on one wave: one
// token per non-blank run with the run's first / last frame and the FIRST maximum of m over its frames.  Entered with the run
// that reaches into the slab (c_first: its first frame, -1 = none known; c_max: its maximum so far) and the tokens (n_tok)
// and blank frames (n_blank) counted before it; leaves the same four for the slab behind it.  The run operator is
// associative: no bit depends on how [0, T) is cut into slabs.  EMIT: sink(k, id, first, last, max) receives token k from
// the lane of the run's last frame (a struct with an inlinable operator(); EMIT = false only counts and carries).
template <bool EMIT, typename Sink>
static __device__ __forceinline__ void run_collapse(const int16_t *fid, const float *m, int T, int base0, int base1, int lane, int &n_tok,
                                                    int &n_blank, int &c_first, float &c_max, const Sink &sink) {
    for (int base = base0; base < base1; base += 64) {
        const int t = base + lane;
        const bool valid = t < T;
        const int id = valid ? (int)fid[t] : -2;
        const int prev = valid && t > 0 ? (int)fid[t - 1] : -3;
        const int next = t + 1 < T ? (int)fid[t + 1] : -1;
        const bool start = valid && id != prev, end = valid && id != next;
        // inclusive segmented scan over the lanes: f = the latest run start at or before this frame (-1: none in this
        // chunk), mx = the FIRST maximum of m over the frames of that run seen so far (a later frame replaces an earlier
        // one only when strictly greater: the operator is associative, the bits do not depend on the scan's shape)
        int f = start ? t : -1;
        float mx = valid ? m[t] : -INFINITY;
        bool fl = start;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int f2 = __shfl_up(f, o);
            const float m2 = __shfl_up(mx, o);
            const int fl2 = __shfl_up((int)fl, o);
            if (lane >= o) {
                f = f2 > f ? f2 : f;
                if (!fl) mx = mx > m2 ? mx : m2;
                fl = fl || fl2 != 0;
            }
        }
        if (!fl) { f = c_first; mx = mx > c_max ? mx : c_max; }
        const bool blank = id == QV_BLANK;
        const unsigned long long ks = __ballot(start && !blank);
        n_blank += __popcll(__ballot(valid && blank));
        if (EMIT && end && !blank) sink(n_tok + __popcll(ks & (~0ull >> (63 - lane))) - 1, id, f, t, mx);   // starts at or before this lane
        n_tok += __popcll(ks);
        c_first = __shfl(f, 63);
        c_max = __shfl(mx, 63);
    }
}

// sum of x[0 .. n) as the public header defines it: lane l adds x[l], x[l + 64], ... in ascending order from +0.0, then the
// 64 partials are combined by p[l] += p[l ^ o], o = 32 .. 1 (addition commutes: every lane ends with the same bits).  The
// additions of a lane are one dependent chain; eight loads are requested ahead of it (the order fixes the bits, not the
// prefetch).
static __device__ __forceinline__ double lane_sum(const float *x, int n, int lane) {
    double p = 0.0;
    for (int i = lane; i < n; i += 64 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i + 64 * u < n ? x[i + 64 * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i + 64 * u < n) p = __dadd_rn(p, (double)v[u]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p = __dadd_rn(p, __shfl_xor(p, o));
    return p;
}

// the first minimum of x[0 .. n) over a wave (value, then index: -0.0 and +0.0 compare equal, the earlier entry is
// reported); 0.f when n == 0.  Valid in every lane.
static __device__ __forceinline__ float wave_first_min(const float *x, int n, int lane) {
    float mn = 0.f;
    int mi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const float v = x[i];
        if (mi == 0x7fffffff || v < mn) { mn = v; mi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(mn, o);
        const int i2 = __shfl_xor(mi, o);
        if (i2 != 0x7fffffff && (mi == 0x7fffffff || v2 < mn || (v2 == mn && i2 < mi))) { mn = v2; mi = i2; }
    }
    return mn;
}
