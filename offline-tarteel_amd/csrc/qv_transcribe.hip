// qv_transcribe.hip -- greedy transcription with confidence, from log-probs already in HBM (include/qverse.h:
// qv_transcribe, qv_transcribe_batch).
//
// What the reference's streaming gate asks of its transcriber is {"text", "avg_logprob"} (shared/streaming.py:158-181).
// k_decode already takes the per-frame argmax, but it belongs to a context's retrieval state and throws the maxima away;
// k_transcribe keeps them.  One workgroup per utterance:
//   all sixteen waves: per-frame argmax with numpy semantics (first maximum) -- k_decode's loop, instruction for instruction,
//                      plus the maximum itself; frame ids and maxima stay in LDS;
//   wave 0 alone:      runs of equal frame ids (segmented scan over 64 frames at a time, carried across chunks), one token
//                      per non-blank run with its first / last frame and the run's maximum, then the two float64 sums in
//                      the fixed order the header documents.
// Every float that is reported is either a value of the input or the result of a documented sequence of IEEE operations
// (explicit _rn intrinsics, no contraction), so a batch is reproducible bit for bit.
#include "qv_common.h"

#include <string.h>

namespace {

#define TR_WAVES 16
#define TR_TCAP 770   // >= t_cap of any engine (qv_create refuses more than 768 + 2 frames)

// sum of x[0 .. n) as the header defines it: lane l adds x[l], x[l + 64], ... in ascending order from +0.0, then the 64
// partials are combined by p[l] += p[l ^ o], o = 32 .. 1 (addition commutes: every lane ends with the same bits)
__device__ __forceinline__ double tr_sum(const float *x, int n, int lane) {
    double p = 0.0;
    for (int i = lane; i < n; i += 64) p = __dadd_rn(p, (double)x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p = __dadd_rn(p, __shfl_xor(p, o));
    return p;
}

// record of row b: qv_transcript_info, then ids i32[P], logp f32[P], first i16[P], last i16[P]  (P even: 8-byte rows)
__global__ __launch_bounds__(64 * TR_WAVES) void k_transcribe(const float *__restrict__ lp, int t_max, const int32_t *__restrict__ t_dev,
                                                             unsigned char *__restrict__ out, int P) {
    __shared__ int16_t s_fid[TR_TCAP];
    __shared__ float s_m[TR_TCAP];    // the frame's maximum, lp[t][fid[t]]
    __shared__ float s_lp[TR_TCAP];   // the tokens' log-probs
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int T = t_dev[b];
    T = T < 0 ? 0 : T;
    T = T > t_max ? t_max : T;
    T = T > TR_TCAP ? TR_TCAP : T;
    // a wave takes every 16th frame; the 17 loads of a row are all requested before the first comparison
    for (int t = wave; t < T; t += TR_WAVES) {
        const float *row = lp + ((size_t)b * t_max + t) * QV_VOCAB;
        float x[17];
#pragma unroll
        for (int i = 0; i < 17; ++i) x[i] = lane + 64 * i < QV_VOCAB ? row[lane + 64 * i] : -INFINITY;
        float best = x[0];
        int bi = lane;
#pragma unroll
        for (int i = 1; i < 17; ++i)
            if (x[i] > best) { best = x[i]; bi = lane + 64 * i; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            float b2 = __shfl_xor(best, o);
            int i2 = __shfl_xor(bi, o);
            if (b2 > best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
        }
        if (lane == 0) { s_fid[t] = (int16_t)bi; s_m[t] = best; }
    }
    __syncthreads();
    if (wave != 0) return;
    unsigned char *rec = out + (size_t)b * (sizeof(qv_transcript_info) + (size_t)P * 12);
    int32_t *o_ids = (int32_t *)(rec + sizeof(qv_transcript_info));
    float *o_logp = (float *)(o_ids + P);
    int16_t *o_first = (int16_t *)(o_logp + P), *o_last = o_first + P;

    int n_tok = 0, n_blank = 0;
    int c_first = -1;          // the run that reaches into this chunk: its first frame and its maximum so far
    float c_max = -INFINITY;
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        const bool valid = t < T;
        const int id = valid ? (int)s_fid[t] : -2;
        const int prev = valid && t > 0 ? (int)s_fid[t - 1] : -3;
        const int next = t + 1 < T ? (int)s_fid[t + 1] : -1;
        const bool start = valid && id != prev, end = valid && id != next;
        // inclusive segmented scan over the lanes: f = the latest run start at or before this frame (-1: none in this
        // chunk), mx = the FIRST maximum of m over the frames of that run seen so far (a later frame replaces an earlier
        // one only when strictly greater: the operator is associative, the bits do not depend on the scan's shape)
        int f = start ? t : -1;
        float mx = valid ? s_m[t] : -INFINITY;
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
        if (end && !blank) {
            const int k = n_tok + __popcll(ks & (~0ull >> (63 - lane))) - 1;   // starts at or before this lane
            o_ids[k] = id;
            o_first[k] = (int16_t)f;
            o_last[k] = (int16_t)t;
            o_logp[k] = mx;
            s_lp[k] = mx;
        }
        n_tok += __popcll(ks);
        c_first = __shfl(f, 63);
        c_max = __shfl(mx, 63);
    }
    for (int i = n_tok + lane; i < P; i += 64) { o_ids[i] = -1; o_first[i] = -1; o_last[i] = -1; o_logp[i] = 0.f; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // s_lp: written and read by this wave alone
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const double frame_sum = tr_sum(s_m, T, lane), tok_sum = tr_sum(s_lp, n_tok, lane);
    // the first minimum over the tokens (value, then index: -0.0 and +0.0 compare equal, the earlier token is reported)
    float mn = 0.f;
    int mi = 0x7fffffff;
    for (int i = lane; i < n_tok; i += 64) {
        const float v = s_lp[i];
        if (mi == 0x7fffffff || v < mn) { mn = v; mi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(mn, o);
        const int i2 = __shfl_xor(mi, o);
        if (i2 != 0x7fffffff && (mi == 0x7fffffff || v2 < mn || (v2 == mn && i2 < mi))) { mn = v2; mi = i2; }
    }
    if (lane == 0) {
        qv_transcript_info inf;
        inf.n_tokens = n_tok;
        inf.t_frames = T;
        inf.n_blank_frames = n_blank;
        inf.flags = n_tok == 0 ? QV_FLAG_EMPTY_TRANSCRIPT : 0;
        inf.min_token_logprob = n_tok ? mn : 0.f;
        inf.reserved_f = 0.f;
        inf.avg_logprob = n_tok ? __ddiv_rn(tok_sum, (double)n_tok) : 0.0;
        inf.frame_avg_logprob = T ? __ddiv_rn(frame_sum, (double)T) : 0.0;
        *(qv_transcript_info *)rec = inf;
    }
}

}  // namespace

static_assert(sizeof(qv_transcript_info) == 40, "record layout");

// The transcription workspace of one context, allocated by the first call that uses it: per row of max_batch the frame
// count going up and one record coming back (40 + 12 * t_cap bytes), in device memory and in a pinned mirror.
static int transcribe_ws(qv_engine *eng, QvCtx &c, QvTranscribeWs **out) {
    QvTranscribeWs &w = c.transcribe;
    *out = &w;
    if (w.dev) return QV_OK;
    const size_t B = (size_t)c.work.max_batch, P = ((size_t)c.work.t_cap + 1) & ~(size_t)1;
    w.t_bytes = (B * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t bytes = w.t_bytes + B * (sizeof(qv_transcript_info) + P * 12);
    void *d = nullptr, *h = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess || hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) {
        if (d) (void)hipFree(d);
        (void)hipGetLastError();
        qv_set_error(eng, "transcription workspace: out of memory");
        return QV_ERR_HIP;
    }
    eng->allocs.push_back(d);   // freed by qv_destroy (the pinned mirror: with the context)
    w.dev = (unsigned char *)d;
    w.host = (unsigned char *)h;
    return QV_OK;
}

// frame counts up, kernel, one copy back, scatter into the caller's arrays; SYNCHRONOUS on `stream`
int qv_transcribe_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max,
                       qv_transcript_info *info_host, int32_t *ids_host, float *logp_host, int16_t *first_host, int16_t *last_host,
                       int pitch, hipStream_t stream) {
    if (batch > c.work.max_batch) { qv_set_error(eng, "qv_transcribe: batch exceeds engine capacity"); return QV_ERR_CAPACITY; }
    if (t_max > c.work.t_cap) { qv_set_error(eng, "qv_transcribe: t_max exceeds the engine's frame capacity"); return QV_ERR_CAPACITY; }
    for (int b = 0; b < batch; ++b)
        if (t_host[b] < 0 || t_host[b] > t_max) { qv_set_error(eng, "qv_transcribe: t_host[b] outside 0..t_max"); return QV_ERR_ARG; }
    QvTranscribeWs *w = nullptr;
    int rc = transcribe_ws(eng, c, &w);
    if (rc) return rc;
    // (the previous call has finished with the mirror: transcription calls are synchronous and serialised by the engine's lock)
    const int P = (t_max + 1) & ~1;
    const size_t row = sizeof(qv_transcript_info) + (size_t)P * 12;
    memcpy(w->host, t_host, sizeof(int32_t) * batch);
    QV_HIP(hipMemcpyAsync(w->dev, w->host, sizeof(int32_t) * batch, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_transcribe, dim3(batch), dim3(64 * TR_WAVES), 0, stream, lp, t_max, (const int32_t *)w->dev, w->dev + w->t_bytes, P);
    QV_HIP(hipGetLastError());
    QV_HIP(hipMemcpyAsync(w->host + w->t_bytes, w->dev + w->t_bytes, row * batch, hipMemcpyDeviceToHost, stream));
    QV_HIP(hipStreamSynchronize(stream));
    for (int b = 0; b < batch; ++b) {
        const unsigned char *rec = w->host + w->t_bytes + row * b;
        const int32_t *r_ids = (const int32_t *)(rec + sizeof(qv_transcript_info));
        const float *r_logp = (const float *)(r_ids + P);
        const int16_t *r_first = (const int16_t *)(r_logp + P), *r_last = r_first + P;
        const size_t o = (size_t)b * pitch;
        memcpy(&info_host[b], rec, sizeof(qv_transcript_info));
        memcpy(ids_host + o, r_ids, sizeof(int32_t) * t_max);
        if (logp_host) memcpy(logp_host + o, r_logp, sizeof(float) * t_max);
        if (first_host) memcpy(first_host + o, r_first, sizeof(int16_t) * t_max);
        if (last_host) memcpy(last_host + o, r_last, sizeof(int16_t) * t_max);
        for (int i = t_max; i < pitch; ++i) {
            ids_host[o + i] = -1;
            if (logp_host) logp_host[o + i] = 0.f;
            if (first_host) first_host[o + i] = -1;
            if (last_host) last_host[o + i] = -1;
        }
    }
    return QV_OK;
}
