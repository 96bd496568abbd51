// qv_transcribe.hip -- greedy transcription with confidence, from log-probs already in HBM (include/qverse.h:
// qv_transcribe, qv_transcribe_batch).
//
// What the reference's streaming gate asks of its transcriber is {"text", "avg_logprob"} (shared/streaming.py:158-181).
// k_decode already takes the per-frame argmax, but it belongs to a context's retrieval state and throws the maxima away;
// k_transcribe keeps them.  One workgroup per utterance:
//   all sixteen waves: per-frame argmax with numpy semantics (first maximum) -- frame_argmax, as k_decode -- keeping the
//                      maximum itself; frame ids and maxima stay in LDS;
//   wave 0 alone:      runs of equal frame ids (run_collapse: a segmented scan over 64 frames at a time, carried across
//                      chunks), one token per non-blank run with its first / last frame and the run's maximum, then the
//                      two float64 sums in the fixed order the header documents (lane_sum).  All of it: qv_greedy.h.
// Every float that is reported is either a value of the input or the result of a documented sequence of IEEE operations
// (explicit _rn intrinsics, no contraction), so a batch is reproducible bit for bit.
#include "qv_greedy.h"
#include "qv_rows.h"

namespace {

#define TR_WAVES 16

// a token of run_collapse into the row's record (int16 positions) and its log-prob into LDS for the sums
struct TrSink {
    int32_t *ids;
    float *logp;
    int16_t *first, *last;
    float *s_lp;
    __device__ __forceinline__ void operator()(int k, int id, int f, int t, float mx) const {
        ids[k] = id;
        first[k] = (int16_t)f;
        last[k] = (int16_t)t;
        logp[k] = mx;
        s_lp[k] = mx;
    }
};

// record of row b: qv_transcript_info, then ids i32[P], logp f32[P], first i16[P], last i16[P]  (P even: 8-byte rows)
__global__ __launch_bounds__(64 * TR_WAVES) void k_transcribe(const float *__restrict__ lp, int t_max, const int32_t *__restrict__ t_dev,
                                                             unsigned char *__restrict__ out, int P) {
    __shared__ int16_t s_fid[QV_FRAME_CAP];
    __shared__ float s_m[QV_FRAME_CAP];    // the frame's maximum, lp[t][fid[t]]
    __shared__ float s_lp[QV_FRAME_CAP];   // the tokens' log-probs
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int T = t_dev[b];
    T = T < 0 ? 0 : T;
    T = T > t_max ? t_max : T;
    T = T > QV_FRAME_CAP ? QV_FRAME_CAP : T;
    // a wave takes every 16th frame
    for (int t = wave; t < T; t += TR_WAVES) {
        float best;
        int bi;
        frame_argmax(lp + ((size_t)b * t_max + t) * QV_VOCAB, lane, best, bi);
        if (lane == 0) { s_fid[t] = (int16_t)bi; s_m[t] = best; }
    }
    __syncthreads();
    if (wave != 0) return;
    unsigned char *rec = out + (size_t)b * (sizeof(qv_transcript_info) + (size_t)P * 12);
    int32_t *o_ids = (int32_t *)(rec + sizeof(qv_transcript_info));
    float *o_logp = (float *)(o_ids + P);
    int16_t *o_first = (int16_t *)(o_logp + P), *o_last = o_first + P;

    int n_tok = 0, n_blank = 0, c_first = -1;
    float c_max = -INFINITY;
    run_collapse<true>(s_fid, s_m, T, 0, T, lane, n_tok, n_blank, c_first, c_max, TrSink{o_ids, o_logp, o_first, o_last, s_lp});
    for (int i = n_tok + lane; i < P; i += 64) { o_ids[i] = -1; o_first[i] = -1; o_last[i] = -1; o_logp[i] = 0.f; }
    QV_WSYNC();   // s_lp: written and read by this wave alone
    const double frame_sum = lane_sum(s_m, T, lane), tok_sum = lane_sum(s_lp, n_tok, lane);
    const float mn = wave_first_min(s_lp, n_tok, lane);
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

// frame counts up, kernel, one copy back, scatter into the caller's arrays; SYNCHRONOUS on `stream`.  The workspace of the
// context, allocated by the first call that uses it: per row of max_batch the frame count going up and one record coming
// back (40 + 12 * t_cap bytes).
int qv_transcribe_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max,
                       qv_transcript_info *info_host, int32_t *ids_host, float *logp_host, int16_t *first_host, int16_t *last_host,
                       int pitch, hipStream_t stream) {
    QV_TRY_RC(qv_rows_check(eng, "qv_transcribe", c, batch, t_max, t_host));
    QvRowWs &w = c.transcribe;
    QV_TRY_RC(qv_row_ws(eng, c, w, sizeof(qv_transcript_info) + (((size_t)c.work.t_cap + 1) & ~(size_t)1) * 12, "transcription workspace"));
    const int P = (t_max + 1) & ~1;
    const size_t row = sizeof(qv_transcript_info) + (size_t)P * 12;
    QV_TRY_RC(qv_rows_send_t(eng, w, t_host, batch, stream));
    hipLaunchKernelGGL(k_transcribe, dim3(batch), dim3(64 * TR_WAVES), 0, stream, lp, t_max, (const int32_t *)w.m.dev, w.m.dev + w.t_bytes, P);
    QV_HIP(hipGetLastError());
    QV_TRY_RC(qv_fetch_sync(eng, w.m.host + w.t_bytes, w.m.dev + w.t_bytes, row * batch, stream));
    for (int b = 0; b < batch; ++b) {
        const unsigned char *rec = w.m.host + w.t_bytes + row * b;
        const int32_t *r_ids = (const int32_t *)(rec + sizeof(qv_transcript_info));
        const float *r_logp = (const float *)(r_ids + P);
        const int16_t *r_first = (const int16_t *)(r_logp + P), *r_last = r_first + P;
        memcpy(&info_host[b], rec, sizeof(qv_transcript_info));
        scatter_column(ids_host, pitch, b, r_ids, t_max, (int32_t)-1);
        scatter_column(logp_host, pitch, b, r_logp, t_max, 0.f);
        scatter_column(first_host, pitch, b, r_first, t_max, (int16_t)-1);
        scatter_column(last_host, pitch, b, r_last, t_max, (int16_t)-1);
    }
    return QV_OK;
}
