// qv_long.hip -- transcription with confidence of recordings longer than the engine's capacity (include/qverse.h:
// qv_transcribe_long, qv_transcribe_windows; the cutting rule: qv_long_plan.h).
//
// The recording is cut into overlapping windows the engine accepts; the existing forward runs over rounds of at most max_batch
// windows into the context's log-prob workspace; of every window only the frames it OWNS are looked at again:
//   k_long_gather    the windows of one round out of the caller's [R, pitch] audio into a [round, window_samples] batch,
//                    zero-filled behind a short last window (16-byte loads and stores; HBM-bound);
//   k_long_frames    one wave per owned frame: frame_argmax (qv_greedy.h), as k_transcribe; fid / m go to the
//                    frame's GLOBAL index in per-recording arrays in HBM (before the next round reuses the workspace);
//   k_long_collapse  once per call, one workgroup per recording: runs of equal fid over [0, T), seams included, one token per
//                    non-blank run (run_collapse, qv_greedy.h), the sums in the header's order.  Sixteen waves take a slab each; a wave first reduces
//                    its slab to (latest run start, running maximum, token count, blank count), then scans it again with what
//                    the slabs before it carry in.  The run operator is associative: no bit depends on the partition.
#include "qv_greedy.h"
#include "qv_long_plan.h"
#include "qv_rows.h"

#include <algorithm>

static_assert(QV_LONG_FRAME_CAP == QV_LONG_MAX_FRAMES, "qv_long_plan.h and qverse.h disagree");
static_assert(sizeof(qv_long_info) == 48, "record layout");

namespace {

typedef QvLongWin LongWin;   // one window of the call (qv_common.h)
static_assert(sizeof(LongWin) == 32, "plan table layout");
typedef QvLongRec LongRec;

#define LG_THREADS 256
// grid: (ceil(window_samples / 4 / LG_THREADS), windows of the round).  vec: every window start is 16-byte aligned.
__global__ __launch_bounds__(LG_THREADS) void k_long_gather(const float *__restrict__ audio, const LongWin *__restrict__ tab,
                                                           float *__restrict__ out, int window_samples, int vec) {
    const LongWin w = tab[blockIdx.y];
    const int i = (blockIdx.x * LG_THREADS + threadIdx.x) * 4;
    if (i >= window_samples) return;          // (window_samples % 4 == 0: a float4 never straddles the row's end)
    const float *src = audio + w.src_off;
    float4 v;
    if (vec && i + 4 <= w.len) v = *(const float4 *)(src + i);
    else {
        v.x = i < w.len ? src[i] : 0.f;
        v.y = i + 1 < w.len ? src[i + 1] : 0.f;
        v.z = i + 2 < w.len ? src[i + 2] : 0.f;
        v.w = i + 3 < w.len ? src[i + 3] : 0.f;
    }
    *(float4 *)(out + (size_t)blockIdx.y * window_samples + i) = v;
}

#define LF_WAVES 4
// grid: (ceil(most owned frames of a window / LF_WAVES), windows).  lp: f32[*, t_max, 1025].
__global__ __launch_bounds__(64 * LF_WAVES) void k_long_frames(const float *__restrict__ lp, int t_max, const LongWin *__restrict__ tab,
                                                              int16_t *__restrict__ fid, float *__restrict__ m) {
    const LongWin w = tab[blockIdx.y];
    const int lane = threadIdx.x & 63, f = blockIdx.x * LF_WAVES + (threadIdx.x >> 6);
    if (f >= w.count) return;
    float best;
    int bi;
    frame_argmax(lp + ((size_t)w.lp_win * t_max + (w.j0 + f)) * QV_VOCAB, lane, best, bi);
    if (lane == 0) { fid[w.dst + f] = (int16_t)bi; m[w.dst + f] = best; }
}

#define LC_WAVES 16

// a token of run_collapse into the recording's record in HBM (int32 positions)
struct LongSink {
    int32_t *ids;
    float *logp;
    int32_t *first, *last;
    __device__ __forceinline__ void operator()(int k, int id, int f, int t, float mx) const {
        ids[k] = id;
        first[k] = f;
        last[k] = t;
        logp[k] = mx;
    }
};

// record of recording r: qv_long_info, then ids i32[P], logp f32[P], first i32[P], last i32[P]
__global__ __launch_bounds__(64 * LC_WAVES) void k_long_collapse(const int16_t *__restrict__ fid_all, const float *__restrict__ m_all,
                                                                const LongRec *__restrict__ recs, unsigned char *out, int P) {
    __shared__ int s_first[LC_WAVES], s_ntok[LC_WAVES], s_nblank[LC_WAVES];
    __shared__ float s_max[LC_WAVES];
    __shared__ double s_sum[2];
    __shared__ float s_min;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LongRec rec_in = recs[r];
    int T = rec_in.t_frames;
    T = T < 0 ? 0 : (T > P ? P : T);
    const int16_t *fid = fid_all + (size_t)r * P;
    const float *m = m_all + (size_t)r * P;
    unsigned char *rec = out + (size_t)r * (sizeof(qv_long_info) + (size_t)P * 16);
    int32_t *o_ids = (int32_t *)(rec + sizeof(qv_long_info));
    float *o_logp = (float *)(o_ids + P);
    int32_t *o_first = (int32_t *)(o_logp + P), *o_last = o_first + P;

    const int chunks = (T + 63) / 64, per = (chunks + LC_WAVES - 1) / LC_WAVES;
    const int base0 = wave * per * 64 < T ? wave * per * 64 : T, base1 = (wave + 1) * per * 64 < T ? (wave + 1) * per * 64 : T;
    {   // pass 1: the slab on its own
        int n_tok = 0, n_blank = 0, c_first = -1;
        float c_max = -INFINITY;
        run_collapse<false>(fid, m, T, base0, base1, lane, n_tok, n_blank, c_first, c_max, LongSink{});
        if (lane == 0) { s_first[wave] = c_first; s_max[wave] = c_max; s_ntok[wave] = n_tok; s_nblank[wave] = n_blank; }
    }
    __syncthreads();
    // pass 2: what the slabs before this one carry in, then the slab again, emitting
    int n_tok = 0, n_blank = 0, c_first = -1;
    float c_max = -INFINITY;
    for (int s = 0; s < wave; ++s) {
        n_tok += s_ntok[s];
        if (s_first[s] >= 0) { c_first = s_first[s]; c_max = s_max[s]; }
        else c_max = s_max[s] > c_max ? s_max[s] : c_max;      // the later slab replaces only when strictly greater
    }
    run_collapse<true>(fid, m, T, base0, base1, lane, n_tok, n_blank, c_first, c_max, LongSink{o_ids, o_logp, o_first, o_last});
    int tok_all = 0, blank_all = 0;
    for (int s = 0; s < LC_WAVES; ++s) { tok_all += s_ntok[s]; blank_all += s_nblank[s]; }
    for (int i = tok_all + tid; i < P; i += 64 * LC_WAVES) { o_ids[i] = -1; o_first[i] = -1; o_last[i] = -1; o_logp[i] = 0.f; }
    // o_logp: written to HBM by every wave, read below by waves 1 and 2 -- released to the device's L2 before the barrier,
    // this CU's vector cache dropped behind it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (wave == 0) {
        const double s = lane_sum(m, T, lane);
        if (lane == 0) s_sum[0] = s;
    } else if (wave == 1) {
        const double s = lane_sum(o_logp, tok_all, lane);
        if (lane == 0) s_sum[1] = s;
    } else if (wave == 2) {
        const float mn = wave_first_min(o_logp, tok_all, lane);
        if (lane == 0) s_min = mn;
    }
    __syncthreads();
    if (tid == 0) {
        qv_long_info inf;
        inf.n_tokens = tok_all;
        inf.t_frames = T;
        inf.n_blank_frames = blank_all;
        inf.flags = tok_all == 0 ? QV_FLAG_EMPTY_TRANSCRIPT : 0;
        inf.n_windows = rec_in.n_windows;
        inf.reserved = 0;
        inf.min_token_logprob = tok_all ? s_min : 0.f;
        inf.reserved_f = 0.f;
        inf.avg_logprob = tok_all ? __ddiv_rn(s_sum[1], (double)tok_all) : 0.0;
        inf.frame_avg_logprob = T ? __ddiv_rn(s_sum[0], (double)T) : 0.0;
        *(qv_long_info *)rec = inf;
    }
}

}  // namespace

void qv_long_free(QvLongWs &w) {
    qv_mirror_free(w.m);
    if (w.batch) (void)hipFree(w.batch);
    w = {};
}

// The long workspace of the engine, allocated or grown by the first call that needs it: the plan tables going up (windows,
// recordings), per recording fid / m and one record coming back, in device memory; the tables and the records once more in a
// pinned mirror; with a model, the [max_batch, window_samples] batch the windows of a round are gathered into.
static int long_ws(qv_engine *eng, QvLongWs &w, size_t n_win, int rows, int P, size_t batch_floats) {
    const size_t tab = qv_up16(n_win * sizeof(LongWin)), recs = qv_up16((size_t)rows * sizeof(LongRec));
    const size_t out = (size_t)rows * (sizeof(qv_long_info) + (size_t)P * 16);
    const size_t fid = qv_up16((size_t)rows * P * sizeof(int16_t)), m = qv_up16((size_t)rows * P * sizeof(float));
    const size_t dev_bytes = tab + recs + out + fid + m, host_bytes = tab + recs + out;
    w.tab_bytes = tab; w.rec_bytes = recs; w.out_bytes = out; w.fid_bytes = fid;
    if (dev_bytes > w.m.dev_bytes || host_bytes > w.m.host_bytes) {
        qv_mirror_free(w.m);
        QV_TRY_RC(qv_mirror_alloc(eng, w.m, dev_bytes, host_bytes, "long transcription workspace"));
    }
    if (batch_floats > w.batch_cap) {
        if (w.batch) (void)hipFree(w.batch);
        w.batch = nullptr;
        w.batch_cap = 0;
        QV_HIP(hipMalloc((void **)&w.batch, batch_floats * sizeof(float)));
        w.batch_cap = batch_floats;
    }
    return QV_OK;
}


int qv_long_check(qv_engine *eng, const char *who_c, QvCtx &c, const float *audio, int64_t audio_pitch, int t_max_in,
                  const int64_t *n_host, int rows, int window_samples, int margin_frames, QvLongCall &call) {
    const std::string who = who_c;
    if (rows > c.work.max_batch) { qv_set_error(eng, who + ": rows exceed engine capacity"); return QV_ERR_CAPACITY; }
    call.plans.assign(rows, QvLongPlan{});
    call.n_win = 0;
    call.t_top = 0;
    for (int r = 0; r < rows; ++r) {
        const int rc = qv_long_plan_make(n_host[r], eng->cfg.max_samples, window_samples, margin_frames, &call.plans[r]);
        if (rc == QV_LONG_TOO_LONG) { qv_set_error(eng, who + ": recording longer than QV_LONG_MAX_FRAMES frames"); return QV_ERR_CAPACITY; }
        if (rc) { qv_set_error(eng, who + ": bad length, window_samples (a multiple of 1280, at most max_samples) or margin_frames (window - 2 margins >= 1 frame)"); return QV_ERR_ARG; }
        if (audio && n_host[r] > audio_pitch) { qv_set_error(eng, who + ": a recording is longer than audio_pitch"); return QV_ERR_ARG; }
        if (audio && n_host[r] < QV_LONG_MIN_SAMPLES) { qv_set_error(eng, "utterance length out of range (need 400 <= n)"); return QV_ERR_CAPACITY; }
        call.n_win += call.plans[r].n_windows;
        call.t_top = std::max(call.t_top, call.plans[r].t_total);
    }
    call.kw = call.plans[0].kw;
    call.wn = call.kw * QV_LONG_HOP;
    call.P = (call.t_top + 3) & ~3;
    if (!audio && t_max_in < call.kw + 1) { qv_set_error(eng, who + ": t_max smaller than a window's frame count"); return QV_ERR_ARG; }
    if (call.n_win > (size_t)INT32_MAX) { qv_set_error(eng, who + ": too many windows"); return QV_ERR_CAPACITY; }
    return QV_OK;
}

// the long workspace for this call (call.P entries per record; 0 = a caller without fid / m / records), its tables filled
// and on their way up
int qv_long_tables(qv_engine *eng, QvCtx &c, bool audio, int64_t audio_pitch, int rows, QvLongCall &call, hipStream_t stream) {
    const int max_batch = c.work.max_batch, P = call.P;
    QvLongWs &w = eng->long_ws;
    QV_TRY_RC(long_ws(eng, w, call.n_win, rows, P, audio ? (size_t)max_batch * call.wn : 0));
    LongWin *tab_h = (LongWin *)w.m.host;
    LongRec *rec_h = (LongRec *)(w.m.host + w.tab_bytes);
    call.tab_d = (const LongWin *)w.m.dev;
    call.rec_d = (const LongRec *)(w.m.dev + w.tab_bytes);
    call.fwd_len.assign(audio ? call.n_win : 0, 0);
    size_t k = 0;
    for (int r = 0; r < rows; ++r) {
        const QvLongPlan &p = call.plans[r];
        rec_h[r].t_frames = p.t_total;
        rec_h[r].n_windows = p.n_windows;
        for (int v = 0; v < p.n_windows; ++v, ++k) {
            LongWin &t = tab_h[k];
            const int lo = qv_long_lo(p, v), hi = qv_long_hi(p, v);
            t.src_off = (int64_t)r * audio_pitch + qv_long_start(p, v);
            t.dst = (int64_t)r * P + lo;
            t.len = qv_long_len(p, v);
            t.lp_win = audio ? (int32_t)(k % (size_t)max_batch) : (int32_t)k;
            t.j0 = lo - v * p.h;
            t.count = hi - lo;
            if (audio) call.fwd_len[k] = qv_long_fwd_len(p, v);
        }
    }
    QV_HIP(hipMemcpyAsync(w.m.dev, w.m.host, w.tab_bytes + w.rec_bytes, hipMemcpyHostToDevice, stream));
    return QV_OK;
}

int qv_long_rounds(qv_engine *eng, QvCtx &c, const QvLongCall &call, const float *audio, int64_t audio_pitch, const float *lp_in,
                   int t_max_in, hipStream_t stream, QvLongTimer *tm,
                   const std::function<int(const float *lp, int t_max, size_t k0, int nb)> &per_round) {
    const int max_batch = c.work.max_batch, wn = call.wn;
    QvLongWs &w = eng->long_ws;
    const size_t n_win = call.n_win;
    if (audio) {
        const bool vec = ((uintptr_t)audio & 15) == 0 && audio_pitch % 4 == 0;
        std::vector<int32_t> t_out(max_batch);
        for (size_t k0 = 0; k0 < n_win; k0 += max_batch) {
            const int nb = (int)std::min<size_t>(max_batch, n_win - k0);
            int64_t lmax = 0;
            for (int b = 0; b < nb; ++b) lmax = std::max(lmax, call.fwd_len[k0 + b]);
            const int t_max = qv_long_frames(lmax);
            if (tm) tm->mark(0);
            hipLaunchKernelGGL(k_long_gather, dim3((wn / 4 + LG_THREADS - 1) / LG_THREADS, nb), dim3(LG_THREADS), 0, stream, audio,
                               call.tab_d + k0, w.batch, wn, (int)vec);
            QV_HIP(hipGetLastError());
            if (tm) tm->mark(0);
            QV_TRY_RC(qv_model_forward(eng, eng->model, eng->cur_ctx, w.batch, call.fwd_len.data() + k0, nb, wn, c.logprobs_ws, t_max,
                                       t_out.data(), stream, /*zero_pad_rows=*/false));
            QV_TRY_RC(per_round((const float *)c.logprobs_ws, t_max, k0, nb));
        }
    } else {
        for (size_t k0 = 0; k0 < n_win; k0 += 32768) {
            const int nb = (int)std::min<size_t>(32768, n_win - k0);
            QV_TRY_RC(per_round(lp_in, t_max_in, k0, nb));
        }
    }
    return QV_OK;
}

// audio != nullptr: cut, forward and collapse (qv_transcribe_long).  audio == nullptr: the caller's window log-probs
// lp_in f32[*, t_max_in, 1025] (qv_transcribe_windows).  Everything is checked before the first launch and before an output
// array is written.  SYNCHRONOUS on `stream`.
int qv_long_run(qv_engine *eng, QvCtx &c, const float *audio, int64_t audio_pitch, const float *lp_in, int t_max_in,
                const int64_t *n_host, int rows, int window_samples, int margin_frames, qv_long_info *info_host, int32_t *ids_host,
                float *logp_host, int32_t *first_host, int32_t *last_host, int pitch, hipStream_t stream) {
    const char *who = audio ? "qv_transcribe_long" : "qv_transcribe_windows";
    QvLongCall call;
    QV_TRY_RC(qv_long_check(eng, who, c, audio, audio_pitch, t_max_in, n_host, rows, window_samples, margin_frames, call));
    const int t_top = call.t_top, P = call.P;
    if (pitch < t_top) { qv_set_error(eng, std::string(who) + ": pitch smaller than the longest recording's frame count"); return QV_ERR_ARG; }
    QV_TRY_RC(qv_long_tables(eng, c, audio != nullptr, audio_pitch, rows, call, stream));
    QvLongWs &w = eng->long_ws;
    unsigned char *out_d = w.m.dev + w.tab_bytes + w.rec_bytes, *out_h = w.m.host + w.tab_bytes + w.rec_bytes;
    int16_t *fid_d = (int16_t *)(out_d + w.out_bytes);
    float *m_d = (float *)((unsigned char *)fid_d + w.fid_bytes);

    QvLongTimer tm = {eng->profile_stages, stream, {}};
    const int most_owned = call.kw + 1;   // grid of k_long_frames: a wave whose frame its window does not own leaves at once
    QV_TRY_RC(qv_long_rounds(eng, c, call, audio, audio_pitch, lp_in, t_max_in, stream, &tm, [&](const float *lp, int t_max, size_t k0, int nb) -> int {
        tm.mark(1);
        hipLaunchKernelGGL(k_long_frames, dim3((most_owned + LF_WAVES - 1) / LF_WAVES, nb), dim3(64 * LF_WAVES), 0, stream, lp, t_max,
                           call.tab_d + k0, fid_d, m_d);
        QV_HIP(hipGetLastError());
        tm.mark(1);
        return QV_OK;
    }));
    tm.mark(2);
    hipLaunchKernelGGL(k_long_collapse, dim3(rows), dim3(64 * LC_WAVES), 0, stream, (const int16_t *)fid_d, (const float *)m_d, call.rec_d, out_d, P);
    QV_HIP(hipGetLastError());
    tm.mark(2);
    QV_TRY_RC(qv_fetch_sync(eng, out_h, out_d, w.out_bytes, stream));
    tm.finish(w.kernel_ms);
    const size_t row = sizeof(qv_long_info) + (size_t)P * 16;
    for (int r = 0; r < rows; ++r) {
        const unsigned char *rec = out_h + row * r;
        const int32_t *r_ids = (const int32_t *)(rec + sizeof(qv_long_info));
        const float *r_logp = (const float *)(r_ids + P);
        const int32_t *r_first = (const int32_t *)(r_logp + P), *r_last = r_first + P;
        memcpy(&info_host[r], rec, sizeof(qv_long_info));
        scatter_column(ids_host, pitch, r, r_ids, t_top, (int32_t)-1);
        scatter_column(logp_host, pitch, r, r_logp, t_top, 0.f);
        scatter_column(first_host, pitch, r, r_first, t_top, (int32_t)-1);
        scatter_column(last_host, pitch, r, r_last, t_top, (int32_t)-1);
    }
    return QV_OK;
}
