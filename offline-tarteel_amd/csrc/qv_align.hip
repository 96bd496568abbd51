// qv_align.hip -- CTC forced alignment (Viterbi) of a token list against frame-level log-probs in HBM:
// which frames did every token of the recognised verse occupy?  (include/qverse.h: qv_align, qv_align_results_ctx)
//
// The recursion is k_ctc's (qv_postlogits.hip, ctc_wave2) with max in place of log-sum-exp: one wave per utterance,
// state s = lane * NS + k over the blank-extended target (S = 2L + 1), the previous lane's last two states handed
// over with __shfl_up, the gathers lp[t][tok] fetched TCH frames ahead.  Differences:
//   * plain float32 in natural-log units, no log2 rescale: the only float operation per state and frame is ONE add
//     (the maximum is exact), so the path score has the bits of a numpy restatement (tests/align_ref.py);
//   * ties go to the smaller step: stay beats s-1 beats s-2 (strict > when the larger step is considered);
//   * every frame leaves two bits per state (the step taken: 0, 1, 2) packed into one uint32 per lane -- one coalesced
//     256-byte row store per frame into bp[b][t][64];
//   * the same wave then walks t = T-1 .. 1 backwards.  Lane l only ever reads back the words lane l wrote, so no
//     cross-lane visibility is needed; the rows are loaded BCH frames ahead of the walk (their addresses do not
//     depend on the path) and the lane that owns the current state supplies the step through v_readlane.
#include "qv_rows.h"

namespace {

constexpr float AL_NEG = -1e30f;

// Leaves the state of every frame in path[0 .. T-1] (LDS) and returns the path score; false = no alignment exists.
template <int NS>
__device__ bool align_wave(const float *__restrict__ lp, int T, const uint16_t *__restrict__ tgt, int L, int lane,
                           uint32_t *__restrict__ bp, float *sa, int16_t *path, float *score_out) {
    constexpr bool PAR = (NS % 2) == 0;   // even NS: the parity of state lane*NS + k is the parity of k (ctc_wave2)
    const int S = 2 * L + 1;
    int tok[NS];
    bool skip_ok[NS];
    float a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = lane * NS + k;
        tok[k] = QV_BLANK;
        skip_ok[k] = false;
        if (s < S && (s & 1)) {
            tok[k] = tgt[s >> 1];
            skip_ok[k] = s > 1 && tgt[s >> 1] != tgt[(s >> 1) - 1];
        }
        a[k] = AL_NEG;
        if (s == 0) a[k] = lp[QV_BLANK];
        if (s == 1) a[k] = lp[tok[k]];
    }
    // Frames fetched ahead.  Unlike k_ctc (hundreds of leader waves per utterance, bound by how many of them a SIMD
    // interleaves) this kernel runs ONE wave per utterance, alone on its SIMD: it is bound by the latency of one round of
    // gathers per TCH frames and has the register file to itself, so it looks further ahead than ctc_wave2 does --
    // G gathers per frame (a parity-specialised lane fetches its NS / 2 token states + the one blank value), up to 64 in flight.
    constexpr int G = PAR ? NS / 2 + 1 : NS;
    constexpr int TCH = G * 16 <= 64 ? 16 : 8;
    for (int t0 = 1; t0 < T; t0 += TCH) {
        float lpv[TCH][NS], lpb[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            const int t = t0 + j < T ? t0 + j : T - 1;
            const float *row = lp + (size_t)t * QV_VOCAB;
            if (PAR) lpb[j] = row[QV_BLANK];
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if (!PAR || (k & 1)) lpv[j][k] = row[tok[k]];
        }
        // ... and really ahead: without this the compiler sinks every frame's loads into that frame's own block (the
        // `break` below splits the chunk into blocks), one full memory latency per frame instead of one per chunk
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            if (PAR) asm volatile("" : "+v"(lpb[j]));
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if (!PAR || (k & 1)) asm volatile("" : "+v"(lpv[j][k]));
        }
        // The frames' back-pointer words are collected in registers and stored after the chunk: no vector-memory operation
        // sits between two frames' updates (loads and stores share one counter, so a wait for either waits for both).
        uint32_t wv[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            wv[j] = 0;
            if (t0 + j >= T) break;
            // previous lane's last two states
            float p1 = __shfl_up(a[NS - 1], 1), p2 = NS >= 2 ? __shfl_up(a[NS - 2], 1) : __shfl_up(a[NS - 1], 2);
            if (lane == 0) { p1 = AL_NEG; p2 = AL_NEG; }
            if (NS == 1 && lane == 1) p2 = AL_NEG;
            uint32_t w = 0;
            // in place from the highest register down: a[k] needs the OLD a[k-1], a[k-2]
#pragma unroll
            for (int k = NS - 1; k >= 0; --k) {
                float best = a[k];
                uint32_t step = 0;
                const float la2 = k >= 1 ? a[k - 1] : p1;
                if (la2 > best) { best = la2; step = 1; }
                if (!(PAR && !(k & 1))) {   // blank states have no skip transition
                    float la3 = k >= 2 ? a[k - 2] : (k == 1 ? p1 : p2);
                    if (NS == 1) la3 = p2;
                    if (!skip_ok[k]) la3 = AL_NEG;
                    if (la3 > best) { best = la3; step = 2; }
                }
                // states beyond 2L never feed a lower state, so they are left unmasked
                a[k] = best + ((PAR && !(k & 1)) ? lpb[j] : lpv[j][k]);
                w |= step << (2 * k);
            }
            asm volatile("" : "+v"(w));   // the word itself stays live until the chunk's stores, not the compare masks it is made of
            wv[j] = w;
        }
#pragma unroll
        for (int j = 0; j < TCH; ++j)
            if (t0 + j < T) bp[(size_t)(t0 + j) * 64 + lane] = wv[j];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) sa[lane * NS + k] = a[k];
    __syncthreads();   // (the block is this one wave)
    const float v_last = sa[S - 1], v_prev = sa[S - 2];
    int s = v_last >= v_prev ? S - 1 : S - 2;
    const float score = v_last >= v_prev ? v_last : v_prev;
    *score_out = score;
    if (score < -1e29f) return false;
    s = __builtin_amdgcn_readfirstlane(s);
    if (lane == 0) path[T - 1] = (int16_t)s;
    // The walk is a scalar chain (state -> owner lane -> its word -> step): the state of frame t1 - 1 - j goes into lane j of
    // one register, and a chunk's states go to LDS in one store.
    constexpr int BCH = 32;
    int owner = s / NS, k = s - owner * NS;
    for (int t1 = T - 1; t1 >= 1; t1 -= BCH) {
        uint32_t w[BCH];
#pragma unroll
        for (int j = 0; j < BCH; ++j) {
            const int t = t1 - j >= 1 ? t1 - j : 1;
            w[j] = bp[(size_t)t * 64 + lane];
        }
        int pv = 0;
#pragma unroll
        for (int j = 0; j < BCH; ++j) {
            if (t1 - j < 1) break;
            const uint32_t ww = __builtin_amdgcn_readlane(w[j], owner);
            const int step = (int)((ww >> (2 * k)) & 3u);
            s -= step;
            k -= step;
            if (k < 0) { k += NS; owner -= 1; }   // a step is at most 2: NS = 1 may cross two lanes
            if (NS == 1 && k < 0) { k += NS; owner -= 1; }
            pv = lane == j ? s : pv;
        }
        if (lane < BCH && t1 - 1 - lane >= 0) path[t1 - 1 - lane] = (int16_t)pv;
    }
    return true;
}

// LONG = engine capacity above 30 s (more than 384 frames): only then are the wide instantiations compiled in (ctc_dispatch)
template <bool LONG>
__device__ bool align_dispatch(const float *lp, int T, const uint16_t *tgt, int L, int lane, uint32_t *bp, float *sa,
                               int16_t *path, float *score) {
    const int S = 2 * L + 1;
    if (S <= 64) return align_wave<1>(lp, T, tgt, L, lane, bp, sa, path, score);
    if (S <= 128) return align_wave<2>(lp, T, tgt, L, lane, bp, sa, path, score);
    if (S <= 192) return align_wave<3>(lp, T, tgt, L, lane, bp, sa, path, score);
    if (S <= 256) return align_wave<4>(lp, T, tgt, L, lane, bp, sa, path, score);
    if (S <= 384 || !LONG) return align_wave<6>(lp, T, tgt, L, lane, bp, sa, path, score);
    if (S <= 512) return align_wave<8>(lp, T, tgt, L, lane, bp, sa, path, score);
    return align_wave<12>(lp, T, tgt, L, lane, bp, sa, path, score);
}

// One wave per utterance: recursion, backtrace, per-token read-out.  Outputs have a pitch of QV_ALIGN_PITCH entries.
template <bool LONG>
__global__ __launch_bounds__(64) void k_align(const float *__restrict__ lp, int t_max, const uint16_t *__restrict__ tok_base,
                                              const QvAlignRow *__restrict__ plan, QvAlignWs ws, int t_cap) {
    constexpr int SCAP = LONG ? 768 : 384;    // states, and frames: t_cap <= 384 for the short kernel
    __shared__ float sa[SCAP];
    __shared__ int16_t path[SCAP];
    __shared__ int16_t s_first[QV_ALIGN_PITCH], s_last[QV_ALIGN_PITCH];
    const int b = blockIdx.x, lane = threadIdx.x;
    const QvAlignRow r = plan[b];
    const int L = r.L, T = r.T;
    const uint16_t *tgt = tok_base + r.tok_off;
    const float *lpb = lp + (size_t)b * t_max * QV_VOCAB;
    int flags = r.flags;
    if (!flags) {
        if (L <= 0) flags = QV_ALIGN_NO_TARGET;
        else if (L > QV_ALIGN_MAX_TOKENS || 2 * L + 1 > SCAP) flags = QV_ALIGN_TOO_LONG;
        else {
            // every token needs a frame, and two equal neighbours a blank frame between them
            int rep = 0;
            for (int i = lane + 1; i < L; i += 64) rep += tgt[i] == tgt[i - 1];
            for (int d = 32; d >= 1; d >>= 1) rep += __shfl_xor(rep, d);
            if (T < L + rep || T > SCAP || T > t_cap) flags = QV_ALIGN_INFEASIBLE;
        }
    }
    float score = 0.f;
    if (!flags && !align_dispatch<LONG>(lpb, T, tgt, L, lane, ws.bp + (size_t)b * t_cap * 64, sa, path, &score))
        flags = QV_ALIGN_INFEASIBLE;
    __syncthreads();
    if (!flags) {
        for (int t = lane; t < T; t += 64) {
            const int st = path[t];
            if (st & 1) {
                if (t == 0 || path[t - 1] != st) s_first[st >> 1] = (int16_t)t;
                if (t == T - 1 || path[t + 1] != st) s_last[st >> 1] = (int16_t)t;
            }
        }
    }
    __syncthreads();
    unsigned char *rec = ws.out + (size_t)b * QV_ALIGN_ROW_BYTES;
    float *o_logp = (float *)(rec + sizeof(qv_align_info));
    int16_t *o_first = (int16_t *)(o_logp + QV_ALIGN_PITCH), *o_last = o_first + QV_ALIGN_PITCH;
    uint16_t *o_ids = (uint16_t *)(o_last + QV_ALIGN_PITCH);
    for (int i = lane; i < QV_ALIGN_PITCH; i += 64) {
        int f = -1, l = -1;
        float mean = 0.f;
        uint16_t id = 0xFFFF;
        if (!flags && i < L) {
            f = s_first[i];
            l = s_last[i];
            id = tgt[i];
            float sum = 0.f;
#pragma unroll 4
            for (int t = f; t <= l; ++t) sum += lpb[(size_t)t * QV_VOCAB + id];
            mean = sum / (float)(l - f + 1);
        }
        o_first[i] = (int16_t)f;
        o_last[i] = (int16_t)l;
        o_logp[i] = mean;
        o_ids[i] = id;
    }
    if (lane == 0) {
        qv_align_info inf;
        inf.n_tokens = L > 0 ? L : 0;
        inf.flags = flags;
        inf.t_frames = T;
        inf.start_verse = r.start;
        inf.span = r.span;
        inf.reserved = 0;
        inf.score = flags ? 0.f : score;
        inf.reserved_f = 0.f;
        *(qv_align_info *)rec = inf;
    }
}

// The winner of every row of a context's last batch, as k_result left it on the device: the token list is the table's,
// as in k_ctc.  A row without a prediction (or whose prediction is withheld: transcript beyond the window) has no target.
__global__ void k_align_plan(QvTables tab, QvWork wk, int batch, int t_max, QvAlignRow *__restrict__ plan) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const qv_result &res = wk.results[b];
    const QvUtt &u = wk.utt[b];
    int st = -1, sp = 0;
    if (res.surah != 0 && !(res.flags & QV_FLAG_TRANSCRIPT_TRUNCATED)) {
        if (res.source == QV_SOURCE_CTC && u.win >= 0 && u.win < QV_CAND_CAP) {
            st = wk.cand_start[(size_t)b * QV_CAND_CAP + u.win];
            sp = wk.cand_span[(size_t)b * QV_CAND_CAP + u.win];
        } else if (res.source == QV_SOURCE_TEXT) {
            st = u.base_start;
            sp = u.base_span;
        }
    }
    QvAlignRow r;
    r.tok_off = 0; r.L = 0; r.flags = QV_ALIGN_NO_TARGET; r.start = -1; r.span = 0;
    r.T = u.t_frames < 0 ? 0 : (u.t_frames > t_max ? t_max : u.t_frames);
    if (st >= 0 && st < tab.n_verses && sp >= 1 && sp <= QV_MAX_SPAN) {
        const size_t k = (size_t)st * QV_MAX_SPAN + (sp - 1);
        r.tok_off = (int32_t)tab.tok_off[k];
        r.L = (int32_t)(tab.tok_off[k + 1] - tab.tok_off[k]);
        r.flags = 0;
        r.start = st;
        r.span = sp;
    }
    plan[b] = r;
}

}  // namespace

// The alignment workspace of one context, allocated on the first alignment call that uses it: an engine that never
// aligns pays nothing.  One mirror: the output records (3,872 bytes per row of max_batch), then plan and targets (792), in
// device memory and in the pinned buffer; behind them, on the device alone, the back-pointers (t_cap * 256).
static int align_ws(qv_engine *eng, QvCtx &c, QvAlignWs **out) {
    QvAlignWs &w = c.align;
    *out = &w;
    if (w.bp) return QV_OK;
    const size_t B = (size_t)c.work.max_batch, tc = (size_t)c.work.t_cap;
    const auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };   // every part as aligned as an allocation of its own
    const size_t n_out = up256(B * QV_ALIGN_ROW_BYTES), n_in = up256(B * (sizeof(QvAlignRow) + QV_ALIGN_PITCH * sizeof(uint16_t)));
    QvMirror m;
    QV_TRY_RC(qv_ctx_mirror(eng, c, n_out + n_in + B * tc * 64 * sizeof(uint32_t), n_out + n_in, "alignment workspace", &m));
    w.out = m.dev;
    w.plan = (QvAlignRow *)(m.dev + n_out);
    w.targets = (uint16_t *)(w.plan + B);
    w.out_host = m.host;
    w.in_host = m.host + n_out;
    w.bp = (uint32_t *)(m.dev + n_out + n_in);
    return QV_OK;
}

// kernel launch, one copy back, scatter into the caller's arrays (pitch >= QV_ALIGN_MAX_TOKENS entries per row); SYNCHRONOUS
static int align_run(qv_engine *eng, QvAlignWs &w, int t_cap, const float *lp, int t_max, const uint16_t *tok_base, int batch,
                     qv_align_info *info_host, uint16_t *ids_host, int16_t *first_host, int16_t *last_host, float *logp_host,
                     int pitch, hipStream_t stream) {
    if (t_cap > 384) hipLaunchKernelGGL(k_align<true>, dim3(batch), dim3(64), 0, stream, lp, t_max, tok_base, w.plan, w, t_cap);
    else hipLaunchKernelGGL(k_align<false>, dim3(batch), dim3(64), 0, stream, lp, t_max, tok_base, w.plan, w, t_cap);
    QV_HIP(hipGetLastError());
    QV_TRY_RC(qv_fetch_sync(eng, w.out_host, w.out, (size_t)batch * QV_ALIGN_ROW_BYTES, stream));
    const int n = QV_ALIGN_MAX_TOKENS;   // (entries past the longest alignable target hold the "no token" values as well)
    for (int b = 0; b < batch; ++b) {
        const unsigned char *rec = w.out_host + (size_t)b * QV_ALIGN_ROW_BYTES;
        const float *r_logp = (const float *)(rec + sizeof(qv_align_info));
        const int16_t *r_first = (const int16_t *)(r_logp + QV_ALIGN_PITCH), *r_last = r_first + QV_ALIGN_PITCH;
        memcpy(&info_host[b], rec, sizeof(qv_align_info));
        scatter_column(logp_host, pitch, b, r_logp, n, 0.f);
        scatter_column(first_host, pitch, b, r_first, n, (int16_t)-1);
        scatter_column(last_host, pitch, b, r_last, n, (int16_t)-1);
        scatter_column(ids_host, pitch, b, (const uint16_t *)(r_last + QV_ALIGN_PITCH), n, (uint16_t)0xFFFF);
    }
    return QV_OK;
}

int qv_align_explicit(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max, const uint16_t *targets_host,
                      const int32_t *lens_host, qv_align_info *info_host, int16_t *first_host, int16_t *last_host,
                      float *logp_host, int pitch, hipStream_t stream) {
    const QvWork &wk = c.work;
    if (batch > wk.max_batch || t_max > wk.t_cap) {
        qv_set_error(eng, "qv_align: batch or frame count exceeds engine capacity");
        return QV_ERR_CAPACITY;
    }
    for (int b = 0; b < batch; ++b)
        if (lens_host[b] < 0 || t_host[b] < 0 || t_host[b] > t_max) { qv_set_error(eng, "qv_align: lens_host[b] / t_host[b] out of range"); return QV_ERR_ARG; }
    QvAlignWs *w = nullptr;
    QV_TRY_RC(align_ws(eng, c, &w));
    // plan and targets are laid out in the pinned mirror as on the device and go up in one copy (the previous call has
    // finished with the mirror: alignment calls are synchronous and serialised by the engine's lock)
    QvAlignRow *plan = (QvAlignRow *)w->in_host;
    uint16_t *tg = (uint16_t *)(plan + wk.max_batch);
    size_t src = 0, n_tg = 0;
    for (int b = 0; b < batch; ++b) {
        const int L = lens_host[b];
        QvAlignRow &r = plan[b];
        r.tok_off = 0; r.L = L; r.T = t_host[b]; r.flags = 0; r.start = -1; r.span = 0;
        if (L >= 1 && L <= QV_ALIGN_MAX_TOKENS) {   // (longer lists are reported as QV_ALIGN_TOO_LONG and never read)
            for (int i = 0; i < L; ++i)
                if (targets_host[src + i] >= QV_BLANK) { qv_set_error(eng, "qv_align: target id outside 0..1023"); return QV_ERR_ARG; }
            r.tok_off = (int32_t)n_tg;
            memcpy(tg + n_tg, targets_host + src, sizeof(uint16_t) * L);
            n_tg += (size_t)L;
        }
        src += (size_t)L;
    }
    QV_HIP(hipMemcpyAsync(w->plan, w->in_host, sizeof(QvAlignRow) * wk.max_batch + sizeof(uint16_t) * n_tg, hipMemcpyHostToDevice, stream));
    return align_run(eng, *w, wk.t_cap, lp, t_max, w->targets, batch, info_host, nullptr, first_host, last_host, logp_host, pitch, stream);
}

int qv_align_results(qv_engine *eng, int k, int batch, qv_align_info *info_host, uint16_t *ids_host, int16_t *first_host,
                     int16_t *last_host, float *logp_host, int pitch) {
    QvCtx &c = eng->ctx[k];
    if (!c.al_lp || batch > c.al_batch) {
        qv_set_error(eng, "qv_align_results_ctx: the context holds no batch of that size (align before the context is reused)");
        return QV_ERR_ARG;
    }
    QvAlignWs *w = nullptr;
    QV_TRY_RC(align_ws(eng, c, &w));
    hipStream_t stream = nullptr;
    QV_TRY_RC(qv_stream_behind_batch(eng, c, &stream));
    hipLaunchKernelGGL(k_align_plan, dim3((batch + 63) / 64), dim3(64), 0, stream, eng->tab, c.work, batch, c.al_tmax, w->plan);
    return align_run(eng, *w, c.work.t_cap, c.al_lp, c.al_tmax, eng->tab.tok, batch, info_host, ids_host, first_host, last_host,
                     logp_host, pitch, stream);
}
