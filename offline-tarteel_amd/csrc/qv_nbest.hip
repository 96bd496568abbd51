// qv_nbest.hip -- ranked alternatives of every prediction, selected on the device from what a batch left in HBM
// (include/qverse.h: qv_nbest_results_ctx, qv_nbest_select).
//
// The rerank's ranked list is `sorted(finite-loss candidates, key=final_score, reverse=True)` (c2c-direct/run.py:378-379):
// a stable descending sort, i.e. the order (final desc, candidate index asc) under IEEE > / == on doubles -- better()
// (qv_greedy.h), which k_result takes the first maximum with.  k_nbest takes the first k of that order: one
// workgroup per utterance, candidate c = tid + 256 j held in a register of thread tid (QV_CAND_CAP / 256 = 8 doubles),
// every thread's best cached; a round is one wave reduction + one four-entry LDS exchange, after which only the thread
// that owned the winner rescans its eight registers (the scheme of local_best / k_topk).  k rounds, no LDS copy of the
// candidate arrays, no bit-pattern keys (so -0.0 and +0.0 tie as they do in Python).
#include "qv_common.h"
#include "qv_greedy.h"
#include "qv_rows.h"

namespace {

constexpr int NB_THREADS = 256;
constexpr int NB_PER = QV_CAND_CAP / NB_THREADS;   // candidates per thread
constexpr uint32_t NB_NONE = 0xFFFFFFFFu;          // "no candidate": loses every comparison against a real index
static_assert(NB_PER * NB_THREADS == QV_CAND_CAP && NB_PER <= 32, "one live bit per register");

struct NbShared {
    double s[2][4];        // the waves' bests of a round (two rounds in flight: one barrier per round)
    uint32_t k[2][4];
    int32_t cnt[4];
    int32_t idx[QV_NBEST_MAX];
};

// Leaves the indices of the stable top k of fin[0 .. n) among the entries with a finite loss in sh.idx and returns how
// many there are (the same value in every thread); *n_ranked = number of finite-loss entries.  n <= QV_CAND_CAP.
__device__ int nbest_select_block(const double *__restrict__ fin, const float *__restrict__ loss, int n, int k, NbShared &sh,
                                  int *n_ranked) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v[NB_PER];
    uint32_t live = 0;
#pragma unroll
    for (int j = 0; j < NB_PER; ++j) {
        const int c = tid + j * NB_THREADS;
        v[j] = -INFINITY;
        if (c < n && isfinite(loss[c])) { v[j] = fin[c]; live |= 1u << j; }
    }
    int cnt = __popc(live);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) sh.cnt[wave] = cnt;
    double ls;
    uint32_t lk;
    auto rescan = [&]() {
        ls = -INFINITY;
        lk = NB_NONE;
#pragma unroll
        for (int j = 0; j < NB_PER; ++j) {
            const uint32_t c = (uint32_t)(tid + j * NB_THREADS);
            if ((live >> j & 1u) && better(v[j], c, ls, lk)) { ls = v[j]; lk = c; }
        }
    };
    rescan();
    int count = 0;
    for (int r = 0; r < k; ++r) {
        double s = ls;
        uint32_t key = lk;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double s2 = __shfl_xor(s, o);
            const uint32_t k2 = __shfl_xor(key, o);
            if (better(s2, k2, s, key)) { s = s2; key = k2; }
        }
        double *ps = sh.s[r & 1];
        uint32_t *pk = sh.k[r & 1];
        if (lane == 0) { ps[wave] = s; pk[wave] = key; }
        __syncthreads();
        s = ps[0];
        key = pk[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (better(ps[w], pk[w], s, key)) { s = ps[w]; key = pk[w]; }
        if (key == NB_NONE) break;   // (the same LDS values in every thread: the exit is uniform)
        if (tid == 0) sh.idx[r] = (int32_t)key;
        if ((int)(key & (NB_THREADS - 1)) == tid) {
            live &= ~(1u << (key / NB_THREADS));
            rescan();
        }
        ++count;
    }
    __syncthreads();
    *n_ranked = sh.cnt[0] + sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
    return count;
}

__device__ __forceinline__ qv_nbest_entry nb_zero_entry() {
    qv_nbest_entry e;
    e.surah = e.ayah = e.ayah_end = 0;
    e.start_verse = 0; e.span = 0; e.cand_index = 0; e.source = QV_SOURCE_NONE; e.n_tokens = 0;
    e.score = 0.0; e.text_score = 0.0;
    e.ctc_loss = 0.f; e.ctc_norm_loss = 0.f;
    return e;
}

__device__ __forceinline__ qv_nbest_entry nb_text_entry(const QvTables &tab, int st, int sp, double score) {
    qv_nbest_entry e = nb_zero_entry();
    e.surah = tab.surah[st]; e.ayah = tab.ayah[st]; e.ayah_end = e.ayah + sp - 1;
    e.start_verse = st; e.span = sp; e.cand_index = -1; e.source = QV_SOURCE_TEXT;
    e.score = score; e.text_score = score;
    return e;
}

// One workgroup per utterance of a finished batch: reads the row's qv_result (which decided the source), the candidate
// arrays k_candidates / k_ctc left, match_verse's runners-up, and writes the row's record.
__global__ __launch_bounds__(NB_THREADS) void k_nbest(QvTables tab, QvWork wk, int k, int flags, unsigned char *__restrict__ out) {
    __shared__ NbShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const qv_result res = wk.results[b];
    const QvUtt &u = wk.utt[b];
    unsigned char *rec = out + (size_t)b * QV_NBEST_ROW_BYTES;
    qv_nbest_entry *ent = (qv_nbest_entry *)(rec + sizeof(qv_nbest_info));
    const bool has = res.surah != 0 && !(res.flags & QV_FLAG_TRANSCRIPT_TRUNCATED);
    int n_entries = 0, n_ranked = 0, source = QV_SOURCE_NONE;
    if (has && res.source == QV_SOURCE_CTC) {
        source = QV_SOURCE_CTC;
        const size_t o = (size_t)b * QV_CAND_CAP;
        const int n = u.n_cand < 0 ? 0 : (u.n_cand > QV_CAND_CAP ? QV_CAND_CAP : u.n_cand);
        n_entries = nbest_select_block(wk.cand_final + o, wk.cand_loss + o, n, k, sh, &n_ranked);
        for (int i = tid; i < n_entries; i += NB_THREADS) {
            const int c = sh.idx[i];
            const int st = wk.cand_start[o + c], sp = wk.cand_span[o + c];
            qv_nbest_entry e = nb_zero_entry();
            e.cand_index = c; e.source = QV_SOURCE_CTC; e.start_verse = st; e.span = sp;
            e.score = wk.cand_final[o + c];
            e.text_score = wk.cand_score[o + c];
            e.ctc_loss = wk.cand_loss[o + c];
            if (st >= 0 && st < tab.n_verses && sp >= 1 && sp <= QV_MAX_SPAN) {
                const size_t tk = (size_t)st * QV_MAX_SPAN + (sp - 1);
                const int L = (int)(tab.tok_off[tk + 1] - tab.tok_off[tk]);
                e.n_tokens = L;
                e.ctc_norm_loss = __fdiv_rn(e.ctc_loss, (float)L);   // k_result's own division: the same bits
                e.surah = tab.surah[st]; e.ayah = tab.ayah[st]; e.ayah_end = e.ayah + sp - 1;
            }
            ent[i] = e;
        }
    } else if (has && res.source == QV_SOURCE_TEXT && u.base_start >= 0 && u.base_start < tab.n_verses) {
        source = QV_SOURCE_TEXT;
        n_entries = 1;
        if (tid == 0) ent[0] = nb_text_entry(tab, u.base_start, u.base_span, u.base_score);
        if (flags & QV_NBEST_TEXT_RUNNERS) {
            // ordered compaction of the runner list (at most QV_RUNNER_CAP = 128 entries: waves 0 and 1)
            const int nrun = u.n_runners < 0 ? 0 : (u.n_runners > QV_RUNNER_CAP ? QV_RUNNER_CAP : u.n_runners);
            const int32_t *ri = wk.runner_idx + (size_t)b * QV_RUNNER_CAP;
            const double *rs = wk.runner_score + (size_t)b * QV_RUNNER_CAP;
            int st = -1;
            if (tid < nrun) st = ri[tid];
            const bool keep = st >= 0 && st < tab.n_verses && !(u.base_span == 1 && st == u.base_start);
            const unsigned long long bal = __ballot(keep);
            if (lane == 0) sh.cnt[wave] = __popcll(bal);
            __syncthreads();
            int pos = 1 + __popcll(bal & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) pos += sh.cnt[w];
            if (keep && pos < k) ent[pos] = nb_text_entry(tab, st, 1, rs[tid]);
            const int total = 1 + sh.cnt[0] + sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
            n_entries = total < k ? total : k;
        }
    }
    for (int i = n_entries + tid; i < QV_NBEST_MAX; i += NB_THREADS) ent[i] = nb_zero_entry();
    if (tid == 0) {
        qv_nbest_info inf;
        inf.n_entries = n_entries;
        inf.n_ranked = n_ranked;
        inf.source = source;
        inf.flags = res.flags;
        *(qv_nbest_info *)rec = inf;
    }
}

// the same selection on staged vectors: row r of fin / loss [rows][pitch]; out[r] = count, then QV_NBEST_MAX indices
__global__ __launch_bounds__(NB_THREADS) void k_nbest_select(const double *__restrict__ fin, const float *__restrict__ loss,
                                                             const int32_t *__restrict__ n_rows, int pitch, int k,
                                                             int32_t *__restrict__ out) {
    __shared__ NbShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cap = pitch < QV_CAND_CAP ? pitch : QV_CAND_CAP;
    const int n = n_rows[b] < 0 ? 0 : (n_rows[b] > cap ? cap : n_rows[b]);
    int n_ranked = 0;
    const int count = nbest_select_block(fin + (size_t)b * pitch, loss + (size_t)b * pitch, n, k, sh, &n_ranked);
    int32_t *o = out + (size_t)b * QV_NBEST_SEL_PITCH;
    if (tid == 0) o[0] = count;
    if (tid < QV_NBEST_MAX) o[1 + tid] = tid < count ? sh.idx[tid] : -1;
}

}  // namespace

// The n-best workspace of one context: max_batch records of QV_NBEST_ROW_BYTES (1,808) bytes in device memory plus a
// pinned mirror; an engine that never asks for alternatives pays nothing.
static int nbest_ws(qv_engine *eng, QvCtx &c, QvNbestWs **out) {
    QvNbestWs &w = c.nbest;
    *out = &w;
    if (w.out) return QV_OK;
    const size_t n_out = (size_t)c.work.max_batch * QV_NBEST_ROW_BYTES;
    QvMirror m;
    QV_TRY_RC(qv_ctx_mirror(eng, c, n_out, n_out, "n-best workspace", &m));
    w.out = m.dev;
    w.out_host = m.host;
    return QV_OK;
}

int qv_nbest_results(qv_engine *eng, int k_ctx, int batch, int k, int flags, qv_nbest_info *info_host, qv_nbest_entry *entries_host) {
    QvCtx &c = eng->ctx[k_ctx];
    if (!c.al_lp || batch > c.al_batch) {
        qv_set_error(eng, "qv_nbest_results_ctx: the context holds no batch of that size (ask before the context is reused)");
        return QV_ERR_ARG;
    }
    QvNbestWs *w = nullptr;
    QV_TRY_RC(nbest_ws(eng, c, &w));
    hipStream_t stream = nullptr;
    QV_TRY_RC(qv_stream_behind_batch(eng, c, &stream));
    hipLaunchKernelGGL(k_nbest, dim3(batch), dim3(NB_THREADS), 0, stream, eng->tab, c.work, k, flags, w->out);
    QV_HIP(hipGetLastError());
    QV_TRY_RC(qv_fetch_sync(eng, w->out_host, w->out, (size_t)batch * QV_NBEST_ROW_BYTES, stream));
    for (int b = 0; b < batch; ++b) {
        const unsigned char *rec = w->out_host + (size_t)b * QV_NBEST_ROW_BYTES;
        memcpy(&info_host[b], rec, sizeof(qv_nbest_info));
        memcpy(entries_host + (size_t)b * k, rec + sizeof(qv_nbest_info), sizeof(qv_nbest_entry) * k);
    }
    return QV_OK;
}

int qv_nbest_select_rows(qv_engine *eng, QvCtx &c, const double *final_host, const float *loss_host, const int32_t *n_host, int rows,
                         int pitch, int k, int32_t *index_host, int32_t *count_host, hipStream_t stream) {
    QvNbestWs *w = nullptr;
    QV_TRY_RC(nbest_ws(eng, c, &w));
    const size_t B = (size_t)c.work.max_batch;
    if (!w->sel_final) {
        void *p = nullptr;
        const size_t bytes = B * ((size_t)QV_CAND_CAP * (sizeof(double) + sizeof(float)) + sizeof(int32_t) * (1 + QV_NBEST_SEL_PITCH));
        QV_HIP(hipMalloc(&p, bytes));
        eng->allocs.push_back(p);
        w->sel_final = (double *)p;
        w->sel_loss = (float *)(w->sel_final + B * QV_CAND_CAP);
        w->sel_n = (int32_t *)(w->sel_loss + B * QV_CAND_CAP);
        w->sel_idx = w->sel_n + B;
    }
    static_assert(QV_NBEST_SEL_PITCH * sizeof(int32_t) <= QV_NBEST_ROW_BYTES, "the indices come back through the records' mirror");
    const size_t n = (size_t)rows * pitch;
    if (n) {
        QV_HIP(hipMemcpyAsync(w->sel_final, final_host, n * sizeof(double), hipMemcpyHostToDevice, stream));
        QV_HIP(hipMemcpyAsync(w->sel_loss, loss_host, n * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    QV_HIP(hipMemcpyAsync(w->sel_n, n_host, (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_nbest_select, dim3(rows), dim3(NB_THREADS), 0, stream, w->sel_final, w->sel_loss, w->sel_n, pitch, k, w->sel_idx);
    QV_HIP(hipGetLastError());
    QV_TRY_RC(qv_fetch_sync(eng, w->out_host, w->sel_idx, (size_t)rows * QV_NBEST_SEL_PITCH * sizeof(int32_t), stream));
    const int32_t *got = (const int32_t *)w->out_host;
    for (int r = 0; r < rows; ++r) {
        count_host[r] = got[(size_t)r * QV_NBEST_SEL_PITCH];
        memcpy(index_host + (size_t)r * k, got + (size_t)r * QV_NBEST_SEL_PITCH + 1, sizeof(int32_t) * k);
    }
    return QV_OK;
}
