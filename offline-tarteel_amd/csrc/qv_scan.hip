// qv_scan.hip -- the exhaustive CTC scan: every verse and every span of up to max_span ayat scored by the rerank's float32
// alpha recursion on log-probs already in HBM, the best k selected on the device (include/qverse.h: qv_scan_logprobs,
// qv_scan_batch; the launch plan: qv_scan_plan.h).  No transcript, no retrieval, no candidate cap.
//
//   k_ctc_scan      one wave per recursion of the row's plan (a chain's longest feasible span): ctc_dispatch<true, 1> of
//                   qv_ctc_body.inc over the leader's tokens, then ctc_readout for every span of the chain -- alpha of the
//                   states 0 .. 2 P does not depend on what follows the first P tokens, so the bits are those of a recursion
//                   over the P tokens alone.  grid = (row, block of four plan slots): workgroups are dispatched x-fastest and
//                   the plan is sorted by decreasing length, so every row's longest recursions start first (as k_ctc's).
//   k_scan_select   one workgroup per row: the final score of every feasible key as an order-preserving 64-bit integer, then
//                   k rounds of "the largest key behind the previous winner" in (final descending, key ascending) -- a strict
//                   order, so the result is the stable top k.  Writes the row's record.
// Nothing waits for another workgroup; every loop is bounded by T, the plan or the table.
#include "qv_rows.h"
#include "qv_scan_plan.h"

namespace {

#include "qv_ctc_body.inc"   // ctc_wave2, ctc_dispatch, ctc_readout (k_ctc<> is not instantiated here)

#define SC_THREADS 256
#define SC_INF_BITS 0x7F800000u

struct QvScanRow { int32_t plan_off, n_rec, t_frames, pad; uint32_t mask[4]; };
static_assert(sizeof(QvScanRow) == 32 && sizeof(qv_scan_entry) == 40 && sizeof(qv_scan_info) == 16, "record layout");
#define SC_ROW_BYTES (sizeof(qv_scan_info) + QV_SCAN_MAX * sizeof(qv_scan_entry))

__global__ __launch_bounds__(256) void k_ctc_scan(QvTables tab, const QvScanRow *__restrict__ rows, const QvScanRec *__restrict__ plan,
                                                  const float *__restrict__ lp, int t_max, float *__restrict__ loss) {
    __shared__ float sa_all[4][768];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const QvScanRow r = rows[b];
    const int i = blockIdx.y * 4 + w;
    if (i >= r.n_rec) return;
    float *sa = sa_all[w];
    const QvScanRec e = plan[r.plan_off + i];
    const size_t k0 = (size_t)e.verse * QV_MAX_SPAN;
    const int L = (int)(tab.tok_off[k0 + e.lead_span] - tab.tok_off[k0 + e.lead_span - 1]);
    ctc_dispatch<true, 1>(lp + (size_t)b * t_max * QV_VOCAB, r.t_frames, tab.tok + tab.tok_off[k0 + e.lead_span - 1], L, lane, sa);
    float *out = loss + (size_t)b * tab.n_verses * QV_MAX_SPAN + k0;
    for (int k = e.first_span; k <= e.lead_span; ++k) {
        const int P = (int)(tab.tok_off[k0 + k] - tab.tok_off[k0 + k - 1]);
        const float l = ctc_readout(sa, P);
        if (lane == 0) out[k - 1] = l;
    }
}

// a double as an integer of the same order; 0 is below every value (-inf included)
__device__ __forceinline__ unsigned long long sc_order(double x) {
    x = __dadd_rn(x, 0.0);   // -0.0 and +0.0 are one value
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ bool sc_feasible(const QvTables &tab, const QvScanRow &r, int max_span, int key, int *L_out) {
    const int v = key / QV_MAX_SPAN, sp = key % QV_MAX_SPAN + 1;
    const int L = (int)(tab.tok_off[key + 1] - tab.tok_off[key]);
    *L_out = L;
    const int s = (int)tab.surah[v] - 1;
    return sp <= max_span && L > 0 && 2 * L + 1 <= r.t_frames && ((r.mask[(s >> 5) & 3] >> (s & 31)) & 1u);
}

// -norm - span_penalty * (sp - 1), in the rerank's arithmetic (k_ctc) without the text term
__device__ __forceinline__ double sc_final(float loss, int L, int sp, double penalty, float *norm_out) {
    const float norm = __fdiv_rn(loss, (float)L);
    *norm_out = norm;
    return __dsub_rn(-(double)norm, __dmul_rn(penalty, (double)(sp - 1)));
}

__global__ __launch_bounds__(SC_THREADS) void k_scan_select(QvTables tab, const QvScanRow *__restrict__ rows, const float *__restrict__ loss,
                                                            unsigned long long *__restrict__ order, int max_span, double penalty, int k,
                                                            unsigned char *__restrict__ out) {
    __shared__ unsigned long long s_u[SC_THREADS / 64];
    __shared__ int s_i[SC_THREADS / 64];
    __shared__ int s_cnt[SC_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const QvScanRow r = rows[b];
    const int NK = tab.n_verses * QV_MAX_SPAN;
    const float *ls = loss + (size_t)b * NK;
    unsigned long long *ord = order + (size_t)b * NK;
    int cnt = 0;
    for (int key = tid; key < NK; key += SC_THREADS) {
        int L;
        unsigned long long u = 0ull;
        if (sc_feasible(tab, r, max_span, key, &L)) {
            float norm;
            u = sc_order(sc_final(ls[key], L, key % QV_MAX_SPAN + 1, penalty, &norm));
            ++cnt;
        }
        ord[key] = u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();   // (also: this block's writes to `ord` are visible to all of its threads)
    int n_feasible = 0;
    for (int q = 0; q < SC_THREADS / 64; ++q) n_feasible += s_cnt[q];
    const int n_out = n_feasible < k ? n_feasible : k;

    unsigned char *rec = out + (size_t)b * SC_ROW_BYTES;
    qv_scan_entry *ent = (qv_scan_entry *)(rec + sizeof(qv_scan_info));
    unsigned long long pu = ~0ull;
    int pi = -1;
    for (int round = 0; round < n_out; ++round) {
        unsigned long long bu = 0ull;
        int bi = 0x7FFFFFFF;
        for (int key = tid; key < NK; key += SC_THREADS) {   // (keys ascend within a thread: the first largest one stays)
            const unsigned long long u = ord[key];
            const bool behind = u < pu || (u == pu && key > pi);
            if (u != 0ull && behind && u > bu) { bu = u; bi = key; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ou = __shfl_xor(bu, o);
            const int oi = __shfl_xor(bi, o);
            if (ou > bu || (ou == bu && oi < bi)) { bu = ou; bi = oi; }
        }
        __syncthreads();   // the previous round's s_u / s_i have been read
        if (lane == 0) { s_u[w] = bu; s_i[w] = bi; }
        __syncthreads();
        bu = s_u[0]; bi = s_i[0];
        for (int q = 1; q < SC_THREADS / 64; ++q)
            if (s_u[q] > bu || (s_u[q] == bu && s_i[q] < bi)) { bu = s_u[q]; bi = s_i[q]; }
        pu = bu; pi = bi;
        if (bu == 0ull) bi = 0;   // (cannot happen for round < n_feasible; an index inside the table whatever the scores hold)
        if (tid == 0) {
            qv_scan_entry e;
            const int v = bi / QV_MAX_SPAN, sp = bi % QV_MAX_SPAN + 1;
            const int L = (int)(tab.tok_off[bi + 1] - tab.tok_off[bi]);
            e.start_verse = v; e.span = sp; e.surah = tab.surah[v]; e.ayah = tab.ayah[v]; e.ayah_end = (int)tab.ayah[v] + sp - 1;
            e.n_tokens = L; e.loss = ls[bi];
            e.final_score = sc_final(e.loss, L, sp, penalty, &e.norm);
            ent[round] = e;
        }
    }
    if (tid >= n_out && tid < QV_SCAN_MAX) {
        qv_scan_entry z = {};
        ent[tid] = z;
    }
    if (tid == 0) {
        qv_scan_info inf;
        inf.n_entries = n_out; inf.n_feasible = n_feasible; inf.n_recursions = r.n_rec; inf.t_frames = r.t_frames;
        *(qv_scan_info *)rec = inf;
    }
}

}  // namespace

// What the engine keeps for the scan: the host copies of the table parts the plan is made from.
struct QvScanState {
    std::vector<uint32_t> tok_off;
    std::vector<uint8_t> pfx;
    QvScanView view;
    size_t n_chains = 0;      // recursions a row's plan can have at most
    float kernel_ms[2] = {0.f, 0.f};
};

void qv_scan_free(qv_engine *eng) {
    delete eng->scan;
    eng->scan = nullptr;
}

static int scan_state(qv_engine *eng, QvScanState **out) {
    if (eng->scan) { *out = eng->scan; return QV_OK; }
    QvScanState *s = new QvScanState();
    const size_t N = (size_t)eng->tab.n_verses, NK = N * QV_MAX_SPAN;
    s->tok_off.resize(NK + 1);
    s->pfx.resize(N);
    if (hipMemcpy(s->tok_off.data(), eng->tab.tok_off, sizeof(uint32_t) * (NK + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(s->pfx.data(), eng->tab.tok_pfx, N, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        delete s;
        qv_set_error(eng, "scan: cannot read the token table back");
        return QV_ERR_HIP;
    }
    s->view.n_verses = (int)N;
    s->view.tok_off = s->tok_off.data(); s->view.n_tok_off = s->tok_off.size();
    s->view.pfx = s->pfx.data(); s->view.n_pfx = s->pfx.size();
    s->view.surah = eng->h_surah.data(); s->view.n_surah = eng->h_surah.size();
    std::string err;
    if (int rc = qv_scan_view_check(s->view, err)) {
        delete s;
        qv_set_error(eng, err);
        return rc == QV_SCAN_BAD_ARG ? QV_ERR_ARG : QV_ERR_IO;
    }
    s->n_chains = qv_scan_chain_count(s->view);
    eng->scan = s;
    *out = s;
    return QV_OK;
}

int qv_scan_times(qv_engine *eng, float *ms2) {
    if (!eng->scan) return QV_ERR_ARG;
    ms2[0] = eng->scan->kernel_ms[0]; ms2[1] = eng->scan->kernel_ms[1];
    return QV_OK;
}

// plans (one per distinct (frame count, mask) of the call) and row descriptors up in one copy, two kernels, one copy back;
// SYNCHRONOUS on `stream`.  The workspace of the context, allocated by the first call that uses it: mirrored -- row
// descriptors, plans (max_batch rows of n_chains recursions), records; on the device alone -- the order keys and, for calls
// without loss_out_dev, the losses (max_batch * n_verses * 6 entries each).
int qv_scan_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max, int max_span, double penalty,
                 int k, const uint32_t *mask_host, qv_scan_info *info_host, qv_scan_entry *entries_host, float *loss_out_dev,
                 hipStream_t stream) {
    QV_TRY_RC(qv_rows_check(eng, "scan", c, batch, t_max, t_host));
    if (t_max > 2 * QV_SCAN_MAX_L + 2) { qv_set_error(eng, "scan: more than 768 frames admit targets the wave programs do not hold"); return QV_ERR_CAPACITY; }
    QvScanState *s = nullptr;
    QV_TRY_RC(scan_state(eng, &s));
    const size_t B = (size_t)c.work.max_batch, NK = (size_t)eng->tab.n_verses * QV_MAX_SPAN;
    const size_t rows_bytes = qv_up16(B * sizeof(QvScanRow)), plan_bytes = qv_up16(B * s->n_chains * sizeof(QvScanRec));
    const size_t out_off = rows_bytes + plan_bytes, order_off = qv_up16(out_off + B * SC_ROW_BYTES), loss_off = order_off + B * NK * sizeof(unsigned long long);
    QvMirror &m = c.scan;
    if (!m.dev) QV_TRY_RC(qv_ctx_mirror(eng, c, loss_off + B * NK * sizeof(float), order_off, "scan workspace", &m));

    // ---- the plans
    QvScanRow *rows = (QvScanRow *)m.host;
    QvScanRec *plan = (QvScanRec *)(m.host + rows_bytes);
    size_t used = 0;
    int max_rec = 0;
    QvScanPlan p;
    std::string err;
    for (int b = 0; b < batch; ++b) {
        QvScanRow &r = rows[b];
        r.t_frames = t_host[b]; r.pad = 0;
        for (int q = 0; q < 4; ++q) r.mask[q] = mask_host ? mask_host[(size_t)b * 4 + q] : 0xFFFFFFFFu;
        int same = -1;
        for (int a = 0; a < b && same < 0; ++a)
            if (rows[a].t_frames == r.t_frames && !memcmp(rows[a].mask, r.mask, sizeof r.mask)) same = a;
        if (same >= 0) { r.plan_off = rows[same].plan_off; r.n_rec = rows[same].n_rec; continue; }
        if (int rc = qv_scan_plan_make(s->view, r.t_frames, max_span, r.mask, p, err)) {
            qv_set_error(eng, "qv_scan: " + err);
            return rc == QV_SCAN_BAD_ARG ? QV_ERR_ARG : QV_ERR_IO;
        }
        if (p.rec.size() > s->n_chains) { qv_set_error(eng, "scan: a plan larger than the table's chains"); return QV_ERR_CAPACITY; }
        r.plan_off = (int32_t)used; r.n_rec = (int32_t)p.rec.size();
        if (r.n_rec) memcpy(plan + used, p.rec.data(), sizeof(QvScanRec) * p.rec.size());
        used += p.rec.size();
        max_rec = std::max(max_rec, r.n_rec);
    }
    QV_HIP(hipMemcpyAsync(m.dev, m.host, rows_bytes + used * sizeof(QvScanRec), hipMemcpyHostToDevice, stream));

    // ---- the kernels
    float *loss = loss_out_dev ? loss_out_dev : (float *)(m.dev + loss_off);
    QV_HIP(hipMemsetD32Async((hipDeviceptr_t)loss, (int)SC_INF_BITS, (size_t)batch * NK, stream));
    // qv_profile_stages: events around the two launches (destroyed below on every path: nothing returns in between)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timed = eng->profile_stages;
    for (int q = 0; q < 3 && timed; ++q)
        if (hipEventCreate(&ev[q]) != hipSuccess) { (void)hipGetLastError(); timed = false; }
    if (timed) (void)hipEventRecord(ev[0], stream);
    if (max_rec > 0)
        hipLaunchKernelGGL(k_ctc_scan, dim3(batch, (max_rec + 3) / 4), dim3(256), 0, stream, eng->tab, (const QvScanRow *)m.dev,
                           (const QvScanRec *)(m.dev + rows_bytes), lp, t_max, loss);
    if (timed) (void)hipEventRecord(ev[1], stream);
    hipLaunchKernelGGL(k_scan_select, dim3(batch), dim3(SC_THREADS), 0, stream, eng->tab, (const QvScanRow *)m.dev, (const float *)loss,
                       (unsigned long long *)(m.dev + order_off), max_span, penalty, k, m.dev + out_off);
    if (timed) (void)hipEventRecord(ev[2], stream);
    const hipError_t launched = hipGetLastError();
    const int rc = launched == hipSuccess ? qv_fetch_sync(eng, m.host + out_off, m.dev + out_off, SC_ROW_BYTES * batch, stream) : (int)QV_ERR_HIP;
    if (launched != hipSuccess) qv_set_error(eng, std::string("scan: launch failed: ") + hipGetErrorString(launched));
    if (timed && rc == QV_OK) {
        (void)hipEventElapsedTime(&s->kernel_ms[0], ev[0], ev[1]);
        (void)hipEventElapsedTime(&s->kernel_ms[1], ev[1], ev[2]);
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc) return rc;
    for (int b = 0; b < batch; ++b) {
        const unsigned char *rec = m.host + out_off + SC_ROW_BYTES * b;
        memcpy(&info_host[b], rec, sizeof(qv_scan_info));
        memcpy(entries_host + (size_t)b * k, rec + sizeof(qv_scan_info), sizeof(qv_scan_entry) * k);
    }
    return QV_OK;
}
