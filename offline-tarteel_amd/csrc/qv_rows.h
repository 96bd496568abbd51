// qv_rows.h -- what the row-wise features (alignment, n-best, transcription, beam search, long transcription) share on the
// host: the device buffer + pinned mirror they travel through (QvMirror, qv_common.h), the checks on a batch of rows, the
// copies up and back, the stream a result call runs on, and the scatter of a record's columns into the caller's arrays.
#pragma once

#include <string.h>

#include "qv_common.h"

#define QV_TRY_RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

static inline size_t qv_up16(size_t n) { return (n + 15) & ~(size_t)15; }

static inline void qv_mirror_free(QvMirror &m) {
    if (m.dev) (void)hipFree(m.dev);
    if (m.host) (void)hipHostFree(m.host);
    m = {};
}

// dev_bytes of device memory and host_bytes of pinned memory, or neither: `what` names the workspace in the error text
static inline int qv_mirror_alloc(qv_engine *eng, QvMirror &m, size_t dev_bytes, size_t host_bytes, const char *what) {
    void *d = nullptr, *h = nullptr;
    if (hipMalloc(&d, dev_bytes) != hipSuccess || hipHostMalloc(&h, host_bytes, hipHostMallocDefault) != hipSuccess) {
        if (d) (void)hipFree(d);
        (void)hipGetLastError();   // (the error is reported here: it must not stick to the next HIP call)
        qv_set_error(eng, std::string(what) + ": out of memory");
        return QV_ERR_HIP;
    }
    m = {(unsigned char *)d, (unsigned char *)h, dev_bytes, host_bytes};
    return QV_OK;
}

// a mirror owned by context `c` (freed by qv_destroy); *view is the caller's copy of its pointers
static inline int qv_ctx_mirror(qv_engine *eng, QvCtx &c, size_t dev_bytes, size_t host_bytes, const char *what, QvMirror *view) {
    const int rc = qv_mirror_alloc(eng, *view, dev_bytes, host_bytes, what);
    if (rc == QV_OK) c.mirrors.push_back(*view);
    return rc;
}

// the workspace of a feature with one record of row_bytes per row, allocated by the first call that uses it
static inline int qv_row_ws(qv_engine *eng, QvCtx &c, QvRowWs &w, size_t row_bytes, const char *what) {
    if (w.m.dev) return QV_OK;
    const size_t B = (size_t)c.work.max_batch, t_bytes = qv_up16(B * sizeof(int32_t)), bytes = t_bytes + B * row_bytes;
    const int rc = qv_ctx_mirror(eng, c, bytes, bytes, what, &w.m);
    if (rc == QV_OK) w.t_bytes = t_bytes;
    return rc;
}

// a batch of rows against the context's capacity; `who` is the feature's prefix in the error text
static inline int qv_rows_check(qv_engine *eng, const char *who, const QvCtx &c, int batch, int t_max, const int32_t *t_host) {
    if (batch > c.work.max_batch) { qv_set_error(eng, std::string(who) + ": batch exceeds engine capacity"); return QV_ERR_CAPACITY; }
    if (t_max > c.work.t_cap) { qv_set_error(eng, std::string(who) + ": t_max exceeds the engine's frame capacity"); return QV_ERR_CAPACITY; }
    for (int b = 0; b < batch; ++b)
        if (t_host[b] < 0 || t_host[b] > t_max) { qv_set_error(eng, std::string(who) + ": t_host[b] outside 0..t_max"); return QV_ERR_ARG; }
    return QV_OK;
}

// the rows' frame counts up through the front of the mirror (the previous call has finished with it: the calls that use a
// row workspace are synchronous and serialised by the engine's lock)
static inline int qv_rows_send_t(qv_engine *eng, const QvRowWs &w, const int32_t *t_host, int batch, hipStream_t stream) {
    memcpy(w.m.host, t_host, sizeof(int32_t) * batch);
    QV_HIP(hipMemcpyAsync(w.m.dev, w.m.host, sizeof(int32_t) * batch, hipMemcpyHostToDevice, stream));
    return QV_OK;
}

// one copy back into pinned memory, then the host waits for the stream: what every row-wise call ends its device work with
static inline int qv_fetch_sync(qv_engine *eng, void *host, const void *dev, size_t bytes, hipStream_t stream) {
    QV_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream));
    QV_HIP(hipStreamSynchronize(stream));
    return QV_OK;
}

// The stream for a call about the batch that context `c` ran last, ordered behind that batch: the context's own stream when
// the batch ran there, else the null stream after a device-wide join (the batch ran on a caller's stream we were not given
// -- as qv_fetch_results_ctx).
static inline int qv_stream_behind_batch(qv_engine *eng, QvCtx &c, hipStream_t *stream) {
    *stream = eng->n_ctx > 1 ? c.stream : nullptr;
    if (eng->n_ctx == 1 || c.al_stream != c.stream) QV_HIP(hipDeviceSynchronize());
    return QV_OK;
}

// one column of a record into row `row` of the caller's [*, pitch] array: n entries, `fill` (the "no token" value) behind
// them; a column the caller did not ask for (dst == nullptr) is skipped
template <typename T>
static inline void scatter_column(T *dst, int pitch, int row, const T *src, int n, T fill) {
    if (!dst) return;
    T *d = dst + (size_t)row * pitch;
    memcpy(d, src, sizeof(T) * n);
    for (int i = n; i < pitch; ++i) d[i] = fill;
}

// qv_profile_stages: HIP events around every launch of a long call's own kernels (up to three kinds), summed per kind after
// the call's synchronisation (qv_long.hip, qv_align_long.hip)
struct QvLongTimer {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev[3];
    void mark(int which) {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(e, s);
        ev[which].push_back(e);
    }
    void finish(float ms[3]) {   // after the stream has been synchronised
        for (int k = 0; k < 3; ++k) {
            ms[k] = 0.f;
            for (size_t i = 0; i + 1 < ev[k].size(); i += 2) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, ev[k][i], ev[k][i + 1]) == hipSuccess) ms[k] += t;
            }
        }
    }
    ~QvLongTimer() {
        for (auto &v : ev)
            for (hipEvent_t e : v) (void)hipEventDestroy(e);
    }
};
