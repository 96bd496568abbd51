// qv_long_plan.h -- how a recording longer than the engine's capacity is cut into windows the engine accepts, and which
// encoder frames of each window are kept (include/qverse.h, "recordings of any length").  Pure integer functions of the
// recording's length and three numbers; no HIP here: qv_long.hip turns a plan into launches, tools/long_plan_check.cpp runs
// the plans on a CPU.
//
// Everything is counted in encoder frames of QV_LONG_HOP = 1280 samples: qv_frames_for_samples(n) = n / 1280 + 1, so a
// window that starts at sample 1280 * a and runs to the end of an n-sample recording has T(n) - a frames, and local frame j
// of a window that starts at frame a is global frame a + j with no remainder at the end.
#pragma once

#include <stdint.h>

#define QV_LONG_HOP 1280
#define QV_LONG_FRAME_CAP 262144   // QV_LONG_MAX_FRAMES of the public header
#define QV_LONG_MIN_SAMPLES 400    // the forward's own minimum (one STFT window)

enum { QV_LONG_OK = 0, QV_LONG_BAD_ARG = 1 /* QV_ERR_ARG */, QV_LONG_TOO_LONG = 4 /* QV_ERR_CAPACITY */ };

struct QvLongPlan {
    int64_t n;          // samples of the recording
    int32_t kw;         // frames of a full window (window_samples / 1280)
    int32_t m;          // margin: frames dropped at each cut edge
    int32_t h;          // kw - 2 m: frames a window advances by
    int32_t t_total;    // frames of the recording
    int32_t n_windows;
};

inline int32_t qv_long_frames(int64_t n) { return (int32_t)(n / QV_LONG_HOP) + 1; }

// window_samples: a positive multiple of 1280, at most max_samples; 0 = the largest such multiple.
// margin_frames >= 0; -1 = min(50, kw / 4).  kw - 2 m >= 1.
inline int qv_long_plan_make(int64_t n, int32_t max_samples, int32_t window_samples, int32_t margin_frames, QvLongPlan *p) {
    if (n < 0 || max_samples < QV_LONG_HOP || window_samples < 0 || margin_frames < -1) return QV_LONG_BAD_ARG;
    if (window_samples == 0) window_samples = max_samples / QV_LONG_HOP * QV_LONG_HOP;
    if (window_samples % QV_LONG_HOP != 0 || window_samples > max_samples) return QV_LONG_BAD_ARG;
    const int32_t kw = window_samples / QV_LONG_HOP;
    const int32_t m = margin_frames < 0 ? (kw / 4 < 50 ? kw / 4 : 50) : margin_frames;
    if (m > (kw - 1) / 2) return QV_LONG_BAD_ARG;   // h = kw - 2 m >= 1
    if (n / QV_LONG_HOP + 1 > QV_LONG_FRAME_CAP) return QV_LONG_TOO_LONG;
    p->n = n; p->kw = kw; p->m = m; p->h = kw - 2 * m;
    p->t_total = qv_long_frames(n);
    p->n_windows = 1;
    if (n > window_samples) {
        // the smallest nw with 1280 * ((nw - 1) * h + kw) >= n: the last window is longer than 2 m frames
        const int64_t need = (n + QV_LONG_HOP - 1) / QV_LONG_HOP - kw;   // >= 1
        p->n_windows = 1 + (int32_t)((need + p->h - 1) / p->h);
    }
    return QV_LONG_OK;
}

// window w: its first sample, its samples (the rest of a [*, window_samples] row is zero), its frames
inline int64_t qv_long_start(const QvLongPlan &p, int32_t w) { return (int64_t)QV_LONG_HOP * w * p.h; }
inline int32_t qv_long_len(const QvLongPlan &p, int32_t w) {
    const int64_t rest = p.n - qv_long_start(p, w), full = (int64_t)QV_LONG_HOP * p.kw;
    return (int32_t)(rest < full ? rest : full);
}
inline int32_t qv_long_window_frames(const QvLongPlan &p, int32_t w) { return qv_long_frames(qv_long_len(p, w)); }
// the length the forward is given: a last window of fewer than 400 samples (possible with m = 0 only) is run as 400
// samples, the missing ones zero like the rest of its row -- still one frame
inline int32_t qv_long_fwd_len(const QvLongPlan &p, int32_t w) {
    const int32_t len = qv_long_len(p, w);
    return w > 0 && len < QV_LONG_MIN_SAMPLES ? QV_LONG_MIN_SAMPLES : len;
}
// window w owns the global frames [lo, hi); its local frame j is global frame w * h + j
inline int32_t qv_long_lo(const QvLongPlan &p, int32_t w) { return w == 0 ? 0 : w * p.h + p.m; }
inline int32_t qv_long_hi(const QvLongPlan &p, int32_t w) { return w == p.n_windows - 1 ? p.t_total : (w + 1) * p.h + p.m; }
