// qv_align_long_plan.h -- the thread layout and the workspace bytes of the long CTC alignment (include/qverse.h, "word and
// verse timings for recordings of any length").  Pure integer functions; no HIP here: qv_align_long.hip turns a plan into
// launches, qv_align_long_plan (the C entry) runs it on a CPU.
#pragma once

#include <stdint.h>

#include "qv_long_plan.h"

#define QV_AL_MAX_TOKENS 16383          // QV_ALIGN_LONG_MAX_TOKENS of the public header
#define QV_AL_MAX_BYTES (1LL << 32)     // QV_ALIGN_LONG_MAX_BYTES
#define QV_AL_VOCAB 1025
#define QV_AL_MAX_THREADS 1024

// states per thread of the instantiation that runs S = 2 L + 1 states; 0 = the row does not run (no target, or too long)
inline int32_t qv_al_ns(int32_t L) {
    if (L < 1 || L > QV_AL_MAX_TOKENS) return 0;
    const int32_t S = 2 * L + 1;
    return S <= 4 * QV_AL_MAX_THREADS ? 4 : S <= 8 * QV_AL_MAX_THREADS ? 8 : S <= 16 * QV_AL_MAX_THREADS ? 16 : 32;
}
// threads that hold a state, rounded up to whole waves
inline int32_t qv_al_threads(int32_t L) {
    const int32_t ns = qv_al_ns(L);
    return ns ? ((2 * L + 1 + ns - 1) / ns + 63) / 64 * 64 : 0;
}
// bytes of a recording's kept log-prob rows (every part as aligned as 16 bytes) and of its back-pointers: two bits per
// state and frame, a thread's NS states in one word of NS / 4 bytes, one row of `threads` words per frame
inline int64_t qv_al_kept_bytes(int32_t T) { return ((int64_t)T * QV_AL_VOCAB * 4 + 15) & ~(int64_t)15; }
inline int64_t qv_al_bp_bytes(int32_t T, int32_t L) { return (int64_t)T * qv_al_threads(L) * qv_al_ns(L) / 4; }

// windows and bytes of a whole call.  QV_LONG_BAD_ARG / QV_LONG_TOO_LONG as qv_long_plan_make, QV_LONG_TOO_LONG also above
// QV_AL_MAX_BYTES (the outputs are written all the same).
inline int qv_al_plan_rows(const int64_t *n_samples, const int32_t *n_tokens, int32_t rows, int32_t max_samples, int32_t window_samples,
                           int32_t margin_frames, int64_t *n_windows_total, int64_t *bytes) {
    if (!n_samples || !n_tokens || rows < 1) return QV_LONG_BAD_ARG;
    int64_t nw = 0, total = 0;
    for (int32_t r = 0; r < rows; ++r) {
        QvLongPlan p;
        const int rc = qv_long_plan_make(n_samples[r], max_samples, window_samples, margin_frames, &p);
        if (rc) return rc;
        if (n_tokens[r] < 0) return QV_LONG_BAD_ARG;
        nw += p.n_windows;
        total += qv_al_kept_bytes(p.t_total) + qv_al_bp_bytes(p.t_total, n_tokens[r]);
    }
    if (n_windows_total) *n_windows_total = nw;
    if (bytes) *bytes = total;
    return total > QV_AL_MAX_BYTES ? QV_LONG_TOO_LONG : QV_LONG_OK;
}
