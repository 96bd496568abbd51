// qv_align_long.hip -- CTC forced alignment over the frames of a whole recording and a target of up to 16,383 tokens
// (include/qverse.h: qv_align_long, qv_align_windows, qv_align_long_plan; the byte formula: qv_align_long_plan.h).
//
// The recording goes through the windows and rounds of qv_transcribe_long (qv_long.hip: qv_long_check / qv_long_tables /
// qv_long_rounds).  What differs is what a round leaves behind:
//   k_long_keep     the log-prob rows a window OWNS, from the round's tensor to their GLOBAL frame index in a per-recording
//                   f32[T, 1025] buffer, before the next round reuses the tensor (16-byte stores, 16-byte loads where the
//                   source is as aligned as the destination; HBM-bound);
//   k_align_long    once per call, one workgroup per recording: qv_align.hip's recursion with the states spread over up to
//                   1,024 threads.  Thread i holds states i * NS .. i * NS + NS - 1 of the blank-extended target in registers
//                   (NS even: even registers are blank states, odd ones token states) and updates them in place from the
//                   highest down; state i * NS needs the OLD last state of thread i - 1 -- __shfl_up inside a wave, a
//                   double-buffered LDS slot per wave across waves: ONE workgroup barrier per frame.  The gathers
//                   lp[t][tok] of TCH frames are issued before the first of those frames' barriers (no LDS-DMA is in flight
//                   in this kernel, so the barrier does not wait for them).  Every frame leaves two bits per state, a
//                   thread's NS states in one word of NS / 4 bytes, stored coalesced (bp[t][thread]) after the chunk.
//                   Wave 0 then walks t = T-1 .. 1 backwards in the same launch: it reads words OTHER waves wrote, so the
//                   workgroup releases to the device's L2 before the barrier and acquires behind it (as k_long_collapse
//                   before it reads o_logp).  The path moves at most two states per frame, so a chunk of 16 frames touches
//                   at most 32 / NS + 2 threads' words per frame: lane l loads the words of thread (owner - l) for the
//                   whole chunk ahead of the scalar chain, which picks its word with v_readlane.  first / last are written
//                   where the state changes; the read-out (one thread per token, a sequential float32 sum over the kept
//                   rows) follows behind a second release / acquire.
// No other workgroup is involved: nothing is handed from one workgroup to another.
#include "qv_align_long_plan.h"
#include "qv_rows.h"

#include <algorithm>

static_assert(QV_AL_MAX_TOKENS == QV_ALIGN_LONG_MAX_TOKENS && QV_AL_MAX_BYTES == QV_ALIGN_LONG_MAX_BYTES && QV_AL_VOCAB == QV_VOCAB,
              "qv_align_long_plan.h and qverse.h disagree");
static_assert(sizeof(qv_align_long_info) == 24, "record layout");

namespace {

constexpr float AL_NEG = -1e30f;

// one recording of the call (device plan table)
struct AlRow {
    int64_t lp_off;      // first float of the recording's kept rows
    int64_t bp_off;      // first byte of its back-pointers
    int32_t tok_off;     // first token of its target in the staged targets
    int32_t L, T;
    int32_t ns;          // the instantiation that runs it; 0 = flagged on the host, never run
    int32_t threads;     // threads that hold a state (a multiple of 64): words per frame of the back-pointers
    int32_t n_windows;
};
static_assert(sizeof(AlRow) == 40, "plan table layout");

#define LK_THREADS 256
// grid: (ceil((2 + ceil(most owned floats / 4)) / LK_THREADS), windows of the round).  Thread group 0 copies the floats in
// front of the first 16-byte boundary of the destination, group g >= 1 the four floats behind it, the last one the rest.
__global__ __launch_bounds__(LK_THREADS) void k_long_keep(const float *__restrict__ lp, int t_max, const QvLongWin *__restrict__ tab,
                                                         const int64_t *__restrict__ keep_dst, float *__restrict__ kept) {
    const QvLongWin w = tab[blockIdx.y];
    const int64_t d0 = keep_dst[blockIdx.y];
    if (d0 < 0) return;                                 // a recording that is not aligned (flagged on the host)
    const int64_t n = (int64_t)w.count * QV_VOCAB;
    const float *src = lp + ((size_t)w.lp_win * t_max + w.j0) * QV_VOCAB;
    float *dst = kept + d0;                             // (kept itself is 16-byte aligned)
    const int head = (int)((4 - (d0 & 3)) & 3);
    const int64_t g = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
    const int64_t lo = g == 0 ? 0 : head + 4 * (g - 1);
    int64_t hi = g == 0 ? head : lo + 4;
    hi = hi < n ? hi : n;
    if (lo >= hi) return;
    if (g > 0 && hi - lo == 4) {
        float4 v;
        if ((((uintptr_t)(src + lo)) & 15) == 0) v = *(const float4 *)(src + lo);
        else { v.x = src[lo]; v.y = src[lo + 1]; v.z = src[lo + 2]; v.w = src[lo + 3]; }
        *(float4 *)(dst + lo) = v;
    } else {
        for (int64_t i = lo; i < hi; ++i) dst[i] = src[i];
    }
}

template <int NS> struct BpWord;
template <> struct BpWord<4> { typedef uint8_t type; };
template <> struct BpWord<8> { typedef uint16_t type; };
template <> struct BpWord<16> { typedef uint32_t type; };
template <> struct BpWord<32> { typedef uint64_t type; };

#define AL_WAVES 16

// grid: recordings; block: the most threads a recording of this instantiation needs (threads behind a recording's own count
// hold states beyond 2L, which never feed a lower state; they store nothing).  first / last / logp: [rows, P].
template <int NS>
__global__ __launch_bounds__(64 * AL_WAVES) void k_align_long(const float *__restrict__ kept, const uint16_t *__restrict__ targets,
                                                             const AlRow *__restrict__ plan, unsigned char *bp_base,
                                                             qv_align_long_info *__restrict__ o_info, int32_t *o_first, int32_t *o_last,
                                                             float *__restrict__ o_logp, int P) {
    typedef typename BpWord<NS>::type W;
    constexpr int G = NS / 2;                                        // token states (gathers) per thread and frame
    constexpr int TCH = NS <= 8 ? 8 : NS == 16 ? 4 : 2;             // frames fetched ahead: (G + 1) * TCH <= 40 registers
    constexpr int BCH = 16;                                          // frames of the backward walk per chunk
    __shared__ float xch[2][AL_WAVES];
    __shared__ float s_end[2];
    const AlRow r = plan[blockIdx.x];
    if (r.ns != NS) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = r.L, T = r.T, S = 2 * L + 1, nthr = r.threads;
    const float *lp = kept + r.lp_off;
    const uint16_t *tgt = targets + r.tok_off;
    W *bp = (W *)(bp_base + r.bp_off);
    int32_t *first = o_first + (size_t)blockIdx.x * P, *last = o_last + (size_t)blockIdx.x * P;
    float *logp = o_logp + (size_t)blockIdx.x * P;

    int tok[G];
    bool skip_ok[G];
    float a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = tid * NS + k;
        a[k] = AL_NEG;
        if (k & 1) {
            tok[k >> 1] = QV_BLANK;
            skip_ok[k >> 1] = false;
            if (s < S) {
                tok[k >> 1] = tgt[s >> 1];
                skip_ok[k >> 1] = s > 1 && tgt[s >> 1] != tgt[(s >> 1) - 1];
            }
        }
    }
    if (tid == 0) { a[0] = lp[QV_BLANK]; a[1] = lp[tok[0]]; }

    for (int t0 = 1; t0 < T; t0 += TCH) {
        float lpv[TCH][G], lpb[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            const int t = t0 + j < T ? t0 + j : T - 1;
            const float *row = lp + (size_t)t * QV_VOCAB;
            lpb[j] = row[QV_BLANK];
#pragma unroll
            for (int g = 0; g < G; ++g) lpv[j][g] = row[tok[g]];
        }
        // the frames' words are collected in registers and stored after the chunk (qv_align.hip says why)
        W wv[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            wv[j] = 0;
            if (t0 + j >= T) break;                      // (uniform: every thread of the workgroup leaves here)
            const int par = (t0 + j) & 1;                // the slot of frame t is written again at t + 2, behind frame t + 1's barrier
            if (lane == 63) xch[par][wave] = a[NS - 1];
            __syncthreads();
            // the previous thread's last state (its last but one is never needed: state i * NS is a blank state)
            float p1 = __shfl_up(a[NS - 1], 1);
            if (lane == 0) p1 = wave ? xch[par][wave - 1] : AL_NEG;
            uint32_t w[2] = {0, 0};                      // states 0..15 and 16..31 of the thread
            // in place from the highest register down: a[k] needs the OLD a[k-1], a[k-2]
#pragma unroll
            for (int k = NS - 1; k >= 0; --k) {
                float best = a[k];
                uint32_t step = 0;
                const float la2 = k >= 1 ? a[k - 1] : p1;
                if (la2 > best) { best = la2; step = 1; }
                if (k & 1) {                             // blank states have no skip transition
                    float la3 = k >= 2 ? a[k - 2] : p1;
                    if (!skip_ok[k >> 1]) la3 = AL_NEG;
                    if (la3 > best) { best = la3; step = 2; }
                }
                a[k] = best + ((k & 1) ? lpv[j][k >> 1] : lpb[j]);
                w[k >> 4] |= step << (2 * (k & 15));
                // the word itself stays live, not the compare masks it is made of (they would fill the scalar registers)
                if ((k & 3) == 0) asm volatile("" : "+v"(w[k >> 4]));
            }
            wv[j] = NS == 32 ? (W)(((uint64_t)w[1] << 32) | w[0]) : (W)w[0];
        }
        if (tid < nthr) {
#pragma unroll
            for (int j = 0; j < TCH; ++j)
                if (t0 + j < T) bp[(size_t)(t0 + j) * nthr + tid] = wv[j];
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = tid * NS + k;
        if (s == S - 1) s_end[0] = a[k];
        if (s == S - 2) s_end[1] = a[k];
    }
    // bp: written to HBM by every wave, read below by wave 0 -- released to the device's L2 before the barrier, this CU's
    // vector cache dropped behind it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const float v_last = s_end[0], v_prev = s_end[1];
    const float score = v_last >= v_prev ? v_last : v_prev;
    const bool ok = !(score < -1e29f);
    if (ok && wave == 0) {
        int s = __builtin_amdgcn_readfirstlane(v_last >= v_prev ? S - 1 : S - 2);
        if (lane == 0 && (s & 1)) {
            last[s >> 1] = T - 1;
            if (T == 1) first[s >> 1] = 0;
        }
        // A scalar chain (state -> owner thread -> its word -> step).  The state of frame t1 - 1 - j goes into lane j of one
        // register; a token's last frame is where the next frame's state differs, its first frame where the previous one's does.
        int owner = s / NS, k = s - owner * NS;
        for (int t1 = T - 1; t1 >= 1; t1 -= BCH) {
            const int s_in = s, owner0 = owner;
            const int thr = owner0 - lane > 0 ? owner0 - lane : 0;
            uint32_t wl[BCH], wh[BCH];
            // (the row stride lives in a vector register: with a uniform one the compiler keeps a scalar base pair per
            // load of the chunk alive and runs out of scalar registers)
            int stride = nthr;
            asm volatile("" : "+v"(stride));
            const W *p = bp + (size_t)t1 * nthr + thr;
#pragma unroll
            for (int j = 0; j < BCH; ++j) {
                const W x = *p;
                if (t1 - j > 1) p -= stride;
                wl[j] = (uint32_t)x;
                wh[j] = NS == 32 ? (uint32_t)((uint64_t)x >> 32) : 0u;
            }
            int pv = 0;
#pragma unroll
            for (int j = 0; j < BCH; ++j) {
                const int d = owner0 - owner;            // < 64: the chunk's frames move the state by at most 2 * BCH = 32
                uint32_t ww = __builtin_amdgcn_readlane(wl[j], d);
                if (NS == 32) {
                    const uint32_t hh = __builtin_amdgcn_readlane(wh[j], d);
                    ww = k >= 16 ? hh : ww;
                }
                const int step = t1 - j >= 1 ? (int)((ww >> (2 * (k & 15))) & 3u) : 0;   // (behind frame 1 the state stands still: lanes nobody reads)
                s -= step;
                k -= step;
                if (k < 0) { k += NS; owner -= 1; }
                if (s < 0) { s = 0; k = 0; owner = 0; }  // (no table the recursion writes leads here)
                int ln = lane;                           // (opaque: the compare stays here instead of BCH lane masks held across the chunk)
                asm volatile("" : "+v"(ln));
                pv = ln == j ? s : pv;
            }
            const int n = t1 < BCH ? t1 : BCH;
            int nxt = __shfl_up(pv, 1);
            if (lane == 0) nxt = s_in;
            if (lane < n) {
                const int t = t1 - 1 - lane;
                if (nxt != pv) {
                    if (pv & 1) last[pv >> 1] = t;
                    if (nxt & 1) first[nxt >> 1] = t + 1;
                }
                if (t == 0 && (pv & 1)) first[pv >> 1] = 0;
            }
        }
    }
    // first / last: written by wave 0, read by every wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (ok) {
        for (int i = tid; i < L; i += blockDim.x) {
            int f = first[i], l = last[i];               // (the walk writes both for every token; the bounds keep the loads inside the rows regardless)
            const int id = tgt[i];
            f = f < 0 ? 0 : f;
            l = l > T - 1 ? T - 1 : l;
            float sum = 0.f;
#pragma unroll 4
            for (int t = f; t <= l; ++t) sum += lp[(size_t)t * QV_VOCAB + id];
            logp[i] = sum / (float)(l - f + 1);
        }
    }
    if (tid == 0) {
        qv_align_long_info inf;
        inf.n_tokens = L;
        inf.flags = ok ? 0 : QV_ALIGN_INFEASIBLE;
        inf.t_frames = T;
        inf.n_windows = r.n_windows;
        inf.score = ok ? score : 0.f;
        inf.reserved_f = 0.f;
        o_info[blockIdx.x] = inf;
    }
}

template <int NS>
int launch_class(qv_engine *eng, const std::vector<AlRow> &rows, const float *kept, const uint16_t *targets, const AlRow *plan_d,
                 unsigned char *bp, qv_align_long_info *o_info, int32_t *o_first, int32_t *o_last, float *o_logp, int P, hipStream_t stream) {
    int threads = 0;
    for (const AlRow &r : rows)
        if (r.ns == NS) threads = std::max(threads, r.threads);
    if (!threads) return QV_OK;
    hipLaunchKernelGGL(k_align_long<NS>, dim3((unsigned)rows.size()), dim3(threads), 0, stream, kept, targets, plan_d, bp, o_info, o_first,
                       o_last, o_logp, P);
    QV_HIP(hipGetLastError());
    return QV_OK;
}

}  // namespace

void qv_align_long_free(QvAlignLongWs &w) {
    qv_mirror_free(w.m);
    if (w.big) (void)hipFree(w.big);
    w = {};
}

extern "C" int qv_align_long_plan(const int64_t *n_samples, const int32_t *n_tokens, int32_t rows, int32_t max_samples,
                                  int32_t window_samples, int32_t margin_frames, int32_t *n_windows_total, int64_t *bytes) {
    int64_t nw = 0, total = 0;
    const int rc = qv_al_plan_rows(n_samples, n_tokens, rows, max_samples, window_samples, margin_frames, &nw, &total);
    if (rc == QV_LONG_BAD_ARG || (rc == QV_LONG_TOO_LONG && total == 0)) return rc;   // QV_ERR_ARG; QV_ERR_CAPACITY above QV_LONG_MAX_FRAMES
    if (n_windows_total) *n_windows_total = (int32_t)std::min<int64_t>(nw, INT32_MAX);
    if (bytes) *bytes = total;
    return rc;
}

// audio != nullptr: cut, forward, keep, align (qv_align_long).  audio == nullptr: the caller's window log-probs
// lp_in f32[*, t_max_in, 1025] (qv_align_windows).  Everything is checked before the first allocation or launch and before an
// output array is written.  SYNCHRONOUS on `stream`.
int qv_align_long_run(qv_engine *eng, QvCtx &c, const float *audio, int64_t audio_pitch, const float *lp_in, int t_max_in,
                      const int64_t *n_host, int rows, int window_samples, int margin_frames, const uint16_t *targets_host,
                      const int32_t *lens_host, qv_align_long_info *info_host, int32_t *first_host, int32_t *last_host,
                      float *logp_host, int pitch, hipStream_t stream) {
    const std::string who = audio ? "qv_align_long" : "qv_align_windows";
    QvLongCall call;
    QV_TRY_RC(qv_long_check(eng, who.c_str(), c, audio, audio_pitch, t_max_in, n_host, rows, window_samples, margin_frames, call));
    int l_top = 0;
    size_t total = 0;
    for (int r = 0; r < rows; ++r) {
        if (lens_host[r] < 0) { qv_set_error(eng, who + ": lens_host[r] is negative"); return QV_ERR_ARG; }
        l_top = std::max(l_top, lens_host[r]);
        total += (size_t)lens_host[r];
    }
    if (pitch < l_top) { qv_set_error(eng, who + ": pitch smaller than the longest target"); return QV_ERR_ARG; }
    if (total > 0 && !targets_host) { qv_set_error(eng, who + ": targets_host is null"); return QV_ERR_ARG; }
    int64_t nw = 0, bytes = 0;
    const int prc = qv_al_plan_rows(n_host, lens_host, rows, eng->cfg.max_samples, window_samples, margin_frames, &nw, &bytes);
    if (prc) { qv_set_error(eng, who + ": the workspace would exceed QV_ALIGN_LONG_MAX_BYTES"); return QV_ERR_CAPACITY; }

    // the rows: flags the host can decide (no target, too long, fewer frames than the target needs), offsets by the formula
    std::vector<AlRow> plan(rows);
    std::vector<int32_t> flags(rows, 0);
    size_t src = 0, n_tg = 0;
    int64_t kept_bytes = 0, bp_bytes = 0;
    bool any = false;
    for (int r = 0; r < rows; ++r) {
        const int L = lens_host[r], T = call.plans[r].t_total;
        AlRow &a = plan[r];
        if (L == 0) flags[r] = QV_ALIGN_NO_TARGET;
        else if (L > QV_ALIGN_LONG_MAX_TOKENS) flags[r] = QV_ALIGN_TOO_LONG;   // (never read)
        else {
            int rep = 0;
            for (int i = 0; i < L; ++i) {
                if (targets_host[src + i] >= QV_BLANK) { qv_set_error(eng, who + ": target id outside 0..1023"); return QV_ERR_ARG; }
                rep += i > 0 && targets_host[src + i] == targets_host[src + i - 1];
            }
            if (T < L + rep) flags[r] = QV_ALIGN_INFEASIBLE;
        }
        a.lp_off = kept_bytes / 4;
        a.bp_off = bp_bytes;
        a.tok_off = (int32_t)n_tg;
        a.L = L;
        a.T = T;
        a.ns = flags[r] ? 0 : qv_al_ns(L);
        a.threads = qv_al_threads(L);
        a.n_windows = call.plans[r].n_windows;
        kept_bytes += qv_al_kept_bytes(T);
        bp_bytes += qv_al_bp_bytes(T, L);
        if (!flags[r]) { n_tg += (size_t)L; any = true; }
        src += (size_t)L;
    }

    const int P = std::max(4, (l_top + 3) & ~3);
    const size_t b_plan = qv_up16((size_t)rows * sizeof(AlRow)), b_dst = qv_up16(call.n_win * sizeof(int64_t)),
                 b_tg = qv_up16(n_tg * sizeof(uint16_t)), b_info = qv_up16((size_t)rows * sizeof(qv_align_long_info)),
                 b_col = (size_t)rows * P * 4, b_up = b_plan + b_dst + b_tg, b_back = b_info + 3 * b_col;
    QvAlignLongWs &w = eng->align_long_ws;
    if (any) {
        call.P = 0;   // (no fid / m / transcript records in the long workspace for this call)
        QV_TRY_RC(qv_long_tables(eng, c, audio != nullptr, audio_pitch, rows, call, stream));
        if (b_up + b_back > w.m.dev_bytes) {
            qv_mirror_free(w.m);
            QV_TRY_RC(qv_mirror_alloc(eng, w.m, b_up + b_back, b_up + b_back, "long alignment workspace"));
        }
        if ((size_t)bytes > w.big_bytes) {
            if (w.big) (void)hipFree(w.big);
            w.big = nullptr;
            w.big_bytes = 0;
            if (hipMalloc((void **)&w.big, (size_t)bytes) != hipSuccess) {
                (void)hipGetLastError();
                qv_set_error(eng, "long alignment workspace: out of memory");
                return QV_ERR_HIP;
            }
            w.big_bytes = (size_t)bytes;
        }
        AlRow *plan_h = (AlRow *)w.m.host;
        int64_t *dst_h = (int64_t *)(w.m.host + b_plan);
        uint16_t *tg_h = (uint16_t *)(w.m.host + b_plan + b_dst);
        memcpy(plan_h, plan.data(), sizeof(AlRow) * rows);
        size_t k = 0;
        src = 0;
        for (int r = 0; r < rows; ++r) {
            const QvLongPlan &p = call.plans[r];
            for (int v = 0; v < p.n_windows; ++v, ++k)
                dst_h[k] = flags[r] ? -1 : plan[r].lp_off + (int64_t)qv_long_lo(p, v) * QV_VOCAB;
            if (!flags[r]) memcpy(tg_h + plan[r].tok_off, targets_host + src, sizeof(uint16_t) * lens_host[r]);
            src += (size_t)lens_host[r];
        }
        QV_HIP(hipMemcpyAsync(w.m.dev, w.m.host, b_up, hipMemcpyHostToDevice, stream));
        const AlRow *plan_d = (const AlRow *)w.m.dev;
        const int64_t *dst_d = (const int64_t *)(w.m.dev + b_plan);
        const uint16_t *tg_d = (const uint16_t *)(w.m.dev + b_plan + b_dst);
        unsigned char *back_d = w.m.dev + b_up, *back_h = w.m.host + b_up;
        float *kept = (float *)w.big;
        unsigned char *bp = w.big + kept_bytes;
        const int64_t most = (int64_t)(call.kw + 1) * QV_VOCAB;   // floats a window owns at most
        const unsigned gx = (unsigned)((2 + (most + 3) / 4 + LK_THREADS - 1) / LK_THREADS);
        QvLongTimer tm = {eng->profile_stages, stream, {}};   // kinds: k_long_keep, k_align_long
        QV_TRY_RC(qv_long_rounds(eng, c, call, audio, audio_pitch, lp_in, t_max_in, stream, nullptr,
                                 [&](const float *lp, int t_max, size_t k0, int nb) -> int {
            tm.mark(0);
            hipLaunchKernelGGL(k_long_keep, dim3(gx, nb), dim3(LK_THREADS), 0, stream, lp, t_max, call.tab_d + k0, dst_d + k0, kept);
            QV_HIP(hipGetLastError());
            tm.mark(0);
            return QV_OK;
        }));
        qv_align_long_info *o_info = (qv_align_long_info *)back_d;
        int32_t *o_first = (int32_t *)(back_d + b_info), *o_last = (int32_t *)(back_d + b_info + b_col);
        float *o_logp = (float *)(back_d + b_info + 2 * b_col);
        tm.mark(1);
        QV_TRY_RC(launch_class<4>(eng, plan, kept, tg_d, plan_d, bp, o_info, o_first, o_last, o_logp, P, stream));
        QV_TRY_RC(launch_class<8>(eng, plan, kept, tg_d, plan_d, bp, o_info, o_first, o_last, o_logp, P, stream));
        QV_TRY_RC(launch_class<16>(eng, plan, kept, tg_d, plan_d, bp, o_info, o_first, o_last, o_logp, P, stream));
        QV_TRY_RC(launch_class<32>(eng, plan, kept, tg_d, plan_d, bp, o_info, o_first, o_last, o_logp, P, stream));
        tm.mark(1);
        QV_TRY_RC(qv_fetch_sync(eng, back_h, back_d, b_back, stream));
        tm.finish(w.kernel_ms);
    }
    // a row flagged here or by the kernel: -1 / 0 in every entry, as behind a row's n_tokens
    const int32_t no_i = -1;
    const float no_f = 0.f;
    for (int r = 0; r < rows; ++r) {
        qv_align_long_info inf = {lens_host[r], flags[r], call.plans[r].t_total, call.plans[r].n_windows, 0.f, 0.f};
        const unsigned char *back_h = w.m.host ? w.m.host + b_up : nullptr;   // (no row ran: no mirror yet)
        if (!flags[r]) memcpy(&inf, back_h + sizeof(qv_align_long_info) * r, sizeof(inf));
        const bool ran = !inf.flags;
        const int n = ran ? inf.n_tokens : 0;
        info_host[r] = inf;
        scatter_column(first_host, pitch, r, ran ? (const int32_t *)(back_h + b_info) + (size_t)r * P : &no_i, n, (int32_t)-1);
        scatter_column(last_host, pitch, r, ran ? (const int32_t *)(back_h + b_info + b_col) + (size_t)r * P : &no_i, n, (int32_t)-1);
        scatter_column(logp_host, pitch, r, ran ? (const float *)(back_h + b_info + 2 * b_col) + (size_t)r * P : &no_f, n, 0.f);
    }
    return QV_OK;
}
