// qv_match_body.inc -- the post-logits kernels that depend on the matching window (the transcript's buffer pitches, LDS arrays,
// the word counts the LCS core is instantiated for): decode into codes and match masks, trigram candidates, full-string LCS +
// fragment scores, hint scores, both span passes, the verse tracker.  qv_match.hip (1,024 characters) and qv_match_wide.hip
// (2,048) define QV_MAXQ, QV_MATCH_NS and QV_MATCH_SET and include this file.  What only the wide set needs is under
// `#if QV_MAXW > 16` or a template argument the default set never instantiates (tools/dev_kernel_diff.py compares two
// libraries kernel by kernel).  Each compilation ends in one QvMatchSet (qv_common.h) for the launchers of qv_postlogits.hip.
#define QV_MAXW (QV_MAXQ / 64)

#include "qv_post_util.h"   // qv_common.h, qv_greedy.h
#include "qv_lcs.h"
#include <type_traits>

namespace QV_MATCH_NS {

// ------------------------------------------------------------------ 1. argmax + decode --
// One 1024-thread block per utterance (three launches in the first version: reset, argmax per frame, decode):
//   all sixteen waves: per-frame argmax with numpy semantics (first maximum), frame ids kept in LDS;
//   wave 0 alone:   CTC collapse, piece expansion into normalised codes, whitespace collapse + strip, spaceless copy,
//                   match masks (c2c-direct/run.py:187-204, shared/normalizer.py) -- a serial, 64-lane job.
// Within that single wave the LDS / global hand-offs between lanes only need the wave's own memory operations to have
// completed (QV_WSYNC, qv_greedy.h), not a block barrier.
#define DEC_WAVES 16
__global__ __launch_bounds__(64 * DEC_WAVES) void k_decode(QvTables tab, QvWork wk, const float *__restrict__ lp, int t_max,
                                                          const int32_t *__restrict__ t_dev) {
    __shared__ uint8_t raw[QV_RAW_CAP];
    __shared__ unsigned long long pm[2][QV_NSYM][QV_MAXW];
    __shared__ int16_t s_fid[QV_FRAME_CAP];
    __shared__ int32_t s_tok[QV_FRAME_CAP];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (b == 0 && tid == 0) { *wk.n_fail = 0; wk.frag_ctr[0] = 0; wk.frag_ctr[1] = 0; wk.frag_ctr[2] = 0; }
    QvUtt &u = wk.utt[b];
    const int T = t_dev[b];
    // a wave takes every 16th frame
    for (int t = wave; t < T; t += DEC_WAVES) {
        float best;
        int bi;
        frame_argmax(lp + ((size_t)b * t_max + t) * QV_VOCAB, lane, best, bi);
        if (lane == 0) s_fid[t] = (int16_t)bi;
    }
    __syncthreads();
    if (wave != 0) return;
    int32_t *greedy = wk.greedy + (size_t)b * wk.t_cap;
    int n_tok = 0;
    for (int base = 0; base < T; base += 64) {
        int t = base + lane;
        int id = -1;
        bool keep = false;
        if (t < T) {
            id = s_fid[t];
            int prev = t > 0 ? s_fid[t - 1] : -1;
            keep = id != prev && id != QV_BLANK;
        }
        int tot, r = wave_rank(keep, lane, tot);
        if (keep) { s_tok[n_tok + r] = id; greedy[n_tok + r] = id; }
        n_tok += tot;
    }
    for (int t = n_tok + lane; t < wk.t_cap; t += 64) greedy[t] = -1;
    QV_WSYNC();
    // piece expansion
    int n_raw = 0;
    bool trunc = false;
    for (int base = 0; base < n_tok; base += 64) {
        int k = base + lane;
        int id = k < n_tok ? s_tok[k] : -1;
        int len = id >= 0 ? (int)(tab.piece_off[id + 1] - tab.piece_off[id]) : 0;
        int incl = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            int x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        int off = n_raw + incl - len;
        if (off + len > QV_RAW_CAP) { trunc = true; len = 0; }
        const uint8_t *src = tab.piece_codes + (id >= 0 ? tab.piece_off[id] : 0);
        for (int i = 0; i < len; ++i) raw[off + i] = src[i];
        n_raw += __shfl(incl, 63);
    }
    trunc = __any(trunc);
    if (n_raw > QV_RAW_CAP) n_raw = QV_RAW_CAP;
    QV_WSYNC();
    int last_ns = -1;
    for (int i = lane; i < n_raw; i += 64)
        if (raw[i] != 0) last_ns = i;
    last_ns = wave_max_i(last_ns);
    uint8_t *q = wk.q + (size_t)b * QV_MAXQ, *qs = wk.qs + (size_t)b * QV_MAXQ;
    // the collapsed codes go to HBM (every later kernel reads them there) and, for the match masks below, stay in
    // registers of the lane that produced them
    unsigned long long *pmf = &pm[0][0][0];
    for (int i = lane; i < 2 * QV_NSYM * QV_MAXW; i += 64) pmf[i] = 0ull;
    QV_WSYNC();
    int qn = 0, qsn = 0, spaces = 0;
    for (int base = 0; base < n_raw; base += 64) {
        int i = base + lane;
        int c = i < n_raw ? raw[i] : 0;
        bool keep = i < n_raw && (c != 0 ? true : (i > 0 && raw[i - 1] != 0 && i < last_ns));
        int tot, r = wave_rank(keep, lane, tot);
        if (keep && qn + r < QV_MAXQ) {
            q[qn + r] = (uint8_t)c;
            if (c < QV_NSYM) atomicOr(&pm[0][c][(qn + r) >> 6], 1ull << ((qn + r) & 63));
        }
        bool ks = keep && c != 0;
        int tots, rs = wave_rank(ks, lane, tots);
        if (ks && qsn + rs < QV_MAXQ) {
            qs[qsn + rs] = (uint8_t)c;
            if (c < QV_NSYM) atomicOr(&pm[1][c][(qsn + rs) >> 6], 1ull << ((qsn + rs) & 63));
        }
        spaces += tot - tots;
        qn += tot;
        qsn += tots;
    }
    if (qn > QV_MAXQ) trunc = true;
    int flags = 0;
    if (trunc) { flags |= QV_FLAG_TRANSCRIPT_TRUNCATED; qn = 0; qsn = 0; }
    else if (qn == 0) flags |= QV_FLAG_EMPTY_TRANSCRIPT;
    QV_WSYNC();
    uint64_t *gpm = wk.pm + (size_t)b * 2 * QV_NSYM * QV_MAXW;
    for (int i = lane; i < 2 * QV_NSYM * QV_MAXW; i += 64) gpm[i] = trunc ? 0ull : pmf[i];
    if (lane == 0) {
        u.t_frames = T;
        u.n_tok = n_tok;
        u.q_len = qn;
        u.qs_len = qsn;
        u.q_words = qn > 0 ? spaces + 1 : 0;
        u.flags = flags;
        u.base_start = -1; u.base_span = 0; u.base_score = 0.0;
        u.use_ctc = 0; u.n_cand = 0; u.win = -1; u.win_norm = 0.f;
        u.n_cand1 = 0; u.full_scan = 0; u.n_runners = 0; u.n_surah20 = 0; u.force_full = 0; u.hint_n = 0;
        u.best1_idx = -1; u.best1_score = 0.0;
    }
}

// debug path: transcript codes already in wk.q (uploaded by the host); build the rest.
__global__ __launch_bounds__(64) void k_prepare_codes(QvWork wk, int n) {
    __shared__ unsigned long long pm[2][QV_NSYM][QV_MAXW];
    int lane = threadIdx.x;
    QvUtt &u = wk.utt[0];
    uint8_t *q = wk.q, *qs = wk.qs;
    int qsn = 0, spaces = 0;
    for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        int c = i < n ? q[i] : 0;
        bool ks = i < n && c != 0;
        int tot, r = wave_rank(ks, lane, tot);
        if (ks) qs[qsn + r] = (uint8_t)c;
        qsn += tot;
        int ts;
        wave_rank(i < n && c == 0, lane, ts);
        spaces += ts;
    }
    unsigned long long *pmf = &pm[0][0][0];
    for (int i = lane; i < 2 * QV_NSYM * QV_MAXW; i += 64) pmf[i] = 0ull;
    __syncthreads();
    for (int i = lane; i < n; i += 64) { int c = q[i]; if (c < QV_NSYM) atomicOr(&pm[0][c][i >> 6], 1ull << (i & 63)); }
    for (int i = lane; i < qsn; i += 64) { int c = qs[i]; if (c < QV_NSYM) atomicOr(&pm[1][c][i >> 6], 1ull << (i & 63)); }
    __syncthreads();
    for (int i = lane; i < 2 * QV_NSYM * QV_MAXW; i += 64) wk.pm[i] = pmf[i];
    if (lane == 0) {
        u.t_frames = 0; u.n_tok = 0; u.q_len = n; u.qs_len = qsn; u.q_words = n > 0 ? spaces + 1 : 0;
        u.flags = n == 0 ? QV_FLAG_EMPTY_TRANSCRIPT : 0;
        u.base_start = -1; u.base_span = 0; u.base_score = 0.0;
        u.use_ctc = 0; u.n_cand = 0; u.win = -1; u.win_norm = 0.f;
        u.n_cand1 = 0; u.full_scan = 0; u.n_runners = 0; u.n_surah20 = 0; u.best1_idx = -1; u.best1_score = 0.0;
        u.force_full = 0; u.hint_n = 0;
    }
}

// ------------------------------------------------------------------ 3. trigram top-50 --
#define TRI_WORDS 352  // >= ceil(10243/32), multiple of 32

// _trigram_candidates (quran_db.py:173-186) + the candidate-set rule of match_verse (:278-288),
// one block per utterance.  The transcript's distinct trigram ids are collected in a bitmap and
// compacted in ascending order; then the INVERTED index is walked: for every query trigram, in
// ascending id (= the canonical summation order), its IDF is added to the fp64 score of every
// verse of its posting list.  The per-verse scores live in LDS; wave w owns quarter w of the verse
// range (posting lists are verse-sorted and carry the four slice starts), so no two waves ever
// touch the same score and the loop needs no block barrier.  Work is sum(df) over the query's
// trigrams instead of a scan of all 420k forward postings per utterance.  Then: fewer than 20
// touched verses -> full scan; else the 50 highest sums, iterated in CPython set order.
__global__ __launch_bounds__(256) void k_trigram(QvTables tab, QvWork wk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *score = (double *)smem;                            // [N]
    double *sh_s = (double *)(score + tab.n_verses);           // [8]
    unsigned long long *sh_k = (unsigned long long *)(sh_s + 8);  // [8]
    int32_t *top = (int32_t *)(sh_k + 8);                      // [64]
    int32_t *tabA = top + 64;                                  // [256]
    int32_t *tabB = tabA + 256;                                // [256]
    uint32_t *tri_scratch = (uint32_t *)(tabB + 256);          // [272]
    double *sel_s = (double *)(tri_scratch + 272);             // [64]
    double *ord_s = sel_s + 64;                                // [64]
    int32_t *sel_p = (int32_t *)(ord_s + 64);                  // [64]
    uint32_t *bits = (uint32_t *)(sel_p + 64);                 // [TRI_WORDS]
    uint16_t *ids = (uint16_t *)(bits + TRI_WORDS);            // [QV_MAXQ]
    int32_t *cnt = (int32_t *)(ids + QV_MAXQ);                 // [8]: [0] number of ids, [1..4] touched per wave
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    QvUtt &u = wk.utt[b];
    const int m = u.q_len, N = tab.n_verses;
    if (m == 0) return;
    int32_t *cand1 = wk.cand1 + (size_t)b * N;
    if (u.force_full) {  // match_verse(use_trigram_index=False): every verse, in verse order
        for (int v = tid; v < N; v += 256) cand1[v] = v;
        if (tid == 0) { u.n_cand1 = N; u.full_scan = 1; }
        return;
    }
    for (int v = tid; v < N; v += 256) score[v] = -1.0;        // -1 = not touched
    for (int i = tid; i < TRI_WORDS; i += 256) bits[i] = 0;
    __syncthreads();
    const uint8_t *q = wk.q + (size_t)b * QV_MAXQ;
    for (int i = tid; i + 2 < m; i += 256) {
        // codes are < 64 (63 = outside the alphabet, never part of an indexed trigram)
        uint32_t key = ((uint32_t)q[i] << 12) | ((uint32_t)q[i + 1] << 6) | q[i + 2];
        int id = tab.tri_map[key];
        if (id == 0xFFFF) id = -1;
        if (id >= 0) atomicOr(&bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    if (wave == 0) {                                            // ascending list of the distinct ids
        int running = 0;
        for (int base = 0; base < TRI_WORDS; base += 64) {
            uint32_t w = base + lane < TRI_WORDS ? bits[base + lane] : 0u;
            int c = __popc(w), incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { int x = __shfl_up(incl, o); if (lane >= o) incl += x; }
            int pos = running + incl - c;
            while (w) { int bit = __ffs(w) - 1; w &= w - 1; ids[pos++] = (uint16_t)((base + lane) * 32 + bit); }
            running += __shfl(incl, 63);
        }
        if (lane == 0) cnt[0] = running;
    }
    __syncthreads();
    const int n_ids = cnt[0];
    for (int k0 = 0; k0 < n_ids; k0 += 64) {
        // this chunk's list bounds and IDFs: one memory round trip for 64 trigrams
        uint32_t P0 = 0, P1 = 0;
        double IDF = 0.0;
        if (k0 + lane < n_ids) {
            int id = ids[k0 + lane];
            P0 = tab.tri_slice[(size_t)id * 5 + wave];
            P1 = tab.tri_slice[(size_t)id * 5 + wave + 1];
            IDF = tab.tri_idf[id];
        }
        const int nchunk = n_ids - k0 < 64 ? n_ids - k0 : 64;
        for (int j0 = 0; j0 < nchunk; j0 += 8) {
            // the first 64 verses of 8 consecutive lists are requested together, then applied in list order
            int vv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                uint32_t p0 = __shfl(P0, (j0 + e) & 63), p1 = __shfl(P1, (j0 + e) & 63);
                vv[e] = (j0 + e < nchunk && p0 + lane < p1) ? (int)tab.tri_post[p0 + lane] : -1;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (j0 + e >= nchunk) break;
                const double idf = __shfl(IDF, (j0 + e) & 63);
                if (vv[e] >= 0) { double sv = score[vv[e]]; score[vv[e]] = sv < 0.0 ? idf : __dadd_rn(sv, idf); }
                uint32_t p0 = __shfl(P0, (j0 + e) & 63), p1 = __shfl(P1, (j0 + e) & 63);
                for (uint32_t base = p0 + 64; base < p1; base += 512) {   // long lists (frequent trigrams), 8 loads in flight
                    int lv[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) {
                        uint32_t p = base + x * 64 + lane;
                        lv[x] = p < p1 ? (int)tab.tri_post[p] : -1;
                    }
#pragma unroll
                    for (int x = 0; x < 8; ++x)
                        if (lv[x] >= 0) { double sv = score[lv[x]]; score[lv[x]] = sv < 0.0 ? idf : __dadd_rn(sv, idf); }
                }
            }
        }
    }
    __syncthreads();
    int local = 0;
    for (int v = tid; v < N; v += 256) local += score[v] >= 0.0;
    local = wave_sum_i(local);
    if (lane == 0) cnt[1 + wave] = local;
    __syncthreads();
    const int touched_total = cnt[1] + cnt[2] + cnt[3] + cnt[4];
    if (touched_total < 20) {  // quran_db.py:285-286
        for (int v = tid; v < N; v += 256) cand1[v] = v;
        if (tid == 0) { u.n_cand1 = N; u.full_scan = 1; }
        return;
    }
    int K = touched_total < 50 ? touched_total : 50;
    block_topk_select(score, N, K, tri_scratch, sel_p, sel_s, top, ord_s);
    if (tid == 0) {
        int n = pyset_order(top, K, cand1, tabA, tabB);
        u.n_cand1 = n;
        u.full_scan = 0;
    }
}

// ------------------------------------------------------------------ 4. fragment score --
// quran_db.py:211-237 (_fragment_score) with partial_ratio (:10-28) inlined.  One wave per
// (utterance, verse text).  mode 0: texts of the pass-1 iteration list; mode 1: every text
// of every gate-failed utterance (search()).
#define FRAG_DIRECT_MAX 128   // up to two rounds of windows: evaluate them all
#ifndef FRAG_STEP
#define FRAG_STEP 4          // anchor spacing of the coarse pass (power of two, >= 4)
#endif
#if QV_MAXW > 16
// wide window: up to 2,048 windows of a verse-sized pattern over the transcript -- 514 anchors, then the refine list
#define FRAG_LIST_OFF 520
#define FRAG_SCRATCH (FRAG_LIST_OFF + QV_MAXQ)
#else
#define FRAG_SCRATCH 2112      // int16 per wave: anchors [QV_MAXQ / 4 + 2] + refine list [QV_MAXQ]
#define FRAG_LIST_OFF (FRAG_SCRATCH / 2)
#endif
#define FRAG_HEAVY 1200       // word-steps per lane above which a window scan counts as expensive (k_lcs_full's two-ended list)
#define FRAG_GRID 1024         // blocks of k_frag (4 waves each): four per CU, the list is consumed by whoever is free
// u64 per symbol row of the wave's LDS copy of the pattern masks (odd: rows spread over the banks).  The pattern of a window
// scan is the SHORTER string, i.e. never longer than the longest verse text (QV_MAX_VW = 11 words): the slice does not grow
// with the window, only the scratch lists do (4 waves: 22.3 KB of masks + 20.5 KB of lists at 2,048, three blocks per CU).
#define FRAG_PM_STRIDE 17
static_assert(FRAG_PM_STRIDE > QV_MAX_VW, "k_frag's mask slice holds a verse-sized pattern");
__device__ __forceinline__ void frag_job(const QvTables &tab, const QvWork &wk, int b, int v, int variant, int lane, int16_t *scratch, uint64_t *lpm) {
    const QvUtt &u = wk.utt[b];
    double *out = wk.fs + ((size_t)b * tab.n_verses + v) * 3 + variant;
    if (variant == 2 && tab.nobsm_len[v] == 0) { if (lane == 0) *out = -1.0; return; }
    TextRef t = text_of(tab, v, variant);
    int m = u.q_len, n = t.n, qw = u.q_words, vw = t.nw;
    const uint8_t *q = wk.q + (size_t)b * QV_MAXQ;
    // " text " in " verse "  (word-boundary substring)
    bool sub = false;
    if (qw >= 3 && m <= n && wk.lcsf[((size_t)b * tab.n_verses + v) * 3 + variant] == m) {   // (needs LCS == m, see k_lcs_full)
        for (int i = lane; i + m <= n && !sub; i += 64) {
            if (i > 0 && t.p[i - 1] != 0) continue;
            if (i + m < n && t.p[i + m] != 0) continue;
            bool ok = true;
            for (int k = 0; k < m; ++k)
                if (q[k] != t.p[i + k] || q[k] >= QV_NSYM) { ok = false; break; }
            sub = ok;
        }
        sub = __any(sub);
    }
    bool windows = !sub && qw >= 4 && vw >= 2;
    // pattern = shorter string, text = (windows of) the longer one
    const uint64_t *pm;
    int stride, s, L;
    const uint8_t *lt;
    if (m <= n) { pm = wk.pm + (size_t)b * 2 * QV_NSYM * QV_MAXW; stride = QV_MAXW; s = m; lt = t.p; L = n; }
    else { pm = tab.pmv + tab.pmv_off[t.tid]; stride = qv_tmpl_w((n + 63) >> 6); s = n; lt = q; L = m; }
    int W = (s + 63) >> 6;
    int nwin = windows ? (L - s + 1) : 0;
    // full-string LCS comes from k_lcs_full (one text per lane); lanes here = sliding windows
    int full = wk.lcsf[((size_t)b * tab.n_verses + v) * 3 + variant], best = 0;
    // Only the maximum over the windows matters, and sliding the window by one position drops one
    // character and appends one, so LCS(w + d) <= LCS(w) + d.  With many windows, pass 0 evaluates
    // every 4th window (and the last one) and takes their maximum B; pass 1 evaluates exactly only
    // the windows whose bound from BOTH neighbouring anchors still exceeds B.  The result is the
    // exact maximum.  Up to FRAG_DIRECT_MAX windows are simply all evaluated in pass 0.
    // The window maximum only enters the score through blend(best), which is monotone in best and
    // never below the full-string ratio fr; and no window can beat the full string: best <= full.
    // If even blend(min(full, s)) == fr the windows cannot change the result and are skipped (the
    // usual case for a verse shorter than the transcript, whose word-count penalty outweighs any
    // window gain).  Otherwise the scan starts from the largest value that still blends to fr.
    const double fr = ratio_from(full, m, n);
    double pen = __ddiv_rn((double)vw, (double)(qw > 1 ? qw : 1));
    if (pen > 1.0) pen = 1.0;
    auto blend = [&](int x) -> double {
        double frag = ratio_from(x, s, s);
        if (!(frag > fr)) return fr;
        double blended = __dadd_rn(__dmul_rn(0.25, fr), __dmul_rn(__dmul_rn(0.75, frag), pen));
        return fr > blended ? fr : blended;
    };
    if (nwin > 0) {
        int ub = full < s ? full : s;
        if (blend(ub) == fr) nwin = 0;
        else if (nwin > FRAG_DIRECT_MAX) {
            int x = (int)(__ddiv_rn(fr, pen) * (double)s);         // estimate, then make it exact
            x = x < 0 ? 0 : (x > ub - 1 ? ub - 1 : x);
            while (x > 0 && blend(x) != fr) --x;
            while (x + 1 < ub && blend(x + 1) == fr) ++x;
            best = x;
        }
    }
    int16_t *cv = scratch, *list = scratch + FRAG_LIST_OFF;
    if (nwin > 0) {
        // Round 6: the pattern's match masks (40 symbols x W words) move into the wave's own LDS slice for the scan (row
        // QV_NSYM of the slice stays all zero: lcs_chunk<W, true>).  Every step of every window reads W mask words of ITS code:
        // ds_read instead of flat gathers over up to 40 global rows, and no select per mask word; the copy costs ~5 loads per
        // lane per item.
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < QV_NSYM * W; i += 64) {
            const int c = i / W, w = i - c * W;
            lpm[c * FRAG_PM_STRIDE + w] = pm[(size_t)c * stride + w];
        }
        QV_WSYNC();
    }
    const bool direct = nwin <= FRAG_DIRECT_MAX;
    const int nco = (nwin + FRAG_STEP - 1) / FRAG_STEP;       // anchors k * FRAG_STEP, k < nco; cv[nco] = last window
    int nlist = direct ? nwin : nco + 1;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = lane; i < nlist; i += 64) {
            int w = pass ? (int)list[i] : (direct ? i : (i < nco ? FRAG_STEP * i : nwin - 1));
            int r = lcs_dispatch<true, QV_MAX_VW>(W, lpm, FRAG_PM_STRIDE, lt + w, s, s);
            if (!pass && !direct) cv[i] = (int16_t)r;
            best = max(best, r);
        }
        best = wave_max_i(best);
        if (direct || pass) break;
        __builtin_amdgcn_wave_barrier();
        nlist = 0;
        for (int base = 0; base < nwin; base += 64) {
            int w = base + lane;
            bool need = false;
            if (w < nwin - 1 && (w & (FRAG_STEP - 1)) != 0) {
                int k0 = w / FRAG_STEP, a1 = FRAG_STEP * (k0 + 1);
                int x0 = cv[k0], x1;
                if (a1 <= nwin - 1) x1 = cv[k0 + 1];
                else { a1 = nwin - 1; x1 = cv[nco]; }
                int ub = min(x0 + (w - FRAG_STEP * k0), x1 + (a1 - w));
                need = ub > best;
            }
            unsigned long long mask = __ballot(need);
            if (need) list[nlist + __popcll(mask & ((1ull << lane) - 1ull))] = (int16_t)w;
            nlist += __popcll(mask);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) {
        double res = fr;
        if (sub) res = fr > 0.98 ? fr : 0.98;
        else if (windows) res = blend(best);
        *out = res;
    }
}

// full-string LCS(transcript, text), one text per lane, pattern = the transcript's match masks, AND everything
// _fragment_score decides before it looks at a single window (quran_db.py:211-237): the word-boundary substring test,
// "fewer than 4 query words / fewer than 2 verse words", and the exact bound "no window can lift the blend above the
// full-string ratio" (frag_job's comment).  Nine texts in ten are final here, one text per LANE; only the rest go on the
// fragment work list that k_frag's waves consume (one text per WAVE, lanes = windows).  The first version ran one wave
// per text for all of them: 64 lanes repeating the same scalar decision for 12,472 texts per gate-failed utterance.
// mode 0: the texts of the pass-1 iteration list; mode 1 (slow-list utterances): clean + alt of every verse for search()
// (skipped when pass 1 already scanned everything) and, as a third job per verse, pass 3's LCS of the spaceless
// transcript against the clean text (c2c-direct/run.py:284-297; a space matches nothing in the spaceless pattern, so
// the spaced text is streamed).
__global__ __launch_bounds__(256) void k_lcs_full(QvTables tab, QvWork wk, int mode) {
    // grid = (utterance, chunk of the job list): the hardware dispatches workgroups x-fastest, and in mode 1 chunk 0 holds
    // every utterance's LONGEST verses (len_order).  With the chunk on x the 64 long blocks were spread over the whole
    // launch and the last of them started when everything else was done; on y they all start first (longest first).
    const int slot = blockIdx.x, chunk = blockIdx.y, nchunk = gridDim.y;
    int b;
    if (mode == 0) b = slot;
    else { if (slot >= *wk.n_fail) return; b = wk.fail_list[slot]; }
    const QvUtt &u = wk.utt[b];
    if (u.q_len == 0) return;
    const int m = u.q_len, ms = u.qs_len, W = (m + 63) >> 6, N = tab.n_verses, qw = u.q_words;
    __shared__ uint64_t spm[2 * QV_PM_ROWS * QV_PMS];
    load_pm_lds(spm, wk.pm + (size_t)b * 2 * QV_NSYM * QV_MAXW);
    const uint64_t *pm = spm;
    const int32_t *cand1 = wk.cand1 + (size_t)b * N;
    int16_t *out = wk.lcsf + (size_t)b * N * 3;
    const bool short_q = qw < 4;
    const uint8_t *q = wk.q + (size_t)b * QV_MAXQ;
    const int lane = threadIdx.x & 63;
    const int jobs = mode == 0 ? u.n_cand1 * 3 : N * 3;
    for (int j = chunk * 256 + threadIdx.x; j < jobs; j += nchunk * 256) {
        int v, variant;
        if (mode == 0) { v = cand1[j / 3]; variant = j % 3; }
        else {
            v = tab.len_order[j / 3];   // similar lengths per wave
            variant = j % 3;
            if (variant == 2) {         // pass 3
                wk.lcs_p3[(size_t)b * N + v] =
                    (int16_t)lcs_dispatch<true>((ms + 63) >> 6, spm + QV_PM_ROWS * QV_PMS, QV_PMS, tab.clean + tab.clean_off[v], tab.clean_len[v], ms);
                continue;
            }
            if (u.full_scan) continue;  // search(): pass 1 already scored every verse
        }
        double *fs = wk.fs + ((size_t)b * N + v) * 3 + variant;
        if (variant == 2 && tab.nobsm_len[v] == 0) { *fs = -1.0; continue; }
        TextRef t = text_of(tab, v, variant);
        const int l = lcs_dispatch<true>(W, pm, QV_PMS, t.p, t.n, m);
        out[v * 3 + variant] = (int16_t)l;
        const int n = t.n, vw = t.nw;
        const double fr = ratio_from(l, m, n);
        bool sub = false;   // " text " in " verse "  (word-boundary substring)
        // (a substring is a common subsequence of full length: only texts with LCS == m are scanned at all)
        if (qw >= 3 && m <= n && l == m) {
            for (int i = 0; i + m <= n && !sub; ++i) {
                if (i > 0 && t.p[i - 1] != 0) continue;
                if (i + m < n && t.p[i + m] != 0) continue;
                bool ok = true;
                for (int k = 0; k < m; ++k)
                    if (q[k] != t.p[i + k] || q[k] >= QV_NSYM) { ok = false; break; }
                sub = ok;
            }
        }
        bool need = false, heavy = false;
        if (sub) *fs = fr > 0.98 ? fr : 0.98;
        else if (short_q || vw < 2) *fs = fr;                 // no windows below 4 query words / 2 verse words
        else {
            const int s = m <= n ? m : n;
            double pen = __ddiv_rn((double)vw, (double)(qw > 1 ? qw : 1));
            if (pen > 1.0) pen = 1.0;
            const int ub = l < s ? l : s;                      // no window beats the full string
            const double frag = ratio_from(ub, s, s);
            double bl = fr;
            if (frag > fr) {
                const double blended = __dadd_rn(__dmul_rn(0.25, fr), __dmul_rn(__dmul_rn(0.75, frag), pen));
                bl = fr > blended ? fr : blended;
            }
            if (bl == fr) *fs = fr;
            else {
                need = true;
                // Round 6: what the scan will cost (rounds of 64 windows x pattern length x words), so that k_frag can start the
                // expensive items first: they go to the FRONT of the list, the cheap ones fill it from the BACK, and the queue is
                // consumed front to back -- the longest scans no longer start when everything else is done
                const int nwin = (m <= n ? n : m) - s + 1, nev = nwin <= FRAG_DIRECT_MAX ? nwin : (nwin + FRAG_STEP - 1) / FRAG_STEP + 1;
                heavy = ((nev + 63) >> 6) * s * ((s + 63) >> 6) >= FRAG_HEAVY;
            }
        }
        // wave-aggregated append to the work list (two ends)
        const unsigned long long mh = __ballot(need && heavy), ml = __ballot(need && !heavy);
        if (need) {
            const unsigned long long mask = heavy ? mh : ml;
            const int leader = __ffsll((long long)mask) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&wk.frag_ctr[heavy ? 0 : 2], __popcll(mask));
            base = __shfl(base, leader);
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            wk.frag_list[heavy ? pos : wk.frag_cap - 1 - pos] = ((uint32_t)b << 15) | ((uint32_t)v << 2) | (uint32_t)variant;
        }
    }
}

// the window scans: one text per wave, taken off the work list k_lcs_full left.  A wave's first item is its own index;
// further ones come from a shared cursor, so the waves of a launch that finds few items leave without an atomic and a
// long text (hundreds of windows of a 16-word pattern) does not hold a fixed share of the list hostage.
__global__ __launch_bounds__(256) void k_frag(QvTables tab, QvWork wk) {
    __shared__ int16_t frag_scratch[4][FRAG_SCRATCH];
    __shared__ uint64_t frag_pm[4][QV_PM_ROWS * FRAG_PM_STRIDE];
    int16_t *scratch = frag_scratch[threadIdx.x >> 6];
    uint64_t *lpm = frag_pm[threadIdx.x >> 6];
    for (int i = threadIdx.x & 63; i < FRAG_PM_STRIDE; i += 64) lpm[QV_NSYM * FRAG_PM_STRIDE + i] = 0ull;   // the all-zero row
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwave = gridDim.x * 4;
    const int n_heavy = wk.frag_ctr[0], n_items = n_heavy + wk.frag_ctr[2];
    int idx = wave;
    while (idx < n_items) {
        const uint32_t it = wk.frag_list[idx < n_heavy ? idx : wk.frag_cap - 1 - (idx - n_heavy)];
        frag_job(tab, wk, (int)(it >> 15), (int)((it >> 2) & 0x1FFFu), (int)(it & 3u), lane, scratch, lpm);
        int nx = 0;
        if (lane == 0) nx = atomicAdd(&wk.frag_ctr[1], 1);
        idx = nwave + __shfl(nx, 0);
    }
}

// ------------------------------------------------------------------ 4b. hint scores ----
// _suffix_prefix_score (quran_db.py:188-208) for the <= 3 verses of the continuation hint, both
// of their texts: the transcript minus its first 1..min(words/2, 4) words against the equally
// long word prefix of the verse.  One lane per (verse, text, trim); pattern = the verse's
// precomputed match masks (a word prefix of the pattern is the low bits of the same masks).
__global__ __launch_bounds__(64) void k_hint_sp(QvTables tab, QvWork wk, int b) {
    QvUtt &u = wk.utt[b];
    const int lane = threadIdx.x, m = u.q_len, qw = u.q_words;
    const uint8_t *q = wk.q + (size_t)b * QV_MAXQ;
    double best = 0.0;
    const int k = lane >> 3, variant = (lane >> 2) & 1, trim = (lane & 3) + 1;   // 3 x 2 x 4 jobs
    const int max_trim = (qw >> 1) < 4 ? (qw >> 1) : 4;
    if (k < u.hint_n && m > 0 && qw >= 2 && trim <= max_trim) {
        const int v = u.hint_v[k];
        TextRef t = text_of(tab, v, variant);
        if (t.nw >= 2) {
            int start = 0, seen = 0;                         // transcript after its first `trim` words
            for (int i = 0; i < m; ++i)
                if (q[i] == 0 && ++seen == trim) { start = i + 1; break; }
            const int nt = qw - trim, pw = nt < t.nw ? nt : t.nw;
            int plen = t.n;
            if (pw < t.nw) {
                seen = 0;
                for (int i = 0; i < t.n; ++i)
                    if (t.p[i] == 0 && ++seen == pw) { plen = i; break; }
            }
            const int ls = m - start;
            const uint64_t *pm = tab.pmv + tab.pmv_off[t.tid];
            int l = lcs_dispatch<false, QV_MAX_VW>((plen + 63) >> 6, pm, qv_tmpl_w((t.n + 63) >> 6), q + start, ls, plen);
            best = ratio_from(l, ls, plen);
        }
    }
    // max over the 8 lanes of a verse
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { double x = __shfl_xor(best, o); if (x > best) best = x; }
    if ((lane & 7) == 0 && k < u.hint_n) u.hint_sp[k] = best;
}

// ------------------------------------------------------------------ 6. span pass -------
// (Measured and rejected, round 3: one START verse per lane with all its spans read off ONE walk over the longest live
// span -- the span texts of a start verse are prefixes of one another and the recurrence walks front to back, lcs_feed /
// lcs_count -- does 3.3x fewer word-steps and reproduces every fixture, but ran 2.4x SLOWER than this kernel at batch 1
// and batch 64 alike (594 vs 235 us, 2,030 vs 840 us), with per-ayah loops, with one loop cut at the boundaries, and with
// the span ends held in registers.  Five times fewer lanes, each carrying the longest chain: the pass is bound by the
// serial add-with-carry chain per lane, and the compiler schedules the plain counted loop below far better.)
// quran_db.py:334-365: every window of 2..max_span ayat of the surahs of the top 20.  One
// span text per lane; texts are contiguous slices of the padded clean array.  A span is
// skipped when even LCS = min(m, n) could not beat the pass-1 best (exact pruning).
__global__ __launch_bounds__(256) void k_spans(QvTables tab, QvWork wk, QvKnobs kn) {
    __shared__ double sh_s[8];
    __shared__ unsigned long long sh_k[8];
    // grid = (block of the utterance's job space, utterance).  (Round 4: the transposed grid that cut k_lcs_full's tail --
    // utterance on x, so that every round of blocks mixes all utterances -- made THIS kernel slower, 738 -> 848 us per
    // launch: its blocks are balanced inside an utterance already, and neighbours then no longer share an utterance's
    // tables in L2.)
    const int b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x, tid = threadIdx.x;
    // pass 1's window scans are done, search()'s have not started: empty the fragment work list
    if (blk == 0 && b == 0 && tid == 0) { wk.frag_ctr[0] = 0; wk.frag_ctr[1] = 0; wk.frag_ctr[2] = 0; }
    const QvUtt &u = wk.utt[b];
    double best = -1.0;
    unsigned long long bkey = ~0ull;
    __shared__ uint64_t spm[2 * QV_PM_ROWS * QV_PMS];
    load_pm_lds(spm, wk.pm + (size_t)b * 2 * QV_NSYM * QV_MAXW);
    if (u.q_len > 0) {
        int m = u.q_len, W = (m + 63) >> 6;
        const uint64_t *pm = spm;
        int per = kn.max_span - 1;
        // One flat job space over the surahs of the top 20, so that every lane of the grid
        // has a span (the surahs are not walked one after the other).  Inside a surah the
        // lanes are span-major - neighbouring lanes hold the same number of ayat starting at
        // consecutive verses, i.e. texts of similar length, which is what bounds a wave.  The
        // tie-break key stays the reference's iteration rank: surahs in order, then start
        // ayah, then span length.
        int cum[21];
        cum[0] = 0;
#pragma unroll
        for (int si = 0; si < 20; ++si)
            cum[si + 1] = cum[si] + (si < u.n_surah20 ? tab.surah_len[u.surah20[si] - 1] * per : 0);
        const int total = cum[20];
        // job g -> (span text, bound check); false = nothing to score (window runs off the surah / cannot beat pass 1)
        auto job = [&](int g, uint32_t &start, int &n, double &bonus, unsigned long long &key) -> bool {
            int si = 0, base = 0;
#pragma unroll
            for (int k = 1; k < 20; ++k)
                if (g >= cum[k]) { si = k; base = cum[k]; }
            int s = u.surah20[si];
            int s0 = tab.surah_start[s - 1], sl = tab.surah_len[s - 1];
            int r = g - base;
            int span = 2 + r / sl, i = r % sl;
            if (i + span > sl) return false;
            int v0 = s0 + i, v1 = v0 + span - 1;
            int nl = tab.nobsm_len[v0];
            start = tab.clean_off[v0] + (nl ? tab.clean_len[v0] - nl : 0);
            n = (int)(tab.clean_off[v1] + tab.clean_len[v1] - start);
            int mn = m < n ? m : n;
            bonus = 0.0;                          // of the span's first verse (quran_db.py:352-353)
            for (int k = 0; k < u.hint_n; ++k)
                if (v0 == u.hint_v[k]) bonus = u.hint_bonus[k];
            double ub = __dadd_rn(ratio_from(mn, m, n), bonus);
            if (!((ub < 1.0 ? ub : 1.0) > u.best1_score)) return false;
            key = (unsigned long long)base + (unsigned long long)(i * per + span - 2);
            return true;
        };
        auto score = [&](int l, int n, double bonus, unsigned long long key) {
            double raw = __dadd_rn(ratio_from(l, m, n), bonus);
            double sc = raw < 1.0 ? raw : 1.0;
            if (better(sc, key, best, bkey)) { best = sc; bkey = key; }
        };
        if (W <= 2) {
            // short transcripts: one span per lane (the chain is at most two words per code)
            for (int g = blk * 256 + tid; g < total; g += nblk * 256) {
                uint32_t start; int n; double bonus; unsigned long long key;
                if (!job(g, start, n, bonus, key)) continue;
                score(lcs_dispatch(W, pm, QV_PMS, tab.clean + start, n, m), n, bonus, key);
            }
        } else {
            // long transcripts: G lanes per span (lcs_systolic).  Every group first walks to its next span that survives
            // the bound -- most do not -- so that the groups of a wave enter the recurrence together.
            auto run = [&](auto g_c) {
                constexpr int G = decltype(g_c)::value;
                const int w = tid & (G - 1), ngroups = nblk * (256 / G);
                for (int g = blk * (256 / G) + tid / G; g < total; g += ngroups) {
                    uint32_t start = 0; int n = 0; double bonus = 0.0; unsigned long long key = 0;
                    bool ok = false;
                    for (; g < total; g += ngroups)
                        if ((ok = job(g, start, n, bonus, key))) break;
                    if (!ok) break;
                    const int l = lcs_systolic<G>(pm, QV_PMS, tab.clean + start, n, m, W, w);
                    if (w == 0) score(l, n, bonus, key);
                }
            };
            if (W <= 4) run(std::integral_constant<int, 4>{});
            else if (W <= 8) run(std::integral_constant<int, 8>{});
#if QV_MAXW > 16
            else if (W > 16) run(std::integral_constant<int, 32>{});   // half a wave per walk, one word per lane
#endif
            else run(std::integral_constant<int, 16>{});
        }
    }
    block_best(best, bkey, sh_s, sh_k);
    if (tid == 0) {
        wk.span_part_score[(size_t)b * QV_SPAN_BLOCKS + blk] = best;
        wk.span_part_key[(size_t)b * QV_SPAN_BLOCKS + blk] = bkey;
    }
}

// ---- k_spans2 (round 5): the span pass with PREFIX SHARING.  The spans that start at verse v0 -- 2, 3, .. max_span ayat --
// are prefixes of one another, and the bit-parallel LCS state after n codes of a text IS the state of its n-code prefix:
// one walk over the longest surviving span of a start verse, with the LCS read off at every ayah end on the way, replaces
// (max_span - 1) walks of 2 + 3 + .. ayat (3.3 x fewer word-steps at max_span = 6).  The walk runs over tab.clean8, where
// every verse is padded to whole 8-code chunks with codes that match nothing, so that an ayah end is a chunk end; a span
// whose first verse loses its bismillah starts inside a chunk and masks the codes in front of it.  Same spans, same
// exact bound, same scores and tie-break keys as k_spans (qv_debug_kernel_variant(2, 0) selects the old kernel;
// tests/test_gpu_postlogits.py compares the two).
__global__ __launch_bounds__(256) void k_spans2(QvTables tab, QvWork wk, QvKnobs kn) {
    __shared__ double sh_s[8];
    __shared__ unsigned long long sh_k[8];
    const int b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x, tid = threadIdx.x;
    // pass 1's window scans are done, search()'s have not started: empty the fragment work list
    if (blk == 0 && b == 0 && tid == 0) { wk.frag_ctr[0] = 0; wk.frag_ctr[1] = 0; wk.frag_ctr[2] = 0; }
    const QvUtt &u = wk.utt[b];
    double best = -1.0;
    unsigned long long bkey = ~0ull;
    __shared__ uint64_t spm[2 * QV_PM_ROWS * QV_PMS];
    load_pm_lds(spm, wk.pm + (size_t)b * 2 * QV_NSYM * QV_MAXW);
    if (u.q_len > 0) {
        const int m = u.q_len, W = (m + 63) >> 6;
        const uint64_t *pm = spm;
        const int per = kn.max_span - 1;
        // job space: one job per START verse of the surahs of the top 20; cum1 counts jobs, cumk the old kernel's
        // (start, span) ranks that the tie-break keys are made of
        int cum1[21];
        cum1[0] = 0;
#pragma unroll
        for (int si = 0; si < 20; ++si) cum1[si + 1] = cum1[si] + (si < u.n_surah20 ? tab.surah_len[u.surah20[si] - 1] : 0);
        const int total = cum1[20];
        auto job = [&](int g, SpanJob &j) -> bool {
            int si = 0, base = 0;
#pragma unroll
            for (int k = 1; k < 20; ++k)
                if (g >= cum1[k]) { si = k; base = cum1[k]; }
            const int s = u.surah20[si];
            const int s0 = tab.surah_start[s - 1], sl = tab.surah_len[s - 1];
            const int i = g - base;
            j.v0 = s0 + i;
            const int nl = tab.nobsm_len[j.v0];
            const uint32_t skip = nl ? tab.clean_len[j.v0] - nl : 0;
            j.start = tab.clean_off[j.v0] + skip;
            j.bonus = 0.0;                        // of the span's first verse (quran_db.py:352-353)
            for (int k = 0; k < u.hint_n; ++k)
                if (j.v0 == u.hint_v[k]) j.bonus = u.hint_bonus[k];
            j.surv = 0; j.emax = 0;
            for (int e = 2; e <= kn.max_span && i + e <= sl; ++e) {
                const int v1 = j.v0 + e - 1;
                const int n = (int)(tab.clean_off[v1] + tab.clean_len[v1] - j.start);
                const int mn = m < n ? m : n;
                const double ub = __dadd_rn(ratio_from(mn, m, n), j.bonus);
                if ((ub < 1.0 ? ub : 1.0) > u.best1_score) { j.surv |= 1u << e; j.emax = e; }
            }
            if (!j.emax) return false;
            const uint32_t s8 = tab.clean8_off[j.v0] + 1 + skip;
            j.a0 = s8 & ~7u;
            j.lead = (int)(s8 - j.a0);
            j.key0 = (unsigned long long)(base * per) + (unsigned long long)(i * per);
            return true;
        };
        auto score = [&](int l, const SpanJob &j, int e) {
            const int v1 = j.v0 + e - 1;
            const int n = (int)(tab.clean_off[v1] + tab.clean_len[v1] - j.start);
            const double raw = __dadd_rn(ratio_from(l, m, n), j.bonus);
            const double sc = raw < 1.0 ? raw : 1.0;
            const unsigned long long key = j.key0 + (unsigned long long)(e - 2);
            if (better(sc, key, best, bkey)) { best = sc; bkey = key; }
        };
        if (W <= 2) {
            // short transcripts: one start verse per lane
            auto walk = [&](auto w_c) {
                constexpr int WW = decltype(w_c)::value;
                for (int g = blk * 256 + tid; g < total; g += nblk * 256) {
                    SpanJob j;
                    if (!job(g, j)) continue;
                    uint64_t V[WW];
#pragma unroll
                    for (int k = 0; k < WW; ++k) V[k] = ~0ull;
                    uint32_t pos = j.a0;
                    uint64_t next = *(const uint64_t *)(tab.clean8 + pos);
                    if (j.lead) next |= (1ull << (8 * j.lead)) - 1ull;
                    for (int e = 1; e <= j.emax; ++e) {
                        const uint32_t end = tab.clean8_off[j.v0 + e];
                        for (; pos < end; pos += 8) {
                            const uint64_t chunk = next;
                            next = *(const uint64_t *)(tab.clean8 + pos + 8);       // (the array is padded by 64 filler codes)
                            lcs_chunk<WW, true>(V, pm, QV_PMS, chunk, 8);
                        }
                        if (j.surv >> e & 1u) score(lcs_count<WW>(V, m), j, e);
                    }
                }
            };
            if (W <= 1) walk(std::integral_constant<int, 1>{});
            else walk(std::integral_constant<int, 2>{});
        } else {
            // long transcripts: G lanes per start verse; every group first walks to its next job that survives the bound,
            // so that the groups of a wave enter the recurrence together
            auto run = [&](auto g_c) {
                constexpr int G = decltype(g_c)::value;
                const int w = tid & (G - 1), ngroups = nblk * (256 / G);
                for (int g = blk * (256 / G) + tid / G; g < total; g += ngroups) {
                    SpanJob j;
                    bool ok = false;
                    for (; g < total; g += ngroups)
                        if ((ok = job(g, j))) break;
                    if (!ok) break;
                    uint64_t snap = lcs_systolic_chunks<G>(pm, QV_PMS, tab.clean8, tab.clean8_off, j, m, W, w);
                    for (int e = 2; e <= j.emax; ++e) {
                        int cnt = (int)((snap >> (7 * (e - 2))) & 0x7F);
#pragma unroll
                        for (int o = G / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
                        if (w == 0 && (j.surv >> e & 1u)) score(cnt, j, e);
                    }
                }
            };
            if (W <= 4) run(std::integral_constant<int, 4>{});
            else if (W <= 8) run(std::integral_constant<int, 8>{});
#if QV_MAXW > 16
            else if (W > 16) run(std::integral_constant<int, 32>{});   // half a wave per walk, one word per lane
#endif
            else run(std::integral_constant<int, 16>{});
        }
    }
    block_best(best, bkey, sh_s, sh_k);
    if (tid == 0) {
        wk.span_part_score[(size_t)b * QV_SPAN_BLOCKS + blk] = best;
        wk.span_part_key[(size_t)b * QV_SPAN_BLOCKS + blk] = bkey;
    }
}

// ------------------------------------------------------------------ 12. verse tracker --
// VerseTracker._find_best_match (shared/verse_tracker.py:67-101) with _score_verse (:41-65)
// inlined.  grid (blocks of 256 verses, texts); the text's match masks are built in LDS by the
// block itself, then one verse per lane: LCS(text, verse) and - when the text has fewer words
// than the verse - LCS(text, first n_text words of the verse), both by streaming the verse
// through the text's bit-vector.  Scores are Python double arithmetic, operation by operation.
__global__ __launch_bounds__(256) void k_track(QvTables tab, QvTrack tw) {
    __shared__ unsigned long long spm[QV_NSYM * QV_PMS];
    __shared__ double sh_s[8];
    __shared__ unsigned long long sh_k[8];
    // grid = (text, chunk of the verse order): chunk 0 = every text's longest verses, dispatched first (see k_lcs_full)
    const int b = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int m = tw.meta[b * 4], n_text = tw.meta[b * 4 + 1], bonus = tw.meta[b * 4 + 2];
    const uint8_t *q = tw.q + tw.meta[b * 4 + 3];
    for (int i = tid; i < QV_NSYM * QV_PMS; i += 256) spm[i] = 0ull;
    __syncthreads();
    for (int i = tid; i < m; i += 256) { int c = q[i]; if (c < QV_NSYM) atomicOr(&spm[c * QV_PMS + (i >> 6)], 1ull << (i & 63)); }
    __syncthreads();
    const int W = (m + 63) >> 6;
    // lanes walk the verses in order of decreasing length, so the 64 verses of a wave cost about
    // the same; the first-maximum rule lives in the key (verse index), not in the visiting order
    const int slot = chunk * 256 + tid;
    const int v = slot < tab.n_verses ? tab.len_order[slot] : -1;
    double best = 0.0;
    unsigned long long bkey = ~0ull;
    if (v >= 0 && m > 0) {
        double score = 0.0;
        int matched_nb = 0;
        const int nl = tab.nobsm_len[v];
        // j: 0 = clean full, 1 = clean prefix, 2 = no_bsm full, 3 = no_bsm prefix (one LCS call site)
        int lfull = 0, n = 0, plen = 0, nwv = 0;
        const uint8_t *p = nullptr;
        for (int j = 0; j < 4; ++j) {
            if (j >= 2 && nl == 0) break;
            if ((j & 1) == 0) {
                n = j == 0 ? tab.clean_len[v] : nl;
                p = tab.clean + tab.clean_off[v] + (j == 0 ? 0 : tab.clean_len[v] - nl);
                nwv = tab.nw[j == 0 ? 0 : 2][v];
                int pw = n_text < nwv ? n_text : nwv;     // prefix = first pw words of the verse
                plen = n;
                if (pw < nwv) {
                    // the no_bsm text is a suffix of the clean text: its words are the clean text's last nwv
                    int drop = tab.nw[0][v] - nwv, shift = tab.clean_len[v] - n;
                    plen = pw > 0 ? (int)tab.wend[tab.wend_off[v] + drop + pw - 1] - shift : 0;
                }
            } else if (plen == n) continue;               // prefix is the whole verse
            int l = lcs_dispatch(W, (const uint64_t *)spm, QV_PMS, p, (j & 1) ? plen : n, m);
            if ((j & 1) == 0) { lfull = l; if (plen != n) continue; }
            double ps = ratio_from(l, m, plen), fs = ratio_from(lfull, m, n);
            double cov = __ddiv_rn((double)n_text, (double)(nwv > 1 ? nwv : 1));
            double raw = cov > 0.8 ? __dadd_rn(__dmul_rn(0.3, ps), __dmul_rn(0.7, fs))
                                   : __dadd_rn(__dmul_rn(0.7, ps), __dmul_rn(0.3, fs));
            if (v == bonus) raw = __dadd_rn(raw, 0.15);
            if (j < 2) score = raw;
            else if (raw > score) { score = raw; matched_nb = 1; }
        }
        best = score;
        bkey = (unsigned long long)v * 2ull + (unsigned long long)matched_nb;
    }
    block_best(best, bkey, sh_s, sh_k);
    if (tid == 0) {
        tw.part_s[(size_t)b * QV_TRACK_BLOCKS + chunk] = best;
        tw.part_k[(size_t)b * QV_TRACK_BLOCKS + chunk] = bkey;
    }
}

#if QV_MAXW > 16
#include "qv_ctc_body.inc"   // the wide set's own k_ctc<true, *>: the recursions inlined, as this set has always had them
#endif

}  // namespace QV_MATCH_NS

static_assert(QV_MAXQ == QV_MAX_TRANSCRIPT || QV_MAXQ == QV_MAX_TRANSCRIPT_WIDE, "a kernel set per window qv_create accepts");
extern const QvMatchSet QV_MATCH_SET = {
    QV_MAXQ, 64 * DEC_WAVES, FRAG_GRID,
    // k_trigram's dynamic LDS behind the N scores (the carve-up at the top of the kernel)
    8 * 8 + 8 * 8 + 64 * 4 + 512 * 4 + 272 * 4 + 128 * 8 + 64 * 4 + TRI_WORDS * 4 + QV_MAXQ * 2 + 8 * 4 + 64,
    QV_MATCH_NS::k_decode, QV_MATCH_NS::k_prepare_codes, QV_MATCH_NS::k_trigram, QV_MATCH_NS::k_frag, QV_MATCH_NS::k_lcs_full,
    QV_MATCH_NS::k_hint_sp, QV_MATCH_NS::k_spans, QV_MATCH_NS::k_spans2, QV_MATCH_NS::k_track,
#if QV_MAXW > 16
    {QV_MATCH_NS::k_ctc<true, 0>, QV_MATCH_NS::k_ctc<true, 1>},
#endif
};
