// qv_postlogits.hip -- everything after the log-probs, on device:
//   argmax -> CTC collapse -> piece expansion + normalisation  (c2c-direct/run.py:187-204)
//   trigram-IDF candidates, fragment scores, span pass          (shared/quran_db.py:173-186,211-237,244-371)
//   search / pass-3 / candidate assembly                        (quran_db.py:92-99; c2c-direct/run.py:251-311)
//   CTC alpha-recursion rerank + decision                       (c2c-direct/run.py:314-380; mixed/run.py:96-133)
//
// Integer/byte work bound by LDS + VALU, not MFMA: the unit of work is a bit-parallel LCS
// (Indel distance) between the transcript and a verse text or text window.  Mapping:
//   * "one text per lane" kernels (pass 3, span pass): pattern = transcript bit-vector (<=16 x
//     64-bit words in VGPRs), each lane streams its own verse/span text.
//   * "one text per wave" kernel (fragment score): lanes = sliding windows of partial_ratio,
//     pattern = the shorter string's match masks, lane 0 additionally does the full-string LCS.
//   * CTC: one wave per (utterance, candidate), 2L+1 states laid contiguously across lanes,
//     two DPP-style shuffles per frame.
// All double arithmetic that feeds comparisons uses explicit _rn intrinsics (no FMA contraction)
// so scores are bit-identical to the reference's Python floats.
//
// This file holds the host launchers and the kernels that never look at the matching window (selection, candidate
// assembly, the CTC family from qv_ctc_body.inc, the decision); it is compiled once.  The kernels that touch the transcript are compiled per
// window from qv_match_body.inc (LCS core: qv_lcs.h), and the launchers below reach them through the engine's QvMatchSet
// (qv_common.h).  Helpers both groups use: qv_post_util.h.

#include "qv_common.h"
#include "qv_graph.h"
#include "qv_greedy.h"
#include "qv_kernels.h"
#include "qv_post_util.h"

#include <math.h>

#include <algorithm>

namespace {

// ------------------------------------------------------------------ 4b. hint (qv_match_verse) --
__global__ void k_set_hint(QvWork wk, int b, int n, int v0, int v1, int v2, double b0, double b1, double b2) {
    QvUtt &u = wk.utt[b];
    u.force_full = 1;
    u.hint_n = n;
    u.hint_v[0] = v0; u.hint_v[1] = v1; u.hint_v[2] = v2;
    u.hint_bonus[0] = b0; u.hint_bonus[1] = b1; u.hint_bonus[2] = b2;
    u.hint_sp[0] = u.hint_sp[1] = u.hint_sp[2] = 0.0;
}

// ------------------------------------------------------------------ 5. pass-1 finalize -
// stable descending sort of min(raw,1.0) in iteration order (quran_db.py:290-331): only the
// first max(top_k,5) entries are ever used, selected by repeated block argmax.
__global__ __launch_bounds__(256) void k_pass1_final(QvTables tab, QvWork wk, QvKnobs kn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *sc = (double *)smem;  // [n_cand1]
    double *sh_s = sc + tab.n_verses;
    unsigned long long *sh_k = (unsigned long long *)(sh_s + 8);
    int b = blockIdx.x, tid = threadIdx.x;
    QvUtt &u = wk.utt[b];
    if (u.q_len == 0) return;
    int n = u.n_cand1, N = tab.n_verses;
    const int32_t *cand1 = wk.cand1 + (size_t)b * N;
    const double *fs = wk.fs + (size_t)b * N * 3;
    for (int p = tid; p < n; p += 256) {
        int v = cand1[p];
        double a = fs[v * 3], c = fs[v * 3 + 1], d = fs[v * 3 + 2];
        double raw = a > c ? a : c;
        if (d > raw) raw = d;
        double bonus = 0.0;                       // continuation hint (quran_db.py:300-311); none on the hot path
        for (int k = 0; k < u.hint_n; ++k)
            if (v == u.hint_v[k]) { if (u.hint_sp[k] > raw) raw = u.hint_sp[k]; bonus = u.hint_bonus[k]; }
        double tot = __dadd_rn(raw, bonus);
        sc[p] = tot < 1.0 ? tot : 1.0;
    }
    __syncthreads();
    int K = kn.top_text > 5 ? kn.top_text : 5;
    if (K > n) K = n;
    if (K > QV_RUNNER_CAP) K = QV_RUNNER_CAP;
    int K20 = n < 20 ? n : 20;
    int rounds = K > K20 ? K : K20;
    int32_t *ridx = wk.runner_idx + (size_t)b * QV_RUNNER_CAP;
    double *rsc = wk.runner_score + (size_t)b * QV_RUNNER_CAP;
    double *sel_s = sh_s;                                 // [128]
    int32_t *sel_p = (int32_t *)(sel_s + QV_RUNNER_CAP);  // [128]
    uint32_t *scratch = (uint32_t *)(sel_p + QV_RUNNER_CAP);  // [272]
    int32_t *ord_p = (int32_t *)(scratch + 272);          // [128]
    double *ord_s = (double *)(ord_p + QV_RUNNER_CAP);    // [128]
    int nsel = block_topk_select(sc, n, rounds, scratch, sel_p, sel_s, ord_p, ord_s);
    for (int r = tid; r < nsel; r += 256) { ridx[r] = cand1[ord_p[r]]; rsc[r] = ord_s[r]; }
    if (tid == 0) {
        u.best1_idx = cand1[ord_p[0]];
        u.best1_score = ord_s[0];
        int ns = 0;
        for (int r = 0; r < K20; ++r) {
            int su = tab.surah[cand1[ord_p[r]]];
            bool seen = false;
            for (int i = 0; i < ns; ++i) seen |= (u.surah20[i] == su);
            if (!seen) u.surah20[ns++] = su;
        }
        u.n_surah20 = ns;
    }
    if (tid == 0) u.n_runners = K < kn.top_text ? K : kn.top_text;
}

__device__ void base_final_one(const QvTables &tab, const QvWork &wk, const QvKnobs &kn, int b, int force_ctc);

// (Measured and rejected: folding this -- and the candidate assembly, and the final decision -- into the tail of the
// kernel in front of it with a "last block done" counter.  Publishing a block's results to a block on another XCD takes an
// agent-scope release, i.e. an L2 write-back per block on this 8-XCD part: k_spans 23 -> 105 us, k_topk 57 -> 108 us,
// k_ctc 143 -> 601 us.  A kernel boundary is the cheap device-wide synchronisation here.)
__global__ void k_base_final(QvTables tab, QvWork wk, QvKnobs kn, int batch, int force_ctc) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) base_final_one(tab, wk, kn, b, force_ctc);
}

// base = better of pass-1 best and span best; gate; result for the text branch.
__device__ void base_final_one(const QvTables &tab, const QvWork &wk, const QvKnobs &kn, int b, int force_ctc) {
    QvUtt &u = wk.utt[b];
    if (u.q_len == 0) return;
    double best = -1.0;
    unsigned long long key = ~0ull;
    for (int i = 0; i < QV_SPAN_BLOCKS; ++i) {
        double s = wk.span_part_score[(size_t)b * QV_SPAN_BLOCKS + i];
        unsigned long long k = wk.span_part_key[(size_t)b * QV_SPAN_BLOCKS + i];
        if (better(s, k, best, key)) { best = s; key = k; }
    }
    u.base_start = u.best1_idx; u.base_span = 1; u.base_score = u.best1_score;
    if (best > u.best1_score) {
        int per = kn.max_span - 1;
        unsigned long long j = key;
        for (int si = 0; si < u.n_surah20; ++si) {
            int s = u.surah20[si];
            unsigned long long jobs = (unsigned long long)tab.surah_len[s - 1] * per;
            if (j < jobs) {
                u.base_start = tab.surah_start[s - 1] + (int)(j / per);
                u.base_span = 2 + (int)(j % per);
                u.base_score = best;
                break;
            }
            j -= jobs;
        }
    }
    u.use_ctc = (u.base_score < kn.threshold) || force_ctc;
    if (u.use_ctc) u.flags |= QV_FLAG_USED_CTC;
    // the "slow list": utterances whose search()/pass-3/candidate stages must run.  With
    // skip_unused == 0 that is every utterance, as in the reference (mixed/run.py:84 precedes
    // the gate at :96); their output is only consumed when use_ctc is set.
    if (u.use_ctc || !kn.skip_unused) {
        int slot = atomicAdd(wk.n_fail, 1);
        wk.fail_list[slot] = b;
    }
}

// ------------------------------------------------------------------ 7. pass 3 ----------
// c2c-direct/run.py:284-297: max(ratio(t, clean), ratio(t.spaceless, clean.spaceless)).  Both LCS values come from
// k_lcs_full (lcsf / lcs_p3); the two ratios and their maximum are formed where they are consumed, in k_topk.
// top-k (score desc, verse index asc) of search() and pass 3
__global__ __launch_bounds__(256) void k_topk(QvTables tab, QvWork wk, QvKnobs kn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *sc = (double *)smem;
    double *sh_s = sc + tab.n_verses;
    unsigned long long *sh_k = (unsigned long long *)(sh_s + 8);
    if ((int)blockIdx.x >= *wk.n_fail) return;
    int b = wk.fail_list[blockIdx.x], which = blockIdx.y, tid = threadIdx.x;
    int N = tab.n_verses;
    if (wk.utt[b].q_len == 0) return;
    if (which == 0) {
        const double *fs = wk.fs + (size_t)b * N * 3;
        for (int v = tid; v < N; v += 256) { double a = fs[v * 3], c = fs[v * 3 + 1]; sc[v] = a > c ? a : c; }
    } else {
        const QvUtt &u = wk.utt[b];
        const int m = u.q_len, ms = u.qs_len;
        for (int v = tid; v < N; v += 256) {
            const int n = tab.clean_len[v], ns = n - (tab.nw[0][v] - 1);
            const double a = ratio_from(wk.lcsf[((size_t)b * N + v) * 3], m, n), c = ratio_from(wk.lcs_p3[(size_t)b * N + v], ms, ns);
            sc[v] = a > c ? a : c;
        }
    }
    __syncthreads();
    int K = kn.top_text < QV_RUNNER_CAP ? kn.top_text : QV_RUNNER_CAP;
    if (K > N) K = N;
    int32_t *oi = (which == 0 ? wk.top_search : wk.top_p3) + (size_t)b * QV_RUNNER_CAP;
    double *os = (which == 0 ? wk.top_search_sc : wk.top_p3_sc) + (size_t)b * QV_RUNNER_CAP;
    double *sel_s = sh_s;                                 // [128]
    int32_t *sel_p = (int32_t *)(sel_s + QV_RUNNER_CAP);  // [128]
    uint32_t *scratch = (uint32_t *)(sel_p + QV_RUNNER_CAP);
    block_topk_select(sc, N, K, scratch, sel_p, sel_s, oi, os);
}


// ------------------------------------------------------------------ 8. candidates ------
// c2c-direct/run.py:251-311: ordered, de-duplicated union + span expansion of the first
#define CAND_PCAP 3072   // proposals before de-duplication: 1 + 3*127 + 128*20 worst case
#define CAND_HT 4096     // open-addressing table (key -> first proposal index)

// Parallel form of the ordered, de-duplicated union: (1) lay out every proposal in reference
// order, (2) a hash table keeps the FIRST proposal index of each (start, span) key, (3) an
// ordered compaction of the proposals that are their key's first occurrence.
__device__ void candidates_block(const QvTables &tab, const QvWork &wk, const QvKnobs &kn, int b, unsigned char *smem) {
    double *pscore = (double *)smem;                       // [CAND_PCAP]
    uint32_t *pkey = (uint32_t *)(pscore + CAND_PCAP);     // [CAND_PCAP]
    uint32_t *htk = pkey + CAND_PCAP;                      // [CAND_HT]
    uint32_t *hti = htk + CAND_HT;                         // [CAND_HT]
    int32_t *refs = (int32_t *)(hti + CAND_HT);            // [128]
    int32_t *roff = refs + 128;                            // [129]
    int32_t *wsum = roff + 132;                            // [8]: 4 wave sums + the leader counter
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    QvUtt &u = wk.utt[b];
    if (u.q_len == 0) return;
    const int N = tab.n_verses;
    int K = kn.top_text < QV_RUNNER_CAP ? kn.top_text : QV_RUNNER_CAP;
    if (K > N) K = N;
    const bool has_base = u.base_start >= 0;
    const int nrun = has_base ? u.n_runners : 0;
    const int nA = (has_base ? 1 : 0) + nrun + 2 * K;      // singles + base, in order
    const int32_t *ri = wk.runner_idx + (size_t)b * QV_RUNNER_CAP;
    const double *rs = wk.runner_score + (size_t)b * QV_RUNNER_CAP;
    const int32_t *si = wk.top_search + (size_t)b * QV_RUNNER_CAP;
    const double *ss = wk.top_search_sc + (size_t)b * QV_RUNNER_CAP;
    const int32_t *pi = wk.top_p3 + (size_t)b * QV_RUNNER_CAP;
    const double *ps = wk.top_p3_sc + (size_t)b * QV_RUNNER_CAP;
    for (int i = tid; i < CAND_HT; i += 256) { htk[i] = 0xFFFFFFFFu; hti[i] = 0xFFFFFFFFu; }
    // segment A + the ref list (first top_span_refs entries of the same sequence)
    const int nrefs = min(min(nA, kn.top_span_refs), 128);
    for (int i = tid; i < nA; i += 256) {
        int j = i, st, sp = 1;
        double sc;
        if (has_base && j == 0) { st = u.base_start; sp = u.base_span; sc = u.base_score; }
        else {
            j -= has_base ? 1 : 0;
            if (j < nrun) { st = ri[j]; sc = py_round3(rs[j]); }
            else if (j < nrun + K) { st = si[j - nrun]; sc = ss[j - nrun]; }
            else { st = pi[j - nrun - K]; sc = ps[j - nrun - K]; }
        }
        pkey[i] = (uint32_t)st * 8u + (uint32_t)sp;
        pscore[i] = sc;
        if (i < nrefs) refs[i] = st;
    }
    __syncthreads();
    // span expansion sizes per ref (c2c-direct/run.py:300-309)
    for (int r = tid; r < nrefs; r += 256) {
        int v = refs[r], s = tab.surah[v], a = tab.ayah[v], max_ayah = tab.surah_len[s - 1];
        int lo = a - kn.max_span + 1; if (lo < 1) lo = 1;
        int hi = a < max_ayah ? a : max_ayah, cnt = 0;
        for (int st = lo; st <= hi; ++st) {
            int e0 = a > st + 1 ? a : st + 1;
            int e1 = st + kn.max_span - 1; if (e1 > max_ayah) e1 = max_ayah;
            if (e1 >= e0) cnt += e1 - e0 + 1;
        }
        roff[r + 1] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        roff[0] = nA;
        for (int r = 0; r < nrefs; ++r) roff[r + 1] += roff[r];
    }
    __syncthreads();
    int nP = roff[nrefs];
    bool overflow = nP > CAND_PCAP;
    if (overflow) nP = CAND_PCAP;
    for (int r = tid; r < nrefs; r += 256) {
        int v = refs[r], s = tab.surah[v], a = tab.ayah[v];
        int s0 = tab.surah_start[s - 1], max_ayah = tab.surah_len[s - 1];
        int lo = a - kn.max_span + 1; if (lo < 1) lo = 1;
        int hi = a < max_ayah ? a : max_ayah, o = roff[r];
        for (int st = lo; st <= hi; ++st) {
            int e0 = a > st + 1 ? a : st + 1;
            int e1 = st + kn.max_span - 1; if (e1 > max_ayah) e1 = max_ayah;
            for (int en = e0; en <= e1; ++en, ++o)
                if (o < CAND_PCAP) { pkey[o] = (uint32_t)(s0 + st - 1) * 8u + (uint32_t)(en - st + 1); pscore[o] = 0.0; }
        }
    }
    __syncthreads();
    // first occurrence per key
    for (int i = tid; i < nP; i += 256) {
        uint32_t key = pkey[i], slot = (key * 2654435761u) >> 20;  // 12 bits
        for (;;) {
            uint32_t old = atomicCAS(&htk[slot], 0xFFFFFFFFu, key);
            if (old == 0xFFFFFFFFu || old == key) { atomicMin(&hti[slot], (uint32_t)i); break; }
            slot = (slot + 1) & (CAND_HT - 1);
        }
    }
    __syncthreads();
    // ordered compaction: thread t owns proposals [t*per, (t+1)*per)
    const int per = (nP + 255) / 256;
    int i0 = tid * per, i1 = min(nP, i0 + per), cnt = 0;
    unsigned keepmask = 0;  // per <= 12
    for (int i = i0; i < i1; ++i) {
        uint32_t key = pkey[i], slot = (key * 2654435761u) >> 20;
        while (htk[slot] != key) slot = (slot + 1) & (CAND_HT - 1);
        if (hti[slot] == (uint32_t)i) { keepmask |= 1u << (i - i0); ++cnt; }
    }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = incl - cnt;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    int32_t *cs = wk.cand_start + (size_t)b * QV_CAND_CAP;
    int32_t *cp = wk.cand_span + (size_t)b * QV_CAND_CAP;
    double *csc = wk.cand_score + (size_t)b * QV_CAND_CAP;
    for (int i = i0; i < i1; ++i) {
        if (!(keepmask >> (i - i0) & 1u)) continue;
        if (base < QV_CAND_CAP) {
            cs[base] = (int32_t)(pkey[i] >> 3); cp[base] = (int32_t)(pkey[i] & 7u); csc[base] = pscore[i];
            // the table now maps a key to its CANDIDATE index (every keepmask loop is behind the barrier above)
            uint32_t key = pkey[i], slot = (key * 2654435761u) >> 20;
            while (htk[slot] != key) slot = (slot + 1) & (CAND_HT - 1);
            hti[slot] = (uint32_t)base;
        } else {
            uint32_t key = pkey[i], slot = (key * 2654435761u) >> 20;
            while (htk[slot] != key) slot = (slot + 1) & (CAND_HT - 1);
            hti[slot] = 0xFFFFFFFFu;
        }
        ++base;
    }
    const int ncand = total < QV_CAND_CAP ? total : QV_CAND_CAP;
    if (tid == 0) {
        u.n_cand = ncand;
        if (overflow || total > QV_CAND_CAP) u.flags |= QV_FLAG_CAND_OVERFLOW;
    }
    // ---- plan of the CTC rerank: which candidates run an alpha recursion ----------------------------------
    // The alpha values of the states 0..2P of a target do not depend on what follows its first P tokens, so
    // ONE recursion over the ids of (start, span k') also yields the loss of every (start, span k < k') whose
    // ids are a prefix of them (tok_pfx): read alpha_T at the states 2P and 2P - 1.  A candidate's leader is
    // the feasible candidate with the same start verse and the largest span its ids are a prefix of; only
    // leaders run (k_ctc), each writes the losses of its members.  Same arithmetic per state as a recursion
    // of its own: the results are bit-identical, the work drops by the sharing factor (windows around a
    // reference verse share their start verse up to max_span - 1 times).
    int32_t *nlead = wsum + 4;
    if (tid == 0) *nlead = 0;
    int16_t *lead = wk.cand_lead + (size_t)b * QV_CAND_CAP;
    int16_t *memb = wk.cand_memb + (size_t)b * QV_CAND_CAP * QV_MAX_SPAN;
    float *closs = wk.cand_loss + (size_t)b * QV_CAND_CAP;
    double *cfin = wk.cand_final + (size_t)b * QV_CAND_CAP;
    for (int i = tid; i < ncand * QV_MAX_SPAN; i += 256) memb[i] = -1;
    __syncthreads();
    const int T = u.t_frames, scap = wk.t_cap > 384 ? 768 : 384;
    for (int c = tid; c < ncand; c += 256) {
        const int st = cs[c], sp = cp[c];
        const size_t k0 = (size_t)st * QV_MAX_SPAN;
        const int L = (int)(tab.tok_off[k0 + sp] - tab.tok_off[k0 + sp - 1]);
        if (!(L > 0 && 2 * L + 1 <= T && 2 * L + 1 <= scap)) {     // gate of c2c-direct/run.py:332: no loss
            closs[c] = INFINITY;
            cfin[c] = -INFINITY;
            continue;
        }
        int leader = c;
        const unsigned chain = tab.tok_pfx[st];
        for (int k = kn.max_span; k > sp; --k) {
            const unsigned need = ((1u << (k - 1)) - 1u) & ~((1u << (sp - 1)) - 1u);   // flags sp .. k - 1
            if ((chain & need) != need) continue;
            const int Lk = (int)(tab.tok_off[k0 + k] - tab.tok_off[k0 + k - 1]);
            if (!(2 * Lk + 1 <= T && 2 * Lk + 1 <= scap)) continue;
            uint32_t key = (uint32_t)st * 8u + (uint32_t)k, slot = (key * 2654435761u) >> 20;
            while (htk[slot] != key && htk[slot] != 0xFFFFFFFFu) slot = (slot + 1) & (CAND_HT - 1);
            if (htk[slot] != key || hti[slot] == 0xFFFFFFFFu) continue;
            leader = (int)hti[slot];
            break;
        }
        if (leader == c) lead[atomicAdd(nlead, 1)] = (int16_t)c;
        else memb[(size_t)leader * QV_MAX_SPAN + sp - 1] = (int16_t)c;
    }
    __syncthreads();
    // Round 6: the leaders in order of DECREASING state count (64-state buckets).  k_ctc hands leader i to wave i mod 256 of the
    // utterance: with ~400 leaders of 64 ... 448 states in arbitrary order, a wave could draw two long recursions and another two
    // short ones; sorted, the waves that take a second leader take the SHORTEST ones.  The order changes no loss.
    {
        const int nl = *nlead;
        int32_t *bcnt = (int32_t *)pscore;                 // [16] bucket counts, then [16] bucket offsets (pscore is dead by now)
        int16_t *tmp = (int16_t *)(bcnt + 32);             // [QV_CAND_CAP]
        if (tid < 32) bcnt[tid] = 0;
        __syncthreads();
        int bk[QV_CAND_CAP / 256], ps[QV_CAND_CAP / 256];
#pragma unroll
        for (int j = 0; j < QV_CAND_CAP / 256; ++j) {
            const int i = tid + j * 256;
            bk[j] = -1;
            if (i < nl) {
                const int c = lead[i], st = cs[c], sp = cp[c];
                const size_t k0 = (size_t)st * QV_MAX_SPAN;
                const int L = (int)(tab.tok_off[k0 + sp] - tab.tok_off[k0 + sp - 1]);
                bk[j] = 15 - min(15, L >> 5);             // bucket 0 = the longest targets
                ps[j] = atomicAdd(&bcnt[bk[j]], 1);
            }
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int k = 0; k < 16; ++k) { bcnt[16 + k] = run; run += bcnt[k]; }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < QV_CAND_CAP / 256; ++j)
            if (bk[j] >= 0) tmp[bcnt[16 + bk[j]] + ps[j]] = lead[tid + j * 256];
        __syncthreads();
        for (int i = tid; i < nl; i += 256) lead[i] = tmp[i];
        if (tid == 0) u.n_lead = nl;
    }
}

__global__ __launch_bounds__(256) void k_candidates(QvTables tab, QvWork wk, QvKnobs kn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if ((int)blockIdx.x >= *wk.n_fail) return;
    candidates_block(tab, wk, kn, wk.fail_list[blockIdx.x], smem);
}

#include "qv_ctc_body.inc"   // 9. CTC: ctc_wave, ctc_wave2, ctc_dispatch, k_ctc<LONG, VAR>

template <int VAR>
__global__ __launch_bounds__(64) void k_ctc_debug(const float *__restrict__ lp, int T, const uint16_t *__restrict__ tg,
                                                  const int32_t *__restrict__ off, int n, float *__restrict__ loss) {
    __shared__ float sa[768];
    int c = blockIdx.x, lane = threadIdx.x;
    if (c >= n) return;
    int L = off[c + 1] - off[c];
    ctc_dispatch<true, VAR>(lp, T, tg + off[c], L, lane, sa);
    float l = ctc_readout(sa, L);
    if (lane == 0) loss[c] = l;
}

// ------------------------------------------------------------------ 10. decision -------
// mixed/run.py:96-133.  ranked = stable sort by final desc of finite-loss candidates -> the
// winner is the first maximum.
__global__ __launch_bounds__(256) void k_result(QvTables tab, QvWork wk, int batch) {
    __shared__ double sh_s[8];
    __shared__ unsigned long long sh_k[8];
    int b = blockIdx.x, tid = threadIdx.x;
    QvUtt &u = wk.utt[b];
    double best = -INFINITY;
    unsigned long long key = ~0ull;
    if (u.use_ctc) {
        for (int c = tid; c < u.n_cand; c += 256) {
            float l = wk.cand_loss[(size_t)b * QV_CAND_CAP + c];
            if (!isfinite(l)) continue;
            double f = wk.cand_final[(size_t)b * QV_CAND_CAP + c];
            if (key == ~0ull || better(f, (unsigned long long)c, best, key)) { best = f; key = c; }
        }
    }
    // block_best with -inf scores: "better" handles -inf vs -inf via key
    block_best(best, key, sh_s, sh_k);
    if (tid != 0) return;
    qv_result r;
    r.surah = r.ayah = r.ayah_end = 0;
    r.source = QV_SOURCE_NONE;
    r.score = 0.0;
    r.base_score = u.base_start >= 0 ? u.base_score : 0.0;
    r.ctc_norm_loss = 0.f;
    r.n_tokens = u.n_tok;
    r.n_chars = u.q_len;
    // literal mode (skip_unused == 0) builds a candidate list for gate-pass utterances too; nothing scores it, so the
    // result reports what include/qverse.h promises: no candidates and no clipped list when the rerank did not run
    r.n_candidates = u.use_ctc ? u.n_cand : 0;
    r.flags = u.use_ctc ? u.flags : (u.flags & ~QV_FLAG_CAND_OVERFLOW);
    r.t_frames = u.t_frames;
    if (u.q_len > 0) {
        if (u.use_ctc && key != ~0ull) {
            int c = (int)key;
            int st = wk.cand_start[(size_t)b * QV_CAND_CAP + c], sp = wk.cand_span[(size_t)b * QV_CAND_CAP + c];
            size_t tk = (size_t)st * QV_MAX_SPAN + (sp - 1);
            int L = (int)(tab.tok_off[tk + 1] - tab.tok_off[tk]);
            float norm = __fdiv_rn(wk.cand_loss[(size_t)b * QV_CAND_CAP + c], (float)L);
            r.source = QV_SOURCE_CTC;
            r.ctc_norm_loss = norm;
            r.score = exp(-(double)norm);  // host recomputes with libm for the authoritative value
            r.surah = tab.surah[st]; r.ayah = tab.ayah[st]; r.ayah_end = r.ayah + sp - 1;
            u.win = c; u.win_norm = norm;
        } else if (u.base_start >= 0) {
            r.source = QV_SOURCE_TEXT;
            r.score = u.base_score;
            r.surah = tab.surah[u.base_start]; r.ayah = tab.ayah[u.base_start];
            r.ayah_end = r.ayah + u.base_span - 1;
        }
    }
    wk.results[b] = r;
    wk.packed[b * 4 + 0] = r.surah;
    wk.packed[b * 4 + 1] = r.ayah;
    wk.packed[b * 4 + 2] = r.ayah_end;
    wk.packed[b * 4 + 3] = __float_as_int((float)r.score);
}

__global__ void k_init_utts(QvWork wk, const int32_t *__restrict__ t_dev, int batch) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) { *wk.n_fail = 0; wk.frag_ctr[0] = 0; wk.frag_ctr[1] = 0; wk.frag_ctr[2] = 0; }
    if (b < batch) wk.utt[b].t_frames = t_dev[b];
}

__global__ void k_track_final(QvTables tab, QvTrack tw, int batch, int nblk) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double best = 0.0;
    unsigned long long key = ~0ull;
    for (int i = 0; i < nblk; ++i) {
        double s = tw.part_s[(size_t)b * QV_TRACK_BLOCKS + i];
        unsigned long long k = tw.part_k[(size_t)b * QV_TRACK_BLOCKS + i];
        if (better(s, k, best, key)) { best = s; key = k; }
    }
    qv_track_match r;
    r.verse = -1; r.surah = 0; r.ayah = 0; r.variant = 0; r.n_words = 0; r.reserved = 0; r.score = 0.0;
    if (best > 0.0 && key != ~0ull) {          // "score > best_score" starts from 0.0 (verse_tracker.py:78,90)
        int v = (int)(key >> 1), nb = (int)(key & 1ull);
        r.verse = v; r.surah = tab.surah[v]; r.ayah = tab.ayah[v];
        r.variant = nb ? 2 : 0; r.n_words = tab.nw[nb ? 2 : 0][v]; r.score = best;
    }
    tw.out[b] = r;
}

}  // namespace

// ====================================================================== host side =======

// dynamic LDS of k_pass1_final and k_topk: n_verses scores + the selection's scratch
static size_t select_lds(const QvTables &tab) { return (size_t)tab.n_verses * 8 + 128 * 8 + 128 * 4 + 272 * 4 + 128 * 4 + 128 * 8 + 64; }

// match_verse up to the gate (quran_db.py:244-371) for the `batch` utterances whose codes and match masks are in the
// workspace: pass 1 over each utterance's iteration list, the span pass, base + gate.  lcs_y: k_lcs_full's grid y over that
// list -- 32 for the trigram candidates of the hot path, 74 (one round of 74 x 256 lanes over 3 texts per verse) when every
// verse is scanned; hint: the suffix-prefix scores of utterance 0's continuation hint (k_set_hint) enter pass 1.
static void launch_match(const QvMatchSet &set, const QvTables &tab, const QvWork &wk, const QvKnobs &kn, int batch, int lcs_y,
                         bool hint, int force_ctc, hipStream_t stream, const QvSwitches &sw) {
    hipLaunchKernelGGL(set.k_trigram, dim3(batch), dim3(256), (size_t)tab.n_verses * 8 + set.trigram_lds, stream, tab, wk);
    hipLaunchKernelGGL(set.k_lcs_full, dim3(batch, lcs_y), dim3(256), 0, stream, tab, wk, 0);
    hipLaunchKernelGGL(set.k_frag, dim3(set.frag_blocks), dim3(256), 0, stream, tab, wk);
    if (hint) hipLaunchKernelGGL(set.k_hint_sp, dim3(1), dim3(64), 0, stream, tab, wk, 0);
    hipLaunchKernelGGL(k_pass1_final, dim3(batch), dim3(256), select_lds(tab), stream, tab, wk, kn);
    auto k_span_pass = sw[QV_KV_SPANS] == 1 ? set.k_spans2 : set.k_spans;
    hipLaunchKernelGGL(k_span_pass, dim3(QV_SPAN_BLOCKS, batch), dim3(256), 0, stream, tab, wk, kn);
    hipLaunchKernelGGL(k_base_final, dim3((batch + 63) / 64), dim3(64), 0, stream, tab, wk, kn, batch, force_ctc);
}

static void launch_retrieval(qv_engine *eng, QvCtx &c, int batch, int force_ctc, hipStream_t stream, const QvSwitches &sw) {
    const QvMatchSet &set = *eng->match;
    const QvTables &tab = eng->tab;
    const QvWork &wk = c.work;
    const QvKnobs &kn = eng->knobs;
    launch_match(set, tab, wk, kn, batch, 32, false, force_ctc, stream, sw);
    // gate-failed utterances only (device-side list; blocks past n_fail exit at once)
    hipLaunchKernelGGL(set.k_lcs_full, dim3(batch, 74), dim3(256), 0, stream, tab, wk, 1);   // 3 jobs per verse: one round of 74 x 256 lanes
    hipLaunchKernelGGL(set.k_frag, dim3(set.frag_blocks), dim3(256), 0, stream, tab, wk);
    hipLaunchKernelGGL(k_topk, dim3(batch, 2), dim3(256), select_lds(tab), stream, tab, wk, kn);
    hipLaunchKernelGGL(k_candidates, dim3(batch), dim3(256), (size_t)CAND_PCAP * 12 + CAND_HT * 8 + 1200, stream, tab, wk, kn);
}

// the rerank: the long-target instantiation (up to 768 states per candidate: 12 state registers per lane, 3 KB of LDS per
// wave; the set's own where it has one) or the common one, each with the wave program QVERSE_CTC picks (0: ctc_wave, cross-check only)
static void launch_ctc(const QvMatchSet &set, bool long_targets, int variant, const QvTables &tab, const QvWork &wk, const QvKnobs &kn,
                       const float *lp, int t_max, int batch, hipStream_t stream) {
    const int v = variant != 0;
    auto k = v ? k_ctc<false, 1> : k_ctc<false, 0>;
    if (long_targets) k = set.k_ctc_long[v] ? set.k_ctc_long[v] : (v ? k_ctc<true, 1> : k_ctc<true, 0>);
    hipLaunchKernelGGL(k, dim3(batch, 64), dim3(256), 0, stream, tab, wk, kn, lp, t_max);
}

int qv_post_run(qv_engine *eng, QvCtx &c, const float *lp, int t_max, const int32_t *t_host, int batch, hipStream_t stream) {
    const QvSwitches sw = qv_switches_now();   // read once per run: the graph key and the launches below see these values
    const QvMatchSet &set = *eng->match;
    QvTables &tab = eng->tab;
    QvWork &wk = c.work;
    if (batch > wk.max_batch || t_max > wk.t_cap) {
        qv_set_error(eng, "batch or frame count exceeds engine capacity");
        return QV_ERR_CAPACITY;
    }
    for (int b = 0; b < batch; ++b)
        if (t_host[b] < 0 || t_host[b] > t_max) { qv_set_error(eng, "t_host[b] out of range"); return QV_ERR_ARG; }
    {
        // pinned staging slot: wait for the copy that last read it (two calls ago), never for the stream
        const int slot = c.t_slot;
        c.t_slot = (slot + 1) % QV_STAGE_SLOTS;
        if (c.t_pending[slot]) { QV_HIP(hipEventSynchronize(c.t_copied[slot])); c.t_pending[slot] = false; }
        int32_t *th = c.t_host_scratch + (size_t)slot * wk.max_batch;
        for (int b = 0; b < batch; ++b) th[b] = t_host[b];
        QV_HIP(hipMemcpyAsync(c.t_dev, th, sizeof(int32_t) * batch, hipMemcpyHostToDevice, stream));
        QV_HIP(hipEventRecord(c.t_copied[slot], stream));
        c.t_pending[slot] = true;
    }
#ifdef QV_DEV_HOOKS
    const int skip = sw[QV_SW_SKIP];   // dev-only, see qv_model.hip
#else
    constexpr int skip = 0;
#endif
    auto launch_chain = [&]() -> int {
        if (skip & 128) return QV_OK;   // (timing experiments only: no post-logits chain at all)
        hipLaunchKernelGGL(set.k_decode, dim3(batch), dim3(set.decode_threads), 0, stream, tab, wk, lp, t_max, c.t_dev);
        qv_stage_mark(eng, c, 2, stream);
        launch_retrieval(eng, c, batch, 0, stream, sw);
        qv_stage_mark(eng, c, 3, stream);
        // the long-target variant only when THIS batch has a clip of more than 384 frames -- not whenever the engine COULD
        // hold one: an engine created for 30 s clips used to run every 10 s batch through it (round 4: tools/sweep.py's 10 s
        // row, 4.8 ms, against bench.py's 3.8 ms for the same batch on an engine sized for it).  2L + 1 <= T <= t_max <= 384
        // holds for every candidate then.
        if (!(skip & 16)) launch_ctc(set, t_max > 384, sw[QV_KV_CTC], tab, wk, eng->knobs, lp, t_max, batch, stream);
        hipLaunchKernelGGL(k_result, dim3(batch), dim3(256), 0, stream, tab, wk, batch);
        qv_stage_mark(eng, c, 4, stream);
        return QV_OK;
    };
    // One graph launch for the whole chain when its arguments are the ones a graph was captured with: the
    // engine's own log-prob workspace (qv_predict_batch*), same batch and frame count -- the steady state of a
    // serving loop.  Everything the 13 kernels decide per utterance (gate, candidate counts, leaders) is read
    // from device memory, so a replay is the same work as the launches it was captured from.  Caller-owned
    // log-prob tensors (pointer changes per call), profiled runs and single-context engines (the chain then runs
    // on the CALLER's stream, which may be the legacy default stream -- not capturable) take the plain launches.
    // Opt-in (QVERSE_POST_GRAPH=1): measured on one MI355X with three batches in flight it changes nothing
    // (4.26 vs 4.13 ms per step, within box noise) -- kernel boundaries cost the same inside a graph, and the
    // host's ~3.5 us per launch is not what limits the step.
    QvCtx::PostGraph *hit = nullptr;
    if (sw[QV_SW_POST_GRAPH] != 0 && !c.post_graph_off && eng->n_ctx > 1 && stream == c.stream && lp == c.logprobs_ws && !eng->profile_stages) {
        // (the kernel variants that pick launches inside the chain are part of the key: a graph captured under another span pass
        // or CTC wave program must not be replayed after qv_debug_kernel_variant changed it)
        const int variants = sw[QV_KV_SPANS] | (sw[QV_KV_CTC] << 4) | ((set.max_q > QV_MAX_TRANSCRIPT) << 8);
        for (int i = 0; i < c.n_post_graph; ++i)
            if (c.post_graph[i].lp == lp && c.post_graph[i].batch == batch && c.post_graph[i].t_max == t_max && c.post_graph[i].variants == variants)
                hit = &c.post_graph[i];
        if (!hit && c.n_post_graph < 4) {
            hipGraphExec_t exec = nullptr;
            bool captured = false;
            // as for the forward graph: a failure of the capture machinery is not a failure of the batch
            int rc = qv_capture_graph(stream, launch_chain, &exec, &captured);
            if (rc) return rc;
            if (captured) {
                c.post_graph[c.n_post_graph] = {lp, batch, t_max, variants, exec};
                hit = &c.post_graph[c.n_post_graph++];
            } else c.post_graph_off = true;
        }
    }
    if (hit) QV_HIP(hipGraphLaunch(hit->exec, stream));
    else {
        int rc = launch_chain();
        if (rc) return rc;
    }
    QV_HIP(hipGetLastError());
    c.last_batch = batch;
    c.last_tmax = t_max;
    return QV_OK;
}

// utterance 0 of the workspace from transcript codes the host already has, in place of k_decode
static int upload_codes(qv_engine *eng, QvCtx &c, const uint8_t *codes_host, int n, hipStream_t stream) {
    static const int32_t zero = 0;
    QV_HIP(hipMemcpyAsync(c.t_dev, &zero, sizeof(int32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_init_utts, dim3(1), dim3(64), 0, stream, c.work, c.t_dev, 1);
    if (n > 0) QV_HIP(hipMemcpyAsync(c.work.q, codes_host, n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(eng->match->k_prepare_codes, dim3(1), dim3(64), 0, stream, c.work, n);
    return QV_OK;
}

int qv_post_debug_retrieve(qv_engine *eng, QvCtx &c, const uint8_t *codes_host, int n, hipStream_t stream) {
    const QvSwitches sw = qv_switches_now();
    if (n > eng->match->max_q) { qv_set_error(eng, "transcript longer than the engine's max_transcript"); return QV_ERR_CAPACITY; }
    int rc = upload_codes(eng, c, codes_host, n, stream);
    if (rc) return rc;
    launch_retrieval(eng, c, 1, 1, stream, sw);
    QV_HIP(hipGetLastError());
    QV_HIP(hipStreamSynchronize(stream));
    return QV_OK;
}

int qv_post_debug_ctc(qv_engine *eng, const float *lp, int T, const uint16_t *tg, const int32_t *lens, int n,
                      float *loss_host, hipStream_t stream) {
    const QvSwitches sw = qv_switches_now();
    std::vector<int32_t> off(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (lens[i] <= 0 || 2 * lens[i] + 1 > 768) { qv_set_error(eng, "target length unsupported"); return QV_ERR_ARG; }
        off[i + 1] = off[i] + lens[i];
    }
    uint16_t *d_t = nullptr;
    int32_t *d_o = nullptr;
    float *d_l = nullptr;
    QV_HIP(hipMalloc(&d_t, sizeof(uint16_t) * std::max(1, off[n])));
    QV_HIP(hipMalloc(&d_o, sizeof(int32_t) * (n + 1)));
    QV_HIP(hipMalloc(&d_l, sizeof(float) * std::max(1, n)));
    QV_HIP(hipMemcpyAsync(d_t, tg, sizeof(uint16_t) * off[n], hipMemcpyHostToDevice, stream));
    QV_HIP(hipMemcpyAsync(d_o, off.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, stream));
    if (sw[QV_KV_CTC] == 0) hipLaunchKernelGGL(k_ctc_debug<0>, dim3(n), dim3(64), 0, stream, lp, T, d_t, d_o, n, d_l);
    else hipLaunchKernelGGL(k_ctc_debug<1>, dim3(n), dim3(64), 0, stream, lp, T, d_t, d_o, n, d_l);
    QV_HIP(hipMemcpyAsync(loss_host, d_l, sizeof(float) * n, hipMemcpyDeviceToHost, stream));
    QV_HIP(hipStreamSynchronize(stream));
    (void)hipFree(d_t); (void)hipFree(d_o); (void)hipFree(d_l);
    return QV_OK;
}

int qv_post_tracker_match(qv_engine *eng, const uint8_t *codes_host, const int32_t *offsets_host,
                          const int32_t *n_words_host, const int32_t *bonus_host, int batch,
                          qv_track_match *out_host, hipStream_t stream) {
    QvTrack &tw = eng->track;
    const int nblk = (eng->tab.n_verses + 255) / 256;
    if (nblk > QV_TRACK_BLOCKS) { qv_set_error(eng, "verse table larger than the tracker workspace"); return QV_ERR_CAPACITY; }
    std::vector<int32_t> meta((size_t)QV_TRACK_CAP * 4);
    for (int b0 = 0; b0 < batch; b0 += QV_TRACK_CAP) {
        int nb = std::min(QV_TRACK_CAP, batch - b0);
        const int32_t base = offsets_host[b0];
        for (int i = 0; i < nb; ++i) {
            meta[i * 4] = offsets_host[b0 + i + 1] - offsets_host[b0 + i];
            meta[i * 4 + 1] = n_words_host[b0 + i];
            meta[i * 4 + 2] = bonus_host[b0 + i];
            meta[i * 4 + 3] = offsets_host[b0 + i] - base;
        }
        const int32_t total = offsets_host[b0 + nb] - base;   // <= nb * max_q (lengths were checked)
        if (total > 0) QV_HIP(hipMemcpyAsync(tw.q, codes_host + base, (size_t)total, hipMemcpyHostToDevice, stream));
        QV_HIP(hipMemcpyAsync(tw.meta, meta.data(), sizeof(int32_t) * 4 * nb, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(eng->match->k_track, dim3(nb, nblk), dim3(256), 0, stream, eng->tab, tw);
        hipLaunchKernelGGL(k_track_final, dim3((nb + 63) / 64), dim3(64), 0, stream, eng->tab, tw, nb, nblk);
        QV_HIP(hipGetLastError());
        QV_HIP(hipMemcpyAsync(out_host + b0, tw.out, sizeof(qv_track_match) * nb, hipMemcpyDeviceToHost, stream));
        QV_HIP(hipStreamSynchronize(stream));   // meta[] and the workspace are reused by the next slice
    }
    return QV_OK;
}

// match_verse(text, max_span, hint, use_trigram_index=False) (quran_db.py:244-371): full scan,
// continuation bonuses, span pass; result in utt[0].base_* (SYNCHRONOUS).
int qv_post_match_verse(qv_engine *eng, QvCtx &c, const uint8_t *codes_host, int n, int n_bonus, const int32_t *bonus_verse,
                        const double *bonus_value, int max_span, hipStream_t stream) {
    const QvSwitches sw = qv_switches_now();
    QvKnobs kn = eng->knobs;
    kn.max_span = max_span;
    int rc = upload_codes(eng, c, codes_host, n, stream);
    if (rc) return rc;
    int hv[3] = {-1, -1, -1};
    double hb[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < n_bonus; ++i) { hv[i] = bonus_verse[i]; hb[i] = bonus_value[i]; }
    hipLaunchKernelGGL(k_set_hint, dim3(1), dim3(1), 0, stream, c.work, 0, n_bonus, hv[0], hv[1], hv[2], hb[0], hb[1], hb[2]);
    launch_match(*eng->match, eng->tab, c.work, kn, 1, 74, n_bonus > 0, 0, stream, sw);
    QV_HIP(hipGetLastError());
    QV_HIP(hipStreamSynchronize(stream));
    return QV_OK;
}
