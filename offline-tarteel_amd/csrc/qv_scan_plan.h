// qv_scan_plan.h -- the launch plan of the exhaustive CTC scan (include/qverse.h, "exhaustive CTC scan"; the kernels:
// qv_scan.hip).  HIP-free (the standard library only): qv_scan_stats is its face on a machine without a GPU.
//
// A KEY is (verse v, span sp) with the token sequence v * 6 + sp - 1 of the tables' token table, L tokens long.  It is
// FEASIBLE for a row of T frames when L > 0, 2 L + 1 <= T, sp <= max_span and the surah of v is in the row's mask.
// A CHAIN is a maximal run of spans sp_a .. sp_b of one verse in which every span's ids are a prefix of the next one's
// (pfx bit sp - 1 of the verse, as qv_tables_host.h derives it: both non-empty, lengths non-decreasing).  Along a chain
// L never shrinks, so a chain's feasible keys are its first ones: sp_a .. sp_c.  One RECURSION runs per chain with a feasible
// key, over the tokens of (v, sp_c) -- the leader -- and the losses of sp_a .. sp_c are read out of its last alpha row.
// Recursions are ordered by decreasing leader length (ties: verse ascending), so the longest ones start first.
//
// The table view is NOT trusted: sizes and offsets are checked before anything is derived from them.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#define QV_SCAN_MAX_SPAN 6     // spans of the token table (QV_MAX_SPAN)
#define QV_SCAN_MAX_L 383      // 2 L + 1 <= 767 states: what the wave programs hold (768); plans are made for at most 768 frames
#define QV_SCAN_SURAHS 128     // bits of a surah mask

enum { QV_SCAN_OK = 0, QV_SCAN_BAD_ARG = 1 /* QV_ERR_ARG */, QV_SCAN_BAD_TABLE = 2 /* QV_ERR_IO */ };

struct QvScanRec { uint16_t verse; uint8_t first_span, lead_span; };   // spans first_span .. lead_span are read out
static_assert(sizeof(QvScanRec) == 4, "plan layout");

struct QvScanView {
    int n_verses = 0;
    const uint32_t *tok_off = nullptr; size_t n_tok_off = 0;   // [n_verses * 6 + 1]
    const uint8_t *pfx = nullptr; size_t n_pfx = 0;            // [n_verses] bit k - 1: span k is a prefix of span k + 1
    const uint8_t *surah = nullptr; size_t n_surah = 0;        // [n_verses] 1 .. 128
};

struct QvScanPlan {
    std::vector<QvScanRec> rec;   // the recursions, longest leader first
    int32_t n_feasible = 0;
    int64_t state_steps = 0;      // sum over the recursions of (2 L_leader + 1) * T
};

inline int qv_scan_view_check(const QvScanView &t, std::string &err) {
    auto fail = [&](int rc, const std::string &msg) { err = msg; return rc; };
    if (t.n_verses < 1 || t.n_verses > 65535 || !t.tok_off || !t.pfx || !t.surah) return fail(QV_SCAN_BAD_ARG, "scan: bad table view");
    const size_t N = (size_t)t.n_verses, NK = N * QV_SCAN_MAX_SPAN;
    if (t.n_tok_off < NK + 1) return fail(QV_SCAN_BAD_TABLE, "scan: tok_off holds " + std::to_string(t.n_tok_off) + " entries, " + std::to_string(NK + 1) + " needed");
    if (t.n_pfx < N || t.n_surah < N) return fail(QV_SCAN_BAD_TABLE, "scan: pfx / surah hold fewer entries than there are verses");
    for (size_t i = 0; i < NK; ++i)
        if (t.tok_off[i] > t.tok_off[i + 1]) return fail(QV_SCAN_BAD_TABLE, "scan: tok_off decreases at entry " + std::to_string(i + 1));
    for (size_t v = 0; v < N; ++v)
        if (t.surah[v] < 1 || t.surah[v] > QV_SCAN_SURAHS) return fail(QV_SCAN_BAD_TABLE, "scan: verse " + std::to_string(v) + " has surah " + std::to_string(t.surah[v]));
    return QV_SCAN_OK;
}

inline bool qv_scan_mask_empty(const uint32_t *mask4) { return mask4 && !(mask4[0] | mask4[1] | mask4[2] | mask4[3]); }
inline bool qv_scan_selected(const uint32_t *mask4, int surah) { return !mask4 || ((mask4[(surah - 1) >> 5] >> ((surah - 1) & 31)) & 1u); }

// the chains of the whole table at max_span 6: no plan of any row has more recursions (a plan's recursions are distinct chains)
inline size_t qv_scan_chain_count(const QvScanView &t) {
    size_t n = 0;
    for (int v = 0; v < t.n_verses; ++v)
        for (int sp = 1; sp <= QV_SCAN_MAX_SPAN; ++sp) {
            const size_t k = (size_t)v * QV_SCAN_MAX_SPAN + sp - 1;
            if (t.tok_off[k + 1] == t.tok_off[k]) continue;
            if (sp == 1 || !((t.pfx[v] >> (sp - 2)) & 1)) ++n;
        }
    return n;
}

// `t` has passed qv_scan_view_check.  mask4 == nullptr: every surah.
inline int qv_scan_plan_make(const QvScanView &t, int T, int max_span, const uint32_t *mask4, QvScanPlan &out, std::string &err) {
    auto fail = [&](int rc, const std::string &msg) { err = msg; return rc; };
    if (T < 0 || T > 2 * QV_SCAN_MAX_L + 2 || max_span < 1 || max_span > QV_SCAN_MAX_SPAN)
        return fail(QV_SCAN_BAD_ARG, "scan: t_frames outside 0..768 or max_span outside 1..6");
    if (qv_scan_mask_empty(mask4)) return fail(QV_SCAN_BAD_ARG, "scan: the surah mask selects nothing");
    out = QvScanPlan();
    if (T < 3) return QV_SCAN_OK;   // nothing is feasible
    const int l_gate = (T - 1) / 2;   // <= QV_SCAN_MAX_L
    // counting sort by leader length, longest first; within a length by (verse, span) ascending
    std::vector<uint32_t> count((size_t)l_gate + 2, 0u);
    std::vector<QvScanRec> found;
    std::vector<uint16_t> found_l;
    for (int v = 0; v < t.n_verses; ++v) {
        if (!qv_scan_selected(mask4, t.surah[v])) continue;
        const uint32_t *off = t.tok_off + (size_t)v * QV_SCAN_MAX_SPAN;
        int sp = 1;
        while (sp <= max_span) {
            // the chain that starts at sp (an empty span is a chain of nothing)
            int end = sp;
            while (end < max_span && ((t.pfx[v] >> (end - 1)) & 1)) ++end;
            int lead = 0;
            for (int k = sp; k <= end; ++k) {
                const uint32_t L = off[k] - off[k - 1];
                if (L == 0 || L > (uint32_t)l_gate) break;   // (lengths do not shrink along a chain)
                lead = k;
            }
            if (lead) {
                const uint32_t L = off[lead] - off[lead - 1];
                found.push_back({(uint16_t)v, (uint8_t)sp, (uint8_t)lead});
                found_l.push_back((uint16_t)L);
                ++count[L];
                out.n_feasible += lead - sp + 1;
                out.state_steps += (int64_t)(2 * L + 1) * T;
            }
            sp = end + 1;
        }
    }
    std::vector<uint32_t> at((size_t)l_gate + 2, 0u);
    uint32_t run = 0;
    for (int L = l_gate; L >= 1; --L) { at[L] = run; run += count[L]; }
    out.rec.resize(found.size());
    for (size_t i = 0; i < found.size(); ++i) out.rec[at[found_l[i]]++] = found[i];
    return QV_SCAN_OK;
}
