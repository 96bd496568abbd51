// qv_trie_host.h -- the trie of the verse token sequences that the constrained beam search walks (include/qverse.h,
// "verse-constrained beam search"; the search itself: qv_beam.hip).  HIP-free (the standard library only), so
// tools/trie_check.cpp runs it under ASan + UBSan on a machine without a GPU; qv_beam.hip uploads `rec`.
//
// Definition.  For a maximum span S in 1..6, for every verse v in ascending order and every span sp = 1..S, the sequence
// of key v * 6 + sp - 1 of the token table (tok_off / tok of qverse_tables.bin: the targets of the CTC rerank) is inserted
// unless it is empty (the table leaves spans that cross a surah's end, and over-long ones, empty); (v, sp) is recorded as an
// END on the sequence's last node.  Nodes are numbered breadth-first from root = 0 with the children of a node in ascending
// token id, so the children of node n are first_child[n] .. first_child[n] + n_child[n] (a leaf's first_child is where its
// children would have been numbered: 1 + the number of children of all nodes before it).  The numbering is part of the
// definition: the search breaks ties by it.
//
// The tables are NOT trusted here either: every offset is checked against what it indexes before it is followed.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#define QV_TRIE_MAX_SPAN 6     // spans of the token table (QV_MAX_SPAN)
#define QV_TRIE_TOKENS 1024    // token ids are 0 .. 1023; 1024 is the blank and never part of a sequence

enum { QV_TRIE_OK = 0, QV_TRIE_BAD_ARG = 1 /* QV_ERR_ARG */, QV_TRIE_BAD_TABLE = 2 /* QV_ERR_IO */ };

struct QvTrieRec { uint32_t first_child; uint16_t n_child; uint16_t tok; };   // tok: the token on the edge INTO the node (root: 0)
struct QvTrieEnd { uint16_t verse; uint8_t span; uint8_t pad; };              // pad = 0
static_assert(sizeof(QvTrieRec) == 8 && sizeof(QvTrieEnd) == 4, "trie layout");

struct QvTrie {
    int max_span = 0;
    std::vector<QvTrieRec> rec;             // [n]  the only array the kernel reads
    std::vector<uint32_t> parent;           // [n]  parent[0] = 0
    std::vector<uint16_t> depth;            // [n]  tokens from the root
    std::vector<uint32_t> end_off;          // [n + 1] into `ends`
    std::vector<QvTrieEnd> ends;            // per node ascending by (verse, span)
    std::vector<uint32_t> below_count;      // [n]  ends at or under the node
    std::vector<QvTrieEnd> below_first;     // [n]  the smallest (verse, span) among them
    int max_depth = 0, max_children = 0;    // max_children: over all nodes, the root included
    int max_children_inner = 0;             // ... over the nodes other than the root
    size_t n_nodes() const { return rec.size(); }
};

inline bool qv_trie_end_less(const QvTrieEnd &a, const QvTrieEnd &b) { return a.verse != b.verse ? a.verse < b.verse : a.span < b.span; }

// tok_off: n_tok_off entries of which the first n_verses * 6 + 1 are used; tok: n_tok entries.
inline int qv_trie_build(int n_verses, const uint32_t *tok_off, size_t n_tok_off, const uint16_t *tok, size_t n_tok, int max_span,
                         QvTrie &out, std::string &err) {
    auto fail = [&](int rc, const std::string &msg) { err = msg; return rc; };
    if (max_span < 1 || max_span > QV_TRIE_MAX_SPAN) return fail(QV_TRIE_BAD_ARG, "trie: max_span " + std::to_string(max_span) + " outside 1..6");
    if (n_verses < 1 || n_verses > 65535 || !tok_off || (!tok && n_tok)) return fail(QV_TRIE_BAD_ARG, "trie: bad table view");
    const size_t NK = (size_t)n_verses * QV_TRIE_MAX_SPAN;
    if (n_tok_off < NK + 1) return fail(QV_TRIE_BAD_TABLE, "trie: tok_off holds " + std::to_string(n_tok_off) + " entries, " + std::to_string(NK + 1) + " needed");
    for (size_t i = 0; i < NK; ++i)
        if (tok_off[i] > tok_off[i + 1]) return fail(QV_TRIE_BAD_TABLE, "trie: tok_off decreases at entry " + std::to_string(i + 1));
    if (tok_off[NK] > n_tok) return fail(QV_TRIE_BAD_TABLE, "trie: tok_off ends at " + std::to_string(tok_off[NK]) + ", the tok section holds " + std::to_string(n_tok) + " ids (truncated?)");
    for (size_t i = 0; i < tok_off[NK]; ++i)
        if (tok[i] >= QV_TRIE_TOKENS) return fail(QV_TRIE_BAD_TABLE, "trie: tok holds id " + std::to_string(tok[i]) + ", not a token");

    struct Seq { uint32_t off, len; uint16_t verse; uint8_t span; };
    std::vector<Seq> seqs;
    for (int v = 0; v < n_verses; ++v)
        for (int sp = 1; sp <= max_span; ++sp) {
            const size_t k = (size_t)v * QV_TRIE_MAX_SPAN + sp - 1;
            const uint32_t len = tok_off[k + 1] - tok_off[k];
            if (len == 0) continue;
            if (len > 65535) return fail(QV_TRIE_BAD_TABLE, "trie: a sequence of " + std::to_string(len) + " tokens");
            seqs.push_back({tok_off[k], len, (uint16_t)v, (uint8_t)sp});
        }
    // lexicographic by tokens (a prefix before what extends it), equal sequences by (verse, span)
    std::sort(seqs.begin(), seqs.end(), [&](const Seq &a, const Seq &b) {
        const uint32_t n = a.len < b.len ? a.len : b.len;
        const uint16_t *pa = tok + a.off, *pb = tok + b.off;
        for (uint32_t i = 0; i < n; ++i)
            if (pa[i] != pb[i]) return pa[i] < pb[i];
        if (a.len != b.len) return a.len < b.len;
        return a.verse != b.verse ? a.verse < b.verse : a.span < b.span;
    });

    QvTrie &t = out;
    t = QvTrie();
    t.max_span = max_span;
    // a node is the run [lo, hi) of sorted sequences that share its prefix; runs are split in node order: breadth-first
    std::vector<uint32_t> lo(1, 0u), hi(1, (uint32_t)seqs.size());
    t.rec.push_back({1u, 0, 0});
    t.parent.push_back(0u);
    t.depth.push_back(0);
    for (size_t n = 0; n < t.rec.size(); ++n) {
        const uint32_t d = t.depth[n];
        uint32_t i = lo[n];
        const uint32_t end = hi[n];
        t.end_off.push_back((uint32_t)t.ends.size());
        for (; i < end && seqs[i].len == d; ++i) t.ends.push_back({seqs[i].verse, seqs[i].span, 0});
        const uint32_t first = (uint32_t)t.rec.size();
        uint32_t n_child = 0;
        while (i < end) {
            const uint16_t k = tok[seqs[i].off + d];
            uint32_t j = i + 1;
            while (j < end && tok[seqs[j].off + d] == k) ++j;
            t.rec.push_back({0u, 0, k});
            t.parent.push_back((uint32_t)n);
            t.depth.push_back((uint16_t)(d + 1));
            lo.push_back(i);
            hi.push_back(j);
            ++n_child;
            i = j;
        }
        t.rec[n].first_child = first;
        t.rec[n].n_child = (uint16_t)n_child;   // <= 1024 distinct tokens
        t.max_children = std::max(t.max_children, (int)n_child);
        if (n) t.max_children_inner = std::max(t.max_children_inner, (int)n_child);
        t.max_depth = std::max(t.max_depth, (int)d);
    }
    t.end_off.push_back((uint32_t)t.ends.size());
    // subtree summaries: children carry larger numbers than their parent, so one reverse pass folds every subtree
    const size_t N = t.rec.size();
    t.below_count.assign(N, 0u);
    t.below_first.assign(N, QvTrieEnd{0xFFFF, 0xFF, 0});
    for (size_t n = 0; n < N; ++n) {
        t.below_count[n] = t.end_off[n + 1] - t.end_off[n];
        if (t.below_count[n]) t.below_first[n] = t.ends[t.end_off[n]];
    }
    for (size_t n = N - 1; n >= 1; --n) {
        const uint32_t p = t.parent[n];
        t.below_count[p] += t.below_count[n];
        if (qv_trie_end_less(t.below_first[n], t.below_first[p])) t.below_first[p] = t.below_first[n];
    }
    return QV_TRIE_OK;
}

// the child of node n along token k, or 0 (the root is nobody's child): binary search over the sorted children
inline uint32_t qv_trie_child(const QvTrie &t, uint32_t n, uint16_t k) {
    uint32_t a = t.rec[n].first_child, b = a + t.rec[n].n_child;
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (t.rec[m].tok < k) a = m + 1; else b = m;
    }
    return a < t.rec[n].first_child + t.rec[n].n_child && t.rec[a].tok == k ? a : 0u;
}

// the tokens from the root to `node` (walk of the parents); false when node is not one
inline bool qv_trie_node_tokens(const QvTrie &t, uint32_t node, std::vector<uint16_t> &out) {
    if (node >= t.rec.size()) return false;
    out.assign(t.depth[node], 0);
    for (uint32_t n = node; n != 0; n = t.parent[n]) out[t.depth[n] - 1] = t.rec[n].tok;
    return true;
}

// Checksums of the arrays, for comparing two builders: sum over i of (x[i] + 1) * (2 i + 1) modulo 2^64, x[i] the element as
// an integer (a record as first_child | n_child << 32 | tok << 48, an end as verse | span << 16).
inline uint64_t qv_trie_sum_step(uint64_t acc, uint64_t x, uint64_t i) { return acc + (x + 1) * (2 * i + 1); }
inline uint64_t qv_trie_rec_key(const QvTrieRec &r) { return (uint64_t)r.first_child | (uint64_t)r.n_child << 32 | (uint64_t)r.tok << 48; }
inline uint64_t qv_trie_end_key(const QvTrieEnd &e) { return (uint64_t)e.verse | (uint64_t)e.span << 16; }
struct QvTrieSums { uint64_t rec, parent, depth, end_off, ends, below_count, below_first; };
inline QvTrieSums qv_trie_checksums(const QvTrie &t) {
    QvTrieSums s = {0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < t.rec.size(); ++i) {
        s.rec = qv_trie_sum_step(s.rec, qv_trie_rec_key(t.rec[i]), i);
        s.parent = qv_trie_sum_step(s.parent, t.parent[i], i);
        s.depth = qv_trie_sum_step(s.depth, t.depth[i], i);
        s.below_count = qv_trie_sum_step(s.below_count, t.below_count[i], i);
        s.below_first = qv_trie_sum_step(s.below_first, qv_trie_end_key(t.below_first[i]), i);
    }
    for (size_t i = 0; i < t.end_off.size(); ++i) s.end_off = qv_trie_sum_step(s.end_off, t.end_off[i], i);
    for (size_t i = 0; i < t.ends.size(); ++i) s.ends = qv_trie_sum_step(s.ends, qv_trie_end_key(t.ends[i]), i);
    return s;
}
