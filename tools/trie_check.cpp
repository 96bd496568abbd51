// dev / test: the trie of the verse token sequences (csrc/qv_trie_host.h) -- host only, no GPU.
//
//     c++ -std=c++17 -fsanitize=address,undefined tools/trie_check.cpp -o trie_check
//     ./trie_check offline-tarteel_amd/data/qverse_tables.bin
//
// Builds the trie for S = 1, 2, 3, 6 from the tables file, checks its invariants (every sequence walks from the root to a node
// that lists it; children sorted and consecutive; depth[parent] + 1 == depth; below_count[0] == number of ends; the subtree
// summaries against a recount), prints the statistics and a checksum of every array, and makes sure a bad span and a truncated
// tok section are refused.  Exit status 0 when everything holds, 1 with a message otherwise, 2 for a bad command line, 3 when
// the tables file itself is refused.  tests/test_beam_host.py builds and runs it.
#include "../offline-tarteel_amd/csrc/qv_tables_host.h"
#include "../offline-tarteel_amd/csrc/qv_trie_host.h"

#include <stdio.h>

#include <string>
#include <vector>

namespace {

int broken(int S, const std::string &what) {
    printf("S %d: %s\n", S, what.c_str());
    return 1;
}

int check_trie(const HostTables &h, int S) {
    QvTrie t;
    std::string err;
    if (qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n, h.tok.p, h.tok.n, S, t, err) != QV_TRIE_OK) return broken(S, err);
    const size_t N = t.n_nodes();
    if (t.parent.size() != N || t.depth.size() != N || t.end_off.size() != N + 1 || t.below_count.size() != N || t.below_first.size() != N)
        return broken(S, "array sizes disagree");
    if (t.end_off[0] != 0 || t.end_off[N] != t.ends.size()) return broken(S, "end_off does not span the ends");
    // children: consecutive in node order, sorted by token, each pointing back
    uint32_t next = 1;
    for (size_t n = 0; n < N; ++n) {
        const QvTrieRec &r = t.rec[n];
        if (r.first_child != next || (size_t)r.first_child + r.n_child > N) return broken(S, "children of node " + std::to_string(n) + " are not consecutive");
        for (uint32_t c = r.first_child; c < r.first_child + r.n_child; ++c) {
            if (t.parent[c] != n || t.depth[c] != t.depth[n] + 1) return broken(S, "node " + std::to_string(c) + ": parent / depth");
            if (c > r.first_child && t.rec[c].tok <= t.rec[c - 1].tok) return broken(S, "children of node " + std::to_string(n) + " are not sorted");
            if (t.rec[c].tok >= QV_TRIE_TOKENS) return broken(S, "token out of range");
        }
        next += r.n_child;
        if (t.end_off[n] > t.end_off[n + 1]) return broken(S, "end_off decreases");
        for (uint32_t e = t.end_off[n] + 1; e < t.end_off[n + 1]; ++e)
            if (!qv_trie_end_less(t.ends[e - 1], t.ends[e])) return broken(S, "ends of node " + std::to_string(n) + " are not ascending");
        if (r.n_child == 0 && t.end_off[n] == t.end_off[n + 1]) return broken(S, "leaf " + std::to_string(n) + " ends nothing");
    }
    if (next != N || t.depth[0] != 0 || t.parent[0] != 0) return broken(S, "numbering does not cover the nodes");
    // every sequence walks from the root to a node that lists it; every end is such a sequence
    size_t n_seq = 0;
    std::vector<uint16_t> walk;
    for (int v = 0; v < h.n_verses; ++v)
        for (int sp = 1; sp <= S; ++sp) {
            const size_t k = (size_t)v * QV_TRIE_MAX_SPAN + sp - 1;
            const uint32_t a = h.tok_off[k], b = h.tok_off[k + 1];
            if (a == b) continue;
            ++n_seq;
            uint32_t n = 0;
            for (uint32_t i = a; i < b; ++i) {
                n = qv_trie_child(t, n, h.tok[i]);
                if (!n) return broken(S, "sequence of verse " + std::to_string(v) + " span " + std::to_string(sp) + " leaves the trie");
            }
            bool listed = false;
            for (uint32_t e = t.end_off[n]; e < t.end_off[n + 1]; ++e) listed = listed || (t.ends[e].verse == v && t.ends[e].span == sp && t.ends[e].pad == 0);
            if (!listed) return broken(S, "verse " + std::to_string(v) + " span " + std::to_string(sp) + " is not listed on its node");
            if (!qv_trie_node_tokens(t, n, walk) || walk.size() != b - a || !std::equal(walk.begin(), walk.end(), h.tok.p + a))
                return broken(S, "the walk of the parents does not give the sequence back");
        }
    if (n_seq != t.ends.size() || t.below_count[0] != t.ends.size()) return broken(S, "below_count[0] is not the number of ends");
    // the subtree summaries against a recount from the children
    int max_ends = 0;
    for (size_t n = N; n-- > 0;) {
        uint32_t cnt = t.end_off[n + 1] - t.end_off[n];
        max_ends = std::max(max_ends, (int)cnt);
        QvTrieEnd first = cnt ? t.ends[t.end_off[n]] : QvTrieEnd{0xFFFF, 0xFF, 0};
        for (uint32_t c = t.rec[n].first_child; c < t.rec[n].first_child + t.rec[n].n_child; ++c) {
            cnt += t.below_count[c];
            if (qv_trie_end_less(t.below_first[c], first)) first = t.below_first[c];
        }
        if (cnt != t.below_count[n] || cnt == 0 || first.verse != t.below_first[n].verse || first.span != t.below_first[n].span)
            return broken(S, "subtree summary of node " + std::to_string(n));
    }
    int deepest = 0;
    for (size_t n = 0; n < N; ++n) deepest = std::max(deepest, (int)t.depth[n]);
    if (deepest != t.max_depth) return broken(S, "max_depth");
    printf("stats S %d nodes %zu ends %zu max_depth %d root_children %d max_children %d inner_children %d max_ends %d\n", S, N, t.ends.size(),
           t.max_depth, (int)t.rec[0].n_child, t.max_children, t.max_children_inner, max_ends);
    const QvTrieSums s = qv_trie_checksums(t);
    printf("sums S %d rec %llu parent %llu depth %llu end_off %llu ends %llu below_count %llu below_first %llu\n", S, (unsigned long long)s.rec,
           (unsigned long long)s.parent, (unsigned long long)s.depth, (unsigned long long)s.end_off, (unsigned long long)s.ends,
           (unsigned long long)s.below_count, (unsigned long long)s.below_first);
    return 0;
}

int check_refusals(const HostTables &h) {
    QvTrie t;
    std::string err;
    for (int S : {0, 7, -1})
        if (qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n, h.tok.p, h.tok.n, S, t, err) != QV_TRIE_BAD_ARG) return broken(S, "a span outside 1..6 was accepted");
    // a tok section that ends before the last offset: refused before any id is read
    if (qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n, h.tok.p, h.tok.n - 1, 3, t, err) != QV_TRIE_BAD_TABLE) return broken(3, "a truncated tok section was accepted");
    if (qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n, h.tok.p, h.tok.n / 2, 1, t, err) != QV_TRIE_BAD_TABLE) return broken(1, "a truncated tok section was accepted");
    if (qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n - 1, h.tok.p, h.tok.n, 1, t, err) != QV_TRIE_BAD_TABLE) return broken(1, "a truncated tok_off section was accepted");
    {   // offsets that decrease, and an id that is no token
        std::vector<uint32_t> off(h.tok_off.p, h.tok_off.p + h.tok_off.n);
        off[5] = off[6] + 1;
        if (qv_trie_build(h.n_verses, off.data(), off.size(), h.tok.p, h.tok.n, 1, t, err) != QV_TRIE_BAD_TABLE) return broken(1, "decreasing offsets were accepted");
        std::vector<uint16_t> ids(h.tok.p, h.tok.p + h.tok.n);
        ids[ids.size() / 2] = QV_TRIE_TOKENS;
        if (qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n, ids.data(), ids.size(), 1, t, err) != QV_TRIE_BAD_TABLE) return broken(1, "the blank was accepted as a token");
    }
    printf("refusals hold\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: trie_check <qverse_tables.bin>\n");
        return 2;
    }
    HostTables h;
    std::string err;
    if (qv_read_host_tables(argv[1], h, err) != QV_OK) { printf("refused: %s\n", err.c_str()); return 3; }
    for (int S : {1, 2, 3, 6})
        if (int rc = check_trie(h, S)) return rc;
    if (int rc = check_refusals(h)) return rc;
    printf("trie holds\n");
    return 0;
}
