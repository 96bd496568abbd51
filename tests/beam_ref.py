"""Restatement of the verse-constrained CTC prefix beam search (include/qverse.h, "verse-constrained beam search";
csrc/qv_trie_host.h, csrc/qv_beam.hip) in numpy and plain float64 Python -- what the host and GPU tests compare with.

The trie.  Sequences (for the Quran: for every verse v ascending and span sp = 1..S the table's tokens of key v * 6 + sp - 1,
empty ones skipped) are inserted into a trie whose nodes are numbered breadth-first from root = 0 with the children of a node
in ascending token id.  Built here without walking: the sequences are sorted lexicographically, row i then opens the nodes of
depths lcp(i - 1, i) + 1 .. len(i), and breadth-first order within a depth is row order.

The search.  A state is at most W hypotheses (node, pb, pnb); lae(a, b) = b if a == -inf, a if b == -inf, else
max + log1p(exp(min - max)); per frame every hypothesis stays (pb' = tot + lp[blank], s = pnb + lp[tok(node)], s = -inf for the
root) and extends into every child c with token k: x(c) = ((node != 0 and k == tok(node)) ? pb : tot) + lp[k]; a candidate
node gets pb' from its own stay (else -inf) and pnb' = lae(s, x); candidates whose total is -inf are dropped, the W largest
totals are kept, ties to the smaller node index; the result is ordered by total descending, ties to the smaller node."""
from __future__ import annotations

import math

import numpy as np

NEG = -math.inf
U64 = np.uint64


def lae(a: float, b: float) -> float:
    if a == NEG:
        return b
    if b == NEG:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


class Trie:
    """arrays as csrc/qv_trie_host.h names them"""

    def __init__(self, seqs, labels):
        """seqs: non-empty token sequences; labels[i] = (verse, span) of sequence i"""
        assert len(seqs) == len(labels) and all(len(s) > 0 for s in seqs)
        n = len(seqs)
        lens = np.array([len(s) for s in seqs], np.int64)
        L = int(lens.max())
        m = np.full((n, L), -1, np.int32)
        for i, s in enumerate(seqs):
            m[i, : len(s)] = np.asarray(s, np.int32)
        lab = np.asarray(labels, np.int64).reshape(n, 2)
        # lexicographic by tokens (a prefix first; big-endian bytes compare like the tokens), equal sequences by (verse, span)
        keys = [(np.asarray(s, ">u2").tobytes(), int(v), int(sp)) for s, (v, sp) in zip(seqs, lab.tolist())]
        order = np.asarray(sorted(range(n), key=keys.__getitem__), np.int64)
        m, lens, lab = m[order], lens[order], lab[order]
        # common prefix of row i and row i - 1, within both lengths
        lcp = np.zeros(n, np.int64)
        if n > 1:
            same = (m[1:] == m[:-1]) & (m[1:] >= 0)
            lcp[1:] = np.where(same.all(axis=1), L, np.argmin(same, axis=1))
        # node (row i, depth k) for k in lcp[i] + 1 .. lens[i]; breadth-first = by depth, then by row
        cnt = lens - lcp                                       # >= 0; 0 for a repeated sequence
        rows = np.repeat(np.arange(n), cnt)
        first = np.repeat(lcp + 1, cnt)
        depth = first + (np.arange(len(rows)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        by = np.lexsort([rows, depth])
        rows, depth = rows[by], depth[by]
        N = 1 + len(rows)
        ident = np.full((n, L + 1), -1, np.int32)              # ident[i, k]: the node of row i at depth k
        ident[:, 0] = 0
        ident[rows, depth] = np.arange(1, N)
        ident = np.maximum.accumulate(ident, axis=0)           # a row shares the node the last opener above it made
        self.n = N
        self.depth = np.zeros(N, np.uint16)
        self.depth[1:] = depth
        self.tok = np.zeros(N, np.uint16)
        self.tok[1:] = m[rows, depth - 1]
        self.parent = np.zeros(N, np.uint32)
        self.parent[1:] = ident[rows, depth - 1]
        self.n_child = np.bincount(self.parent[1:], minlength=N).astype(np.uint16)
        self.first_child = (1 + np.cumsum(self.n_child.astype(np.int64)) - self.n_child).astype(np.uint32)
        # ends: row i ends on ident[i, lens[i]]; per node ascending by (verse, span) -- the rows' own order
        end_node = ident[np.arange(n), lens]
        eo = np.argsort(end_node, kind="stable")
        self.end_verse = lab[eo, 0].astype(np.uint16)
        self.end_span = lab[eo, 1].astype(np.uint8)
        self.end_off = np.zeros(N + 1, np.uint32)
        self.end_off[1:] = np.cumsum(np.bincount(end_node, minlength=N))
        # subtree summaries, folded level by level from the deepest (a level is a contiguous range of nodes)
        key = np.full(N, 0xFFFF * 256 + 0xFF, np.int64)        # verse * 256 + span, the smallest at or under the node
        own = np.diff(self.end_off.astype(np.int64))
        has = own > 0
        key[has] = self.end_verse[self.end_off[:-1][has]].astype(np.int64) * 256 + self.end_span[self.end_off[:-1][has]]
        below = own.copy()
        level_start = np.searchsorted(self.depth, np.arange(int(self.depth.max()) + 2))
        for d in range(int(self.depth.max()), 0, -1):
            a, b = level_start[d], level_start[d + 1]
            np.add.at(below, self.parent[a:b], below[a:b])
            np.minimum.at(key, self.parent[a:b], key[a:b])
        self.below_count = below.astype(np.uint32)
        self.below_verse = (key // 256).astype(np.uint16)
        self.below_span = (key % 256).astype(np.uint8)
        self.max_depth = int(self.depth.max())
        self.max_children = int(self.n_child.max())
        # plain lists for the search
        self._fc, self._nc, self._tok = self.first_child.tolist(), self.n_child.tolist(), self.tok.tolist()

    @classmethod
    def from_tables(cls, tables, max_span: int) -> "Trie":
        assert 1 <= max_span <= 6
        off, tok = tables.s["tok_off"], tables.s["tok"]
        seqs, labels = [], []
        for v in range(tables.n_verses):
            for sp in range(1, max_span + 1):
                k = v * 6 + sp - 1
                if off[k + 1] > off[k]:
                    seqs.append(tok[off[k]: off[k + 1]])
                    labels.append((v, sp))
        return cls(seqs, labels)

    def n_ends(self) -> int:
        return len(self.end_verse)

    def ends_of(self, node: int):
        a, b = int(self.end_off[node]), int(self.end_off[node + 1])
        return list(zip(self.end_verse[a:b].tolist(), self.end_span[a:b].tolist()))

    def tokens_of(self, node: int) -> list[int]:
        out = []
        while node:
            out.append(self._tok[node])
            node = int(self.parent[node])
        return out[::-1]

    def walk(self, ids) -> int:
        """the node the tokens lead to from the root; -1 when they leave the trie"""
        n = 0
        for k in ids:
            a, c = self._fc[n], self._nc[n]
            j = int(np.searchsorted(self.tok[a: a + c], k))
            if j >= c or self._tok[a + j] != k:
                return -1
            n = a + j
        return n

    def checksums(self) -> dict:
        """qv_trie_checksums: sum of (x[i] + 1) * (2 i + 1) modulo 2^64"""
        def s(x):
            x = np.asarray(x).astype(U64)
            with np.errstate(over="ignore"):
                return int(((x + U64(1)) * (U64(2) * np.arange(len(x), dtype=U64) + U64(1))).sum(dtype=U64))
        sh = lambda a, k: np.asarray(a).astype(U64) << U64(k)  # noqa: E731
        return {"rec": s(sh(self.first_child, 0) | sh(self.n_child, 32) | sh(self.tok, 48)), "parent": s(self.parent), "depth": s(self.depth),
                "end_off": s(self.end_off), "ends": s(sh(self.end_verse, 0) | sh(self.end_span, 16)), "below_count": s(self.below_count),
                "below_first": s(sh(self.below_verse, 0) | sh(self.below_span, 16))}


def beam_search(trie: Trie, lp, W: int, blank: int) -> dict:
    """lp: [T, V] array (float32 or float64: widened exactly).  Returns {"hyps": [(node, total, pb, pnb)] best first,
    "max_candidates" (the largest number of distinct candidate nodes a frame produced, before those with a total of -inf
    are dropped; 0 without frames), "prune_margin" (the smallest gap over all frames between the last kept and the first
    dropped total; inf when nothing was ever dropped), "final_gap" (the smallest gap between adjacent returned totals; inf
    for fewer than two)}"""
    assert 1 <= W
    fc, nc, tk = trie._fc, trie._nc, trie._tok
    rows = np.asarray(lp, np.float64).tolist()
    beam = [(0, 0.0, NEG)]
    max_cand, margin = 0, math.inf
    for row in rows:
        lb = row[blank]
        cand = {}                                              # node -> [pb', s, x]
        for n, pb, pnb in beam:
            tot = lae(pb, pnb)
            c = cand.setdefault(n, [NEG, NEG, NEG])
            c[0] = tot + lb
            c[1] = NEG if n == 0 else pnb + row[tk[n]]
            for ch in range(fc[n], fc[n] + nc[n]):
                k = tk[ch]
                cand.setdefault(ch, [NEG, NEG, NEG])[2] = (pb if (n != 0 and k == tk[n]) else tot) + row[k]
        max_cand = max(max_cand, len(cand))
        scored = []
        for n, (pb, s, x) in cand.items():
            pnb = lae(s, x)
            tot = lae(pb, pnb)
            if tot != NEG:
                scored.append((-tot, n, pb, pnb))
        scored.sort()
        if len(scored) > W:
            margin = min(margin, scored[W][0] - scored[W - 1][0])
        beam = [(n, pb, pnb) for _, n, pb, pnb in scored[:W]]
    hyps = sorted(((-lae(pb, pnb), n, pb, pnb) for n, pb, pnb in beam))
    hyps = [(n, -t, pb, pnb) for t, n, pb, pnb in hyps]
    gaps = [a[1] - b[1] for a, b in zip(hyps, hyps[1:])]
    return {"hyps": hyps, "max_candidates": max_cand, "prune_margin": margin, "final_gap": min(gaps) if gaps else math.inf}


def entry_fields(trie: Trie, tables, node: int) -> dict:
    """the integer fields of qv_beam_entry for `node`"""
    ends = trie.ends_of(node)
    d = {"node": node, "n_tokens": int(trie.depth[node]), "n_ends": len(ends), "start_verse": -1, "span": 0, "surah": 0, "ayah": 0,
         "ayah_end": 0, "below_count": int(trie.below_count[node]), "below_verse": int(trie.below_verse[node]),
         "below_span": int(trie.below_span[node]), "flags": 1 if ends else 0}
    if ends:
        v, sp = ends[0]
        d.update(start_verse=v, span=sp, surah=int(tables.surah[v]), ayah=int(tables.ayah[v]), ayah_end=int(tables.ayah[v]) + sp - 1)
    return d
