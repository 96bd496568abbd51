"""Restatement of the correction rule (include/qverse.h, "recitation correction") for the tests: Levenshtein alignment with
the tie order S, D, I, op codes, word folding, prefix mode.  Written from the rule, host only, integers only.

Texts are sequences of alphabet codes WITH their spaces (code 0).  `correct` fills the DP row by row with numpy (the
insertion chain of a row is a running minimum: dp[i][j] = j + min over k <= j of (t[k] - k), t = the better of sub and del);
`correct_plain` is the same rule in plain loops, cell by cell, and the host test holds the two to each other.
"""

from __future__ import annotations

import numpy as np

MAX_REF, MAX_WORDS, MAX_RAW = 1280, 288, 2048
PREFIX = 1
NO_TARGET, NO_TRANSCRIPT, TOO_LONG, LAST_WORD_OPEN = 1, 2, 4, 8
MATCH, SUB, DEL, INS = 0, 1, 2, 3
INFO_FIELDS = ("n_ref", "n_pred", "n_words", "n_ref_used", "words_touched", "distance", "n_match", "n_sub", "n_del", "n_ins",
               "n_ops", "flags", "start_verse", "span")
WORD_FIELDS = ("n_symbols", "n_match", "n_sub", "n_del", "n_ins", "type")


def strip(codes):
    """(symbols, word(r) per symbol, n_words)"""
    sym, word, spaces = [], [], 0
    for c in codes:
        c = int(c)
        if c == 0:
            spaces += 1
        else:
            sym.append(c)
            word.append(spaces)
    return sym, word, spaces + 1


def moves_numpy(ref, pred):
    """(last column dp[i][m] for i in 0..n, move matrix [n+1][m+1]: 0 S, 1 D, 2 I; row 0 and column 0 unused)"""
    n, m = len(ref), len(pred)
    r, p = np.asarray(ref, np.int64), np.asarray(pred, np.int64)
    ar = np.arange(m + 1, dtype=np.int64)
    prev = ar.copy()
    mv = np.zeros((n + 1, m + 1), np.uint8)
    last = np.zeros(n + 1, np.int64)
    last[0] = m
    for i in range(1, n + 1):
        sub = prev[:-1] + (p != r[i - 1])
        dele = prev[1:] + 1
        t = np.concatenate(([i], np.minimum(sub, dele)))
        cur = np.minimum.accumulate(t - ar) + ar
        mv[i, 1:] = np.where(cur[1:] == sub, 0, np.where(cur[1:] == dele, 1, 2))
        prev = cur
        last[i] = cur[m]
    return last, mv


def moves_plain(ref, pred):
    n, m = len(ref), len(pred)
    dp = [[0] * (m + 1) for _ in range(n + 1)]
    mv = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        dp[i][0] = i
    for j in range(m + 1):
        dp[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            sub = dp[i - 1][j - 1] + (ref[i - 1] != pred[j - 1])
            dele = dp[i - 1][j] + 1
            ins = dp[i][j - 1] + 1
            dp[i][j] = min(sub, dele, ins)
            mv[i][j] = 0 if dp[i][j] == sub else (1 if dp[i][j] == dele else 2)
    return [dp[i][m] for i in range(n + 1)], mv


def _flagged(flags):
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["flags"] = flags
    return {"info": info, "ops": [], "words": [], "positions": []}


def correct(pred_codes, ref_codes, prefix=False, max_pred=1024, start_verse=-1, span=0, moves=moves_numpy):
    """{"info": {INFO_FIELDS}, "ops": [op per column], "positions": [position per column], "words": [WORD_FIELDS tuples]}"""
    pred, _, _ = strip(pred_codes)
    ref, word, n_words = strip(ref_codes)
    n, m = len(ref), len(pred)
    flags = (NO_TARGET if n == 0 else 0) | (NO_TRANSCRIPT if m == 0 else 0)
    if n > MAX_REF or m > max_pred or n_words > MAX_WORDS:
        flags |= TOO_LONG
    if flags:
        return _flagged(flags)
    last, mv = moves(ref, pred)
    i_end = n
    if prefix:
        i_end = min(range(n + 1), key=lambda i: (int(last[i]), i))
    cols = []                                  # (op, position), last column first
    i, j = i_end, m
    while i > 0 or j > 0:
        move = 2 if i == 0 else (1 if j == 0 else int(mv[i][j]))
        if move == 0:
            cols.append((MATCH if ref[i - 1] == pred[j - 1] else SUB, i - 1))
            i, j = i - 1, j - 1
        elif move == 1:
            cols.append((DEL, i - 1))
            i -= 1
        else:
            cols.append((INS, i))
            j -= 1
    cols.reverse()
    words = [[0, 0, 0, 0, 0, 0] for _ in range(n_words)]
    for op, pos in cols:
        w = words[word[pos] if pos < n else word[n - 1]]
        w[1 + op] += 1
        if op != MATCH:
            if op == SUB:
                w[5] = SUB
            elif w[5] == 0:
                w[5] = op
    for w in words:
        w[0] = w[1] + w[2] + w[3]
    count = [sum(1 for op, _ in cols if op == k) for k in range(4)]
    flags = LAST_WORD_OPEN if 1 <= i_end < n and word[i_end - 1] == word[i_end] else 0
    info = {"n_ref": n, "n_pred": m, "n_words": n_words, "n_ref_used": i_end, "words_touched": len(set(word[:i_end])),
            "distance": int(last[i_end]), "n_match": count[0], "n_sub": count[1], "n_del": count[2], "n_ins": count[3],
            "n_ops": len(cols), "flags": flags, "start_verse": start_verse, "span": span}
    assert info["distance"] == count[1] + count[2] + count[3]
    return {"info": info, "ops": [op for op, _ in cols], "positions": [pos for _, pos in cols], "words": [tuple(w) for w in words]}


def correct_plain(pred_codes, ref_codes, prefix=False, **kw):
    return correct(pred_codes, ref_codes, prefix, moves=moves_plain, **kw)


def reference_shape(r, ref_syms, pred_syms):
    """(alignment pairs, errors) in align_phonemes' shape from a non-prefix result, symbols as the caller's tokens"""
    align, errors = [], []
    i = j = 0
    names = {SUB: "substitution", DEL: "deletion", INS: "insertion"}
    for op, pos in zip(r["ops"], r["positions"]):
        a = ref_syms[i] if op != INS else None
        b = pred_syms[j] if op != DEL else None
        align.append([a, b])
        if op != MATCH:
            errors.append({"type": names[op], "position": pos, "expected": a, "got": b})
        i += op != INS
        j += op != DEL
    return align, errors
