"""Restatement of the exhaustive CTC scan (include/qverse.h, "exhaustive CTC scan") in numpy and torch: the keys of a row from
Tables, their float64 CTC losses (torch.nn.functional.ctc_loss, batches of 16), the ranking, and the plan statistics
qv_scan_stats reports.  Nothing here calls the library."""
from __future__ import annotations

import numpy as np

MAX_SPAN = 6
BLANK = 1024


def lengths(tables) -> np.ndarray:
    """L of every key v * 6 + sp - 1"""
    return np.diff(tables.s["tok_off"][: tables.n_verses * MAX_SPAN + 1].astype(np.int64))


def selected(tables, surahs) -> np.ndarray:
    """per verse: is its surah in `surahs` (None = all)"""
    if surahs is None:
        return np.ones(tables.n_verses, bool)
    return np.isin(np.asarray(tables.surah[: tables.n_verses]).astype(np.int64), np.asarray(list(surahs), np.int64))


def feasible(tables, T: int, max_span: int = MAX_SPAN, surahs=None) -> np.ndarray:
    """bool per key: L > 0, 2 L + 1 <= T, sp <= max_span, surah selected"""
    L = lengths(tables)
    sp = np.tile(np.arange(1, MAX_SPAN + 1), tables.n_verses)
    return (L > 0) & (2 * L + 1 <= T) & (sp <= max_span) & np.repeat(selected(tables, surahs), MAX_SPAN)


def keys(tables, T: int, max_span: int = MAX_SPAN, surahs=None):
    """(key, v, sp, L) arrays of the feasible keys, key ascending"""
    k = np.flatnonzero(feasible(tables, T, max_span, surahs))
    return k, k // MAX_SPAN, k % MAX_SPAN + 1, lengths(tables)[k]


def chain_ids(tables) -> np.ndarray:
    """per key the number of its chain: a chain is a maximal run of spans of one verse in which every span's ids are a prefix
    of the next one's (both non-empty); an empty key is a chain of its own.  From the token ids themselves."""
    off = tables.s["tok_off"].astype(np.int64)
    tok = tables.s["tok"]
    L = lengths(tables)
    starts = np.ones(tables.n_verses * MAX_SPAN, bool)
    for v in range(tables.n_verses):
        for sp in range(2, MAX_SPAN + 1):
            k = v * MAX_SPAN + sp - 1
            la, lb = L[k - 1], L[k]
            if la > 0 and lb >= la and np.array_equal(tok[off[k - 1]: off[k]], tok[off[k]: off[k] + la]):
                starts[k] = False
    return np.cumsum(starts) - 1


def stats(tables, chains: np.ndarray, T: int, max_span: int = MAX_SPAN, surahs=None) -> dict:
    """what qv_scan_stats counts: feasible keys, chains with a feasible key (one alpha recursion each, over the chain's
    longest feasible key) and the sum over them of (2 L + 1) * T"""
    f = feasible(tables, T, max_span, surahs)
    lead = np.zeros(int(chains.max()) + 1, np.int64)
    np.maximum.at(lead, chains[f], lengths(tables)[f])
    lead = lead[lead > 0]
    return {"n_feasible": int(f.sum()), "n_recursions": int(len(lead)), "state_steps": int(((2 * lead + 1) * T).sum())}


def losses64(lp: np.ndarray, tables, key: np.ndarray) -> np.ndarray:
    """float64 negative log-likelihoods of the keys' targets on the log-probs lp [T, 1025] (any float dtype; widened exactly)"""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float64))
    T = x.shape[0]
    out = np.empty(len(key), np.float64)
    for s in range(0, len(key), 16):
        part = key[s: s + 16]
        tg = [torch.from_numpy(tables.token_ids(int(k) // MAX_SPAN, int(k) % MAX_SPAN + 1).astype(np.int64)) for k in part]
        n = len(part)
        out[s: s + n] = F.ctc_loss(x[:, None, :].expand(T, n, -1), torch.cat(tg), torch.full((n,), T, dtype=torch.long),
                                   torch.tensor([len(t) for t in tg], dtype=torch.long), blank=BLANK, reduction="none",
                                   zero_infinity=False).numpy()
    return out


def finals(losses, L, span, penalty: float) -> tuple[np.ndarray, np.ndarray]:
    """(norm float32, final float64): norm = loss / L in float32; final = -(double)norm - penalty * (span - 1) in double"""
    norm = np.asarray(losses, np.float32) / np.asarray(L).astype(np.float32)
    return norm, -norm.astype(np.float64) - np.float64(penalty) * (np.asarray(span).astype(np.float64) - 1.0)


def rank(losses, L, span, penalty: float, k: int) -> np.ndarray:
    """indices of the first k keys by final descending; the arrays are in ascending key order, so the stable sort sends ties
    to the smaller verse, then the smaller span"""
    _, fin = finals(losses, L, span, penalty)
    return np.argsort(-fin, kind="stable")[:k]
