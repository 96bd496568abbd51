"""numpy restatement of the long CTC alignment (csrc/qv_align_long.hip; include/qverse.h, "word and verse timings for
recordings of any length"), shared by the long alignment tests.  Not itself a test.

Ownership is long_ref's: a recording's window tensors (long_ref.cut_logprobs, or `poisoned` below) are stitched back into the
global [T, 1025] matrix by long_ref.stitch -- frame t from the window that owns it -- and the Viterbi pass runs on that.

The recursion is align_ref.viterbi's (float32, NEG = -1e30, one add per state and frame, the smaller step wins a tie, the
end rule) without its 383-token limit: up to MAX_TOKENS = 16,383.  Back-pointers are int8 [T, S], four states to a byte
above 2**26 entries (S = 32,767 and T = 16,500 would be 0.55 GB unpacked).  The per-token log-prob is summed sequentially in
float32, in ascending t, as the device sums it; the tests still allow align_ref's bound of n_frames * 2**-23 relative.
"""

from __future__ import annotations

import numpy as np

import long_ref as L

NEG = np.float32(-1e30)
BLANK = 1024
NO_TARGET, TOO_LONG, INFEASIBLE = 1, 2, 4
MAX_TOKENS = 16383
MAX_BYTES = 1 << 32
PACK_ABOVE = 1 << 26   # back-pointer entries above which four states share a byte


def ns_of(n_tokens: int) -> int:
    """states per thread of the instantiation that runs a target (csrc/qv_align_long_plan.h); 0 = the row does not run"""
    if n_tokens < 1 or n_tokens > MAX_TOKENS:
        return 0
    s = 2 * n_tokens + 1
    return 4 if s <= 4096 else 8 if s <= 8192 else 16 if s <= 16384 else 32


def threads_of(n_tokens: int) -> int:
    ns = ns_of(n_tokens)
    return -(-(-(-(2 * n_tokens + 1) // ns)) // 64) * 64 if ns else 0


def workspace_bytes(frames, n_tokens) -> int:
    """the header's formula: kept rows T * 1025 * 4 rounded up to 16, back-pointers T * threads * NS / 4"""
    return sum(((t * 1025 * 4 + 15) & ~15) + t * threads_of(n) * ns_of(n) // 4 for t, n in zip(frames, n_tokens))


def poisoned(lp: np.ndarray, p: L.Plan, t_max: int, ids) -> np.ndarray:
    """long_ref.cut_logprobs with +100 on every token that is NOT in the target (and not the blank) wherever cut_logprobs
    leaves NaN: a kernel that read such a frame would find a far better path through it"""
    out = L.cut_logprobs(lp, p, t_max)
    wrong = np.ones(1025, bool)
    wrong[np.asarray(ids, np.int64)] = False
    wrong[BLANK] = False
    row = np.where(wrong, np.float32(100.0), np.float32(-100.0)).astype(np.float32)
    hole = np.isnan(out[:, :, 0])
    out[hole] = row
    return out


def stitched(windows: np.ndarray, p: L.Plan) -> np.ndarray:
    return L.stitch([windows[w] for w in range(p.n_windows)], p)


def viterbi(lp: np.ndarray, ids, ties: bool = False) -> dict:
    """lp: float32 [T, 1025]; ids: target token ids (0..1023).  Returns {"flags", "score" (np.float32), "first", "last"
    (int arrays [L]), "logp" (float32 [L]), "path" (state per frame)}; with ties=True also "tie01" / "tie12": the frames
    at which, in the path's own state, stay == s-1 was the maximum / s-1 == s-2 (allowed) was the maximum."""
    ids = np.asarray(ids, dtype=np.int64)
    n, T = len(ids), int(lp.shape[0])
    none = {"flags": 0, "score": np.float32(0), "first": np.full(n, -1), "last": np.full(n, -1), "logp": np.zeros(n, np.float32), "path": None}
    if n == 0:
        return dict(none, flags=NO_TARGET)
    if n > MAX_TOKENS:
        return dict(none, flags=TOO_LONG)
    if T < n + int(np.sum(ids[1:] == ids[:-1])):
        return dict(none, flags=INFEASIBLE)
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    S = 2 * n + 1
    ext = np.full(S, BLANK, dtype=np.int64)
    ext[1::2] = ids
    skip_ok = np.zeros(S, dtype=bool)
    skip_ok[3::2] = ids[1:] != ids[:-1]
    v = np.full(S, NEG, dtype=np.float32)
    v[0] = lp[0, BLANK]
    v[1] = lp[0, ids[0]]
    pack = T * S > PACK_ABOVE
    S4 = (S + 3) // 4
    bp = np.zeros((T, S4 if pack else S), dtype=np.uint8)
    tie = np.zeros((T, S), dtype=np.uint8) if ties else None
    c1 = np.full(S, NEG, dtype=np.float32)
    c2 = np.full(S, NEG, dtype=np.float32)
    step4 = np.zeros(S4 * 4, dtype=np.uint8)
    for t in range(1, T):
        c1[1:] = v[:-1]
        c2[2:] = v[:-2]
        c2[~skip_ok] = NEG
        m1 = c1 > v
        best = np.where(m1, c1, v)
        m2 = c2 > best
        if ties:
            tie[t] = ((v == c1) & (v >= c2)) | (((c1 == c2) & (c1 > v)) << 1)
        best = np.where(m2, c2, best)
        step = m1.astype(np.uint8)
        step[m2] = 2
        v = (best + lp[t, ext]).astype(np.float32)
        if pack:
            step4[:S] = step
            q = step4.reshape(-1, 4)
            bp[t] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
        else:
            bp[t] = step
    s = S - 1 if v[S - 1] >= v[S - 2] else S - 2
    score = v[s]
    if score < np.float32(-1e29):
        return dict(none, flags=INFEASIBLE)
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int((bp[t, s >> 2] >> (2 * (s & 3))) & 3) if pack else int(bp[t, s])
        path[t - 1] = s
    # every odd state is on the path (a step of two goes from a token state to the next one), in ascending order
    tok_frames = np.nonzero(path & 1)[0]
    tok_state = path[tok_frames] >> 1
    change = np.nonzero(np.diff(tok_state))[0]
    first = tok_frames[np.concatenate(([0], change + 1))]
    last = tok_frames[np.concatenate((change, [len(tok_frames) - 1]))]
    assert len(first) == n and (tok_state[np.concatenate(([0], change + 1))] == np.arange(n)).all()
    logp = np.zeros(n, np.float32)
    for i in range(n):
        assert (path[first[i]: last[i] + 1] == 2 * i + 1).all()
        acc = np.float32(0)
        for x in lp[first[i]: last[i] + 1, ids[i]]:
            acc = np.float32(acc + x)
        logp[i] = acc / np.float32(last[i] - first[i] + 1)
    out = {"flags": 0, "score": np.float32(score), "first": first, "last": last, "logp": logp, "path": path}
    if ties:
        on_path = tie[np.arange(1, T), path[1:]]
        out["tie01"] = np.nonzero(on_path & 1)[0] + 1
        out["tie12"] = np.nonzero(on_path & 2)[0] + 1
    return out
