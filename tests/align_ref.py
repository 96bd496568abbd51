"""numpy restatement of the device's CTC forced alignment (csrc/qv_align.hip), shared by the alignment tests.

Float32 throughout, natural-log units, the device's sentinel (NEG = -1e30), tie rule (the smaller step wins: stay beats
s-1 beats s-2, strict > when the larger step is considered) and final-state rule -- the only float operation per state
and frame is one float32 add, so the path score is comparable bit for bit.  The per-token mean log-prob is summed in
float64 here; the device sums in float32 (tolerance: n_frames * 2**-23 relative).
"""

from __future__ import annotations

import itertools

import numpy as np

from synth import synth_logits

NEG = np.float32(-1e30)
BLANK = 1024
NO_TARGET, TOO_LONG, INFEASIBLE = 1, 2, 4
MAX_TOKENS = 383


# (L, T, rep): token i planted at frames i*(rep+1) .. i*(rep+1)+rep-1 (synth.frame_path), noise 1.0, boost 12.0
PLANTED = [(1, 1, 1), (5, 16, 2), (40, 126, 2), (120, 376, 2), (33, 100, 2), (191, 768, 3)]


def planted_case(L, T, rep, seed=0):
    """(ids, float32 log-probs [T, 1025]): L ids, with ids[3] = ids[2] where L > 4, planted at rep frames per token"""
    import torch

    ids = ((np.arange(L) * 37 + 11 + seed) % 1024).astype(np.int64)
    if L > 4:
        ids[3] = ids[2]
    lg = synth_logits(ids.tolist(), T, seed=1000 + L + seed, noise=1.0, boost=12.0, rep=rep)
    return ids, torch.log_softmax(torch.from_numpy(lg), -1).numpy()


def viterbi(lp: np.ndarray, ids) -> dict:
    """lp: float32 [T, 1025] log-probs; ids: target token ids (0..1023).
    Returns {"flags", "score" (np.float32), "first", "last" (int arrays [L]), "logp" (float64 [L]), "path" (state per frame)}."""
    ids = np.asarray(ids, dtype=np.int64)
    L, T = len(ids), int(lp.shape[0])
    none = {"flags": 0, "score": np.float32(0), "first": np.full(L, -1), "last": np.full(L, -1), "logp": np.zeros(L), "path": None}
    if L == 0:
        return dict(none, flags=NO_TARGET)
    if L > MAX_TOKENS:
        return dict(none, flags=TOO_LONG)
    if T < L + int(np.sum(ids[1:] == ids[:-1])):
        return dict(none, flags=INFEASIBLE)
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    S = 2 * L + 1
    ext = np.full(S, BLANK, dtype=np.int64)
    ext[1::2] = ids
    skip_ok = np.zeros(S, dtype=bool)
    skip_ok[3::2] = ids[1:] != ids[:-1]
    v = np.full(S, NEG, dtype=np.float32)
    v[0] = lp[0, BLANK]
    v[1] = lp[0, ids[0]]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        best = v.copy()
        step = np.zeros(S, dtype=np.int8)
        c1 = np.concatenate(([NEG], v[:-1])).astype(np.float32)
        m = c1 > best
        best[m], step[m] = c1[m], 1
        c2 = np.concatenate(([NEG, NEG], v[:-2])).astype(np.float32)
        c2[~skip_ok] = NEG
        m = c2 > best
        best[m], step[m] = c2[m], 2
        v = (best + lp[t, ext]).astype(np.float32)
        bp[t] = step
    s = S - 1 if v[S - 1] >= v[S - 2] else S - 2
    score = v[s]
    if score < np.float32(-1e29):
        return dict(none, flags=INFEASIBLE)
    path = np.zeros(T, dtype=np.int64)
    path[T - 1] = s
    for t in range(T - 1, 0, -1):
        s -= int(bp[t, s])
        path[t - 1] = s
    first, last, logp = np.full(L, -1), np.full(L, -1), np.zeros(L)
    for i in range(L):
        fr = np.nonzero(path == 2 * i + 1)[0]
        first[i], last[i] = fr[0], fr[-1]
        assert len(fr) == last[i] - first[i] + 1
        logp[i] = lp[fr, ids[i]].astype(np.float64).sum() / len(fr)
    return {"flags": 0, "score": np.float32(score), "first": first, "last": last, "logp": logp, "path": path}


def brute_force_best(lp: np.ndarray, ids) -> float | None:
    """Best path score over ALL CTC alignments of ids to the T frames, by enumeration (tiny L, T only): every
    monotone state sequence over the blank-extended target that starts in state 0 / 1, ends in the last two states and
    moves by 0, 1, or 2 (2: onto a token that differs from the previous token).  float32 sum in frame order."""
    ids = list(ids)
    L, T = len(ids), lp.shape[0]
    S = 2 * L + 1
    ext = [BLANK] * S
    ext[1::2] = ids
    best = None
    for steps in itertools.product((0, 1, 2), repeat=T - 1):
        for s0 in (0, 1):
            s, ok = s0, True
            acc = np.float32(lp[0, ext[s]])
            for t, d in enumerate(steps, start=1):
                n = s + d
                if n >= S or (d == 2 and not (n % 2 == 1 and n > 1 and ext[n] != ext[n - 2])):
                    ok = False
                    break
                s = n
                acc = np.float32(acc + lp[t, ext[s]])
            if ok and s >= S - 2 and (best is None or acc > best):
                best = acc
    return best
