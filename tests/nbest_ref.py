"""Python restatement of the device's n-best selection (csrc/qv_nbest.hip) and of what the plugin makes of it, shared by
test_nbest_host.py and test_gpu_nbest.py.

The rerank's ranking is `ranked = [c for c in candidates if isfinite(c.ctc_norm_loss)]; ranked.sort(key=final_score,
reverse=True)` (the reference's c2c-direct/run.py:378-379): a STABLE descending sort, so equal scores keep candidate
order -- and Python compares floats the IEEE way, so -0.0 and +0.0 are equal scores.
"""

from __future__ import annotations

import math

import numpy as np

NBEST_MAX = 32
MARGIN = 2e-3        # what a float32 device loss may move a final score by (tests/test_gpu_postlogits.py)


def rank(finals, losses=None) -> list[int]:
    """Indices of the entries with a finite loss (losses=None: with a final that is not None), best first."""
    if losses is None:
        idx = [i for i, f in enumerate(finals) if f is not None]
    else:
        idx = [i for i, l in enumerate(losses) if l is not None and math.isfinite(float(l))]
    return sorted(idx, key=lambda i: float(finals[i]), reverse=True)


def select(finals, losses, k: int) -> list[int]:
    """what qv_nbest_select returns for one row"""
    return rank(finals, losses)[:k]


def text_row(base_start: int, base_span: int, base_score: float, runner_idx=(), runner_score=(), k: int = 5,
             runners: bool = False) -> list[dict]:
    """The list of a row the text match decided: the base, then (runners=True) match_verse's runners-up in its order,
    unrounded, without the runner that is a single-verse base itself."""
    out = [{"start": int(base_start), "span": int(base_span), "score": float(base_score)}]
    if runners:
        for v, s in zip(runner_idx, runner_score):
            if base_span == 1 and int(v) == int(base_start):
                continue
            out.append({"start": int(v), "span": 1, "score": float(s)})
    return out[:k]


def shape_candidates(entries, k: int = 5) -> list[dict]:
    """The reference's "candidates" (c2c-direct/run.py:424-435) from ranked entries {"surah", "ayah", "ayah_end", "score"}:
    the first k, ayah_end filled in, the score rounded to 4 places."""
    return [{"surah": e["surah"], "ayah": e["ayah"], "ayah_end": e.get("ayah_end") or e["ayah"],
             "score": round(float(e["score"]), 4)} for e in list(entries)[:k]]


def reference_final(loss, length, text_score=0.0, span=1, text_weight=0.0, span_penalty=0.5) -> float:
    """final_score of run.py:363-376 from a float32 loss: the normalised loss is a float32 division"""
    norm = np.float32(loss) / np.float32(length)
    return -float(norm) + text_weight * float(text_score) - span_penalty * (span - 1)


def tie_groups(finals, same_tokens, margin: float = MARGIN) -> list[int]:
    """Group id per rank of a ranked list of final scores: neighbours share a group when they are NEAR -- within `margin`
    of each other without being an exact tie of identical token lists (same_tokens(i, j); such a tie has one loss on the
    device as well, so candidate order decides it on both sides).  A rank alone in its group has to hold the same
    candidate on the device."""
    groups, g = [], 0
    for i in range(len(finals)):
        if i:
            d = abs(finals[i] - finals[i - 1])
            if not (d <= margin and not (d == 0.0 and same_tokens(i - 1, i))):
                g += 1
        groups.append(g)
    return groups
