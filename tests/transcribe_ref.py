"""Numpy restatement of the transcription-with-confidence contract (include/qverse.h, "transcription with confidence";
csrc/qv_transcribe.hip, k_transcribe).  No GPU and no kernel.

    transcribe_ref(lp, T) -> dict   per-frame first-maximum argmax, runs of equal frame ids, one token per non-blank run
                                    (id, first / last frame, the run's maximum), the two float64 averages in the
                                    documented summation order, the minimum, the blank-frame count and the flag.

Two DELIBERATELY WRONG variants, which tests/test_transcribe_host.py shows the cases tell apart:
    logp="first"   a token's log-prob taken at the run's first frame instead of the run's maximum
    total=naive_sum   a sequential float64 sum instead of the lane-strided, then xor-butterfly one"""

from __future__ import annotations

import numpy as np

BLANK = 1024
FLAG_EMPTY = 1   # QV_FLAG_EMPTY_TRANSCRIPT


def lane_sum(x) -> np.float64:
    """the documented order: lane l of 64 adds x[l], x[l + 64], ... ascending from +0.0 in float64; then p[l] += p[l ^ o]
    for o = 32, 16, 8, 4, 2, 1"""
    x = np.asarray(x, np.float32).astype(np.float64)
    p = np.zeros(64, np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(0, len(x), 64):
            seg = x[i: i + 64]
            p[: len(seg)] = p[: len(seg)] + seg
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            p = p + p[idx ^ o]
    assert len({v.tobytes() for v in p}) == 1 or np.isnan(p).any()
    return p[0]


def naive_sum(x) -> np.float64:
    """DELIBERATELY WRONG: the elements one after the other"""
    s = np.float64(0.0)
    with np.errstate(invalid="ignore"):
        for v in np.asarray(x, np.float32).astype(np.float64):
            s = s + v
    return s


def frame_argmax(lp: np.ndarray, T: int):
    """fid [T] (numpy's first maximum) and m [T] = lp[t][fid[t]] as float32"""
    lp = np.asarray(lp, np.float32)[:T]
    fid = lp.argmax(axis=1).astype(np.int64) if T else np.zeros(0, np.int64)
    m = lp[np.arange(T), fid].astype(np.float32) if T else np.zeros(0, np.float32)
    return fid, m


def runs_of(fid: np.ndarray):
    """[(id, first, last)] of every run, blank runs included"""
    out, T = [], len(fid)
    t = 0
    while t < T:
        e = t
        while e + 1 < T and fid[e + 1] == fid[t]:
            e += 1
        out.append((int(fid[t]), t, e))
        t = e + 1
    return out


def transcribe_ref(lp: np.ndarray, T: int, logp: str = "max", total=lane_sum) -> dict:
    fid, m = frame_argmax(lp, T)
    ids, first, last, tok = [], [], [], []
    for i, a, e in runs_of(fid):
        if i == BLANK:
            continue
        seg = m[a: e + 1]
        ids.append(i)
        first.append(a)
        last.append(e)
        # the value at the first frame that attains the maximum (np.argmax: -0.0 and +0.0 tie, the earlier frame wins)
        tok.append(seg[int(np.argmax(seg))] if logp == "max" else seg[0])
    tok = np.asarray(tok, np.float32)
    n = len(ids)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = total(tok) / np.float64(n) if n else np.float64(0.0)
        favg = total(m) / np.float64(T) if T else np.float64(0.0)
    return {"ids": ids, "first": first, "last": last, "logp": tok, "fid": fid, "m": m,
            "n_tokens": n, "t_frames": int(T), "n_blank_frames": int((fid == BLANK).sum()),
            "min_token_logprob": tok[int(np.argmin(tok))] if n else np.float32(0.0),
            "avg_logprob": np.float64(avg), "frame_avg_logprob": np.float64(favg), "flags": 0 if n else FLAG_EMPTY}


def bits32(x) -> bytes:
    return np.asarray(x, np.float32).tobytes()


def bits64(x) -> bytes:
    return np.asarray(x, np.float64).tobytes()


def order_sensitive_values(n: int = 300, seed: int = 7) -> np.ndarray:
    """float32 values of magnitudes from about 1e-8 to 40, all negative like log-probs: their float64 sum depends on the
    order of the additions in its last bits"""
    rng = np.random.default_rng(seed)
    mag = np.exp(rng.uniform(np.log(1e-8), np.log(40.0), n))
    return (-mag).astype(np.float32)
