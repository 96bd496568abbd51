"""Python restatement of the rule by which a recording of any length is cut into windows and stitched again
(include/qverse.h, "recordings of any length"; csrc/qv_long_plan.h).  No GPU and no kernel.

    plan(n, max_samples, window_samples=0, margin_frames=-1) -> Plan, or raises BadPlan (QV_ERR_ARG) / TooLong (QV_ERR_CAPACITY)
    Plan.windows()                 [(start sample, samples, forward length, lo, hi)] per window; [lo, hi) = the GLOBAL frames it owns
    cut_logprobs(lp, plan, t_max)  the window tensors of a global [T, 1025] matrix, NaN wherever the long path must not look
    stitch(window_lps, plan)       the global [T, 1025] matrix from per-window log-probs: owned frames only"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

HOP = 1280            # samples per encoder frame
MAX_FRAMES = 262144   # QV_LONG_MAX_FRAMES
MIN_SAMPLES = 400     # the forward's minimum


class BadPlan(ValueError):
    pass


class TooLong(ValueError):
    pass


def frames(n: int) -> int:
    return n // HOP + 1


@dataclass(frozen=True)
class Plan:
    n: int
    kw: int
    m: int
    h: int
    t_total: int
    n_windows: int

    @property
    def window_samples(self) -> int:
        return self.kw * HOP

    def start(self, w: int) -> int:
        return HOP * w * self.h

    def length(self, w: int) -> int:
        return min(HOP * self.kw, self.n - self.start(w))

    def fwd_length(self, w: int) -> int:
        """what the forward is told: a last window under 400 samples (margin 0 only) runs as 400, zeros behind"""
        n = self.length(w)
        return MIN_SAMPLES if w > 0 and n < MIN_SAMPLES else n

    def lo(self, w: int) -> int:
        return 0 if w == 0 else w * self.h + self.m

    def hi(self, w: int) -> int:
        return self.t_total if w == self.n_windows - 1 else (w + 1) * self.h + self.m

    def windows(self):
        return [(self.start(w), self.length(w), self.fwd_length(w), self.lo(w), self.hi(w)) for w in range(self.n_windows)]


def plan(n: int, max_samples: int, window_samples: int = 0, margin_frames: int = -1) -> Plan:
    if n < 0 or max_samples < HOP or window_samples < 0 or margin_frames < -1:
        raise BadPlan("negative argument, or no room for one frame")
    if window_samples == 0:
        window_samples = max_samples // HOP * HOP
    if window_samples % HOP or window_samples > max_samples:
        raise BadPlan("window_samples: a multiple of 1280, at most max_samples")
    kw = window_samples // HOP
    m = min(50, kw // 4) if margin_frames < 0 else margin_frames
    h = kw - 2 * m
    if h < 1:
        raise BadPlan("window - 2 margins < 1 frame")
    if frames(n) > MAX_FRAMES:
        raise TooLong(n)
    nw = 1
    if n > window_samples:
        while HOP * ((nw - 1) * h + kw) < n:   # the smallest nw whose windows reach the end
            nw += 1
    return Plan(n, kw, m, h, frames(n), nw)


def cut_audio(x: np.ndarray, p: Plan) -> list[np.ndarray]:
    """the windows' samples (not padded)"""
    return [np.asarray(x[s: s + ln], np.float32) for s, ln, _, _, _ in p.windows()]


def cut_logprobs(lp: np.ndarray, p: Plan, t_max: int) -> np.ndarray:
    """float32 [n_windows, t_max, 1025]: window w holds the global frames it OWNS at their local index; every other entry
    -- margins, frames past the window's length, rows past its frames -- is NaN"""
    assert lp.shape == (p.t_total, 1025) and t_max >= p.kw + 1
    out = np.full((p.n_windows, t_max, 1025), np.nan, np.float32)
    for w, (_, _, _, lo, hi) in enumerate(p.windows()):
        out[w, lo - w * p.h: hi - w * p.h] = lp[lo:hi]
    return out


def stitch(window_lps, p: Plan) -> np.ndarray:
    """window_lps[w]: float32 [>= frames of window w, 1025] -> the global [T, 1025]: frame t from the window that owns it"""
    out = np.full((p.t_total, 1025), np.nan, np.float32)
    for w, (_, ln, _, lo, hi) in enumerate(p.windows()):
        assert hi - w * p.h <= frames(ln) <= len(window_lps[w]), (w, lo, hi, ln)
        out[lo:hi] = np.asarray(window_lps[w], np.float32)[lo - w * p.h: hi - w * p.h]
    assert not np.isnan(out).any()
    return out
