#!/usr/bin/env python
"""Cost of the device correction (qv_correct) per call of `rows` rows, in one process, for three shapes:

    typical   a verse of about 60 symbols (67:1) against itself with a few edits
    long      2:282, the longest single verse (551 symbols), against itself with edits
    caps      both texts at the caps: 1,280 reference symbols in 288 words against a prediction that fills the window

    python tools/correct_bench.py [--steps 50] [--rows 64] [--window 1024]

Every row of a call holds the same pair, so a call is `rows` workgroups of equal length.  The call is synchronous (one copy
up, the kernel, one copy back, the host scatter); HIP events on the caller's stream bracket it, and the host clock around it
is reported next to them.  Warm-up: the first call per shape allocates the workspace and loads the code object and is not
timed.  Each shape is timed twice, alternating with the others; the smaller figure is reported with both runs beside it.
With --prefix the calls carry QV_CORRECT_PREFIX.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def edited(rng, codes, n_edits, alphabet=39):
    """the text with n_edits random substitutions, deletions and insertions of symbols (spaces stay)"""
    out = [int(c) for c in codes]
    for _ in range(n_edits):
        at = int(rng.integers(0, len(out)))
        kind = int(rng.integers(0, 3))
        if out[at] == 0:
            continue
        if kind == 0:
            out[at] = int(rng.integers(1, alphabet + 1))
        elif kind == 1:
            del out[at]
        else:
            out.insert(at, int(rng.integers(1, alphabet + 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--window", type=int, default=1024, choices=(1024, 2048))
    ap.add_argument("--prefix", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import CORRECT_MAX_REF, CORRECT_MAX_WORDS, Engine

    import correct_ref

    B = args.rows
    eng = Engine(device=0, with_model=False, max_batch=B, max_transcript=args.window)
    tb = eng.tables
    rng = np.random.default_rng(20261020)
    typical = tb.span_codes(tb.verse_index(67, 1), 1).tolist()
    long_ = tb.span_codes(tb.verse_index(2, 282), 1).tolist()
    cap_ref = []
    per_word = CORRECT_MAX_REF // CORRECT_MAX_WORDS
    sym = rng.integers(1, 40, CORRECT_MAX_REF).tolist()
    for w in range(CORRECT_MAX_WORDS):
        lo, hi = w * per_word, (w + 1) * per_word if w < CORRECT_MAX_WORDS - 1 else CORRECT_MAX_REF
        cap_ref += ([0] if w else []) + sym[lo:hi]
    cap_pred = (edited(rng, sym, 60) + rng.integers(1, 40, args.window).tolist())[: args.window]
    shapes = {"typical": (edited(rng, typical, 4), typical), "long": (edited(rng, long_, 25), long_), "caps": (cap_pred, cap_ref)}
    stream = torch.cuda.current_stream(0)
    out = {"rows": B, "window": args.window, "steps": args.steps, "prefix": args.prefix, "shapes": {}}
    runs = {k: [] for k in shapes}
    for name, (pred, ref) in shapes.items():                      # warm-up and a check of what is being timed
        row = eng.correct([pred] * B, [ref] * B, prefix=args.prefix)[0]
        want = correct_ref.correct(pred, ref, args.prefix, max_pred=args.window)
        assert {k: row[k] for k in correct_ref.INFO_FIELDS} == want["info"] and row["ops"].tolist() == want["ops"], name
        out["shapes"][name] = {"n_ref": row["n_ref"], "n_pred": row["n_pred"], "n_words": row["n_words"], "distance": row["distance"]}
    for _ in range(2):
        for name, (pred, ref) in shapes.items():
            preds, refs = [np.asarray(pred, np.uint8)] * B, [np.asarray(ref, np.uint8)] * B
            eng.correct_raw(preds, refs, args.prefix)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record(stream)
            for _ in range(args.steps):
                eng.correct_raw(preds, refs, args.prefix)
            end.record(stream)
            end.synchronize()
            runs[name].append((start.elapsed_time(end) / args.steps, (time.perf_counter() - t0) * 1e3 / args.steps))
    for name, r in runs.items():
        out["shapes"][name].update({"event_ms_per_call": round(min(x[0] for x in r), 4), "event_ms_per_call_runs": [round(x[0], 4) for x in r],
                                    "host_ms_per_call": round(min(x[1] for x in r), 4)})
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
