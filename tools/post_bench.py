#!/usr/bin/env python
"""Post-logits stages alone (greedy decode -> retrieval -> CTC rerank) on verse-shaped log-probs:
what they cost when the transcript is a real recitation rather than the near-empty string the
random-weight benchmark produces.  Log-probs come from the tests' synthetic recipe (a frame path
through a verse's token ids + hashed noise); verses are drawn with a fixed seed.

    python tools/post_bench.py [--batch 64] [--frames 126] [--steps 20]
    python tools/post_bench.py --chars 1400 --max-transcript 2048      # long recitations on the wide matching window

--chars N replaces the four cases by two: runs of consecutive ayat whose transcripts have about N characters (within 15 %),
as token paths with a blank only between equal neighbours (one frame per token: what fits 61 s of audio), clean (gate
passes) and with 35 % of the tokens replaced (gate fails -> search, pass 3, CTC rerank).  --max-transcript picks the
engine's matching window (1024 / 2048): the same --chars 500 inputs on both show what the wide kernel set costs for work
the default set can do, --chars 1400 needs the wide one (the default window withholds those: the row says so).

--dump PATH writes, case after case, the raw qv_result records of the batch and its ranked alternatives at k = 5 (the
qv_nbest_info records, then the entries, those past a row's n_entries zeroed): run it with two builds of the library
(QVERSE_LIB) or two settings of a kernel switch and compare the files byte for byte.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=126)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--case", type=int, default=-1, help="run only this case (0 = clean / gate passes ... 3 = noisy); default all")
    ap.add_argument("--chars", type=int, default=0, help="transcripts of about this many characters (runs of consecutive ayat) instead of single verses")
    ap.add_argument("--max-transcript", type=int, default=1024, choices=(1024, 2048), help="the engine's matching window")
    ap.add_argument("--dump", default=None, help="write every case's raw result records and n-best entries (k = 5) to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import RESULT_DTYPE, Engine
    from synth import synth_logits

    B, T = args.batch, args.frames
    if args.chars:
        T = 763                                  # 61 s: the longest clip an engine can be created for
    eng = Engine(device=0, with_model=False, max_batch=B, max_samples=976000 if args.chars else T * 1280 + 1280,
                 max_transcript=args.max_transcript)
    rng = np.random.default_rng(20260630)
    n_verses = len(eng.tables.s["tok_off"]) // 6
    rows = []
    dump = open(args.dump, "wb") if args.dump else None
    cases = (("clean (gate passes)", 1.0, 8.0), ("corrupted", 2.0, 6.0), ("corrupted more", 2.4, 6.0),
             ("noisy (gate fails -> CTC rerank)", 3.5, 4.0))
    if args.chars:
        cases = (("clean (gate passes)", 0.0, 12.0), ("35 % of the tokens replaced (gate fails -> CTC rerank)", 0.35, 12.0))
    for name, noise, boost in (cases if args.case < 0 else cases[args.case: args.case + 1]):
        lps, used = [], 0
        while args.chars and len(lps) < B:
            from synth import BLANK, VOCAB, hash_noise

            v, span = int(rng.integers(0, n_verses - 6)), int(rng.integers(1, 7))
            tb = eng.tables
            if tb.surah[v] != tb.surah[v + span - 1]:
                continue
            chars = int(tb.s["clean_off"][v + span]) - int(tb.s["clean_off"][v]) + span - 1
            if not (0.85 * args.chars <= chars <= 1.15 * args.chars):
                continue
            ids = [int(rng.integers(1, 1024)) if rng.random() < noise else int(t) for t in tb.token_ids(v, span).tolist()]
            path = []
            for tok in ids:                      # a blank only between equal neighbours
                if path and path[-1] == tok:
                    path.append(BLANK)
                path.append(tok)
            if len(path) > T:
                continue
            path += [BLANK] * (T - len(path))
            lg = hash_noise((T, VOCAB), 1000 + used)
            lg[np.arange(T), np.asarray(path)] += np.float32(boost)
            lps.append(torch.log_softmax(torch.from_numpy(lg), -1))
            used += 1
        while len(lps) < B:
            v = int(rng.integers(0, n_verses))
            ids = eng.tables.token_ids(v, 1).tolist()
            if not (4 <= len(ids) and 2 * len(ids) + 1 <= T):
                continue
            lg = torch.from_numpy(synth_logits(ids, T, seed=1000 + used, noise=noise, boost=boost, rep=2))
            lps.append(torch.log_softmax(lg, -1))
            used += 1
        lp = torch.stack(lps).cuda().contiguous()
        res = eng.decode_retrieve_rerank(lp, [T] * B)
        if dump:
            raw = np.zeros(B, dtype=RESULT_DTYPE)
            t = np.full(B, T, dtype=np.int32)
            eng._check(eng.lib.qv_decode_retrieve_rerank(eng.h, lp.data_ptr(), t.ctypes.data, B, T, raw.ctypes.data, None, eng._stream()),
                       "qv_decode_retrieve_rerank")
            info, ent = eng.nbest_raw(batch=B, k=5)
            for b in range(B):
                ent[b, int(info[b]["n_entries"]):] = 0
            for a in (raw, info, ent):
                dump.write(a.tobytes())
        for _ in range(3):
            eng.decode_retrieve_rerank(lp, [T] * B, want_text=False)
        regions = []
        for _ in range(3):      # a region is ~60 ms of synchronous calls: one host hiccup doubles it (seen in round 5) -> median of three
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.decode_retrieve_rerank(lp, [T] * B, want_text=False)
            torch.cuda.synchronize()
            regions.append((time.perf_counter() - t0) / args.steps)
        dt = sorted(regions)[1]
        row = {"case": name, "batch": B, "frames": T, "max_transcript": eng.max_transcript,
               "withheld": sum(bool(r["flags"] & 2) for r in res), "ms_per_batch": round(dt * 1e3, 3),
               "regions_ms": [round(r * 1e3, 3) for r in regions],
               "gate_failed": sum(r["use_ctc"] for r in res),
               "mean_candidates": round(sum(r["n_candidates"] for r in res) / B, 1),
               "mean_transcript_chars": round(sum(len(r["transcript"]) for r in res) / B, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if dump:
        dump.close()
    eng.close()


if __name__ == "__main__":
    main()
