#!/usr/bin/env python
"""Cost of the device n-best read-out (qv_nbest_results_ctx) next to the fetch of the plain results
(qv_fetch_results_ctx) on the same finished batch, in one process.

    python tools/nbest_bench.py [--steps 200] [--rows 64] [--frames 126]

Workload: `rows` verse-shaped log-prob matrices that FAIL the 0.80 text gate (the gate-fail recipe of bench.py's
realistic_mix leg: tests/synth.py, noise 3.5, boost 4.0, two frames per token), so every row has a reranked candidate
list for k_nbest to rank.  (At the default 126 frames the recipe's garbled transcripts draw long verses and only a couple
of candidates per row satisfy 2L + 1 <= T, so the selection ends after three rounds: --frames 376 makes most of the list
feasible and all k rounds run; "mean_ranked" in the output says which case was measured.)  The batch is decoded once; then both calls are timed at the C ABI on arrays built once, k = 5
and k = 32.  Both are synchronous (join, kernel or none, one device-to-host copy, host scatter), so the figure is host
wall-clock per call; for kernel time alone run it under `rocprofv3 --kernel-trace --stats` and read k_nbest next to
k_result, the nearest existing kernel (one block per utterance, the same pass over the candidate arrays): --decodes N
repeats the decode N times so that both kernels have as many launches.  One JSON line.
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=126)
    ap.add_argument("--decodes", type=int, default=1, help="decode + one n-best call per k this many times (kernel-trace runs)")
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import NBEST_ENTRY_DTYPE, NBEST_INFO_DTYPE, RESULT_DTYPE, Engine
    from synth import synth_logits

    B, T = args.rows, args.frames
    eng = Engine(device=0, with_model=False, max_batch=B, max_samples=480000)
    rng = np.random.default_rng(20260630)
    n_verses = len(eng.tables.s["tok_off"]) // 6
    lps = []
    while len(lps) < B:
        ids = eng.tables.token_ids(int(rng.integers(0, n_verses)), 1).tolist()
        if not (4 <= len(ids) and 2 * len(ids) + 1 <= T):
            continue
        lps.append(torch.log_softmax(torch.from_numpy(synth_logits(ids, T, seed=9000 + len(lps), noise=3.5, boost=4.0, rep=2)), -1))
    lp = torch.stack(lps).cuda().contiguous()
    for _ in range(max(1, args.decodes)):
        res = eng.decode_retrieve_rerank(lp, [T] * B, want_text=False)
        lists = {k: eng.nbest_results(batch=B, k=k) for k in (5, 32)}       # (first call: workspace allocation, code load)
    assert all(l5 == l32[:5] for l5, l32 in zip(lists[5], lists[32]))
    for r, lst in zip(res, lists[32]):
        assert not lst or (lst[0]["surah"], lst[0]["ayah"], lst[0]["ayah_end"]) == (r["surah"], r["ayah"], r["ayah_end"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    info, ent = np.zeros(B, NBEST_INFO_DTYPE), np.zeros((B, 32), NBEST_ENTRY_DTYPE)
    rows = np.zeros(B, RESULT_DTYPE)
    ctx = int(eng.lib.qv_last_context(eng.h))

    def nbest(k):
        assert eng.lib.qv_nbest_results_ctx(eng.h, ctx, B, k, 0, p(info), p(ent)) == 0

    def fetch():
        assert eng.lib.qv_fetch_results_ctx(eng.h, ctx, B, T, p(rows), None) == 0

    torch.cuda.synchronize()
    ms = {}
    for name, fn in (("nbest5", lambda: nbest(5)), ("nbest32", lambda: nbest(32)), ("fetch", fetch),
                     ("nbest5_again", lambda: nbest(5)), ("nbest32_again", lambda: nbest(32)), ("fetch_again", fetch)):
        fn()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        ms[name] = (time.perf_counter() - t0) * 1e3 / args.steps
    print(json.dumps({"rows": B, "frames": T, "steps": args.steps,
                      "use_ctc_rows": sum(r["use_ctc"] for r in res),
                      "mean_candidates": round(sum(r["n_candidates"] for r in res) / B, 1),
                      "mean_ranked": round(float(info["n_ranked"].mean()), 1),
                      "mean_entries_k32": round(float(info["n_entries"].mean()), 2),
                      "qv_nbest_results_ctx_k5_ms_per_call": round(min(ms["nbest5"], ms["nbest5_again"]), 4),
                      "qv_nbest_results_ctx_k5_ms_per_call_runs": [round(ms["nbest5"], 4), round(ms["nbest5_again"], 4)],
                      "qv_nbest_results_ctx_k32_ms_per_call": round(min(ms["nbest32"], ms["nbest32_again"]), 4),
                      "qv_nbest_results_ctx_k32_ms_per_call_runs": [round(ms["nbest32"], 4), round(ms["nbest32_again"], 4)],
                      "qv_fetch_results_ctx_ms_per_call": round(min(ms["fetch"], ms["fetch_again"]), 4),
                      "qv_fetch_results_ctx_ms_per_call_runs": [round(ms["fetch"], 4), round(ms["fetch_again"], 4)],
                      "nbest_record_bytes_per_call": B * (16 + 32 * 56), "result_bytes_per_call": B * RESULT_DTYPE.itemsize}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
