#!/usr/bin/env python
"""Cost of the verse-constrained beam search (qv_beam_decode) next to qv_transcribe on the same tensor and next to the forward
of the same batch, in one process.

    python tools/beam_bench.py [--rows 64] [--steps 20] [--trials 5] [--out FILE]

Two shapes: `rows` clips of 10 s (126 encoder frames) and of 30 s (376 frames).  The log-probs are verse-shaped and resident in
HBM: row b spells a verse (two frames per token, one blank between, blank behind; boost 12 over unit noise, float32
log-softmax) whose tokens fit the frames, so the search walks deep into the trie instead of idling at the root.

    beam_w8 / beam_w32    qv_beam_decode at the C ABI, max_span 3, k = 5, token ids of the best hypothesis included
    qv_transcribe         the greedy kernel on the same tensor
    forward               Engine.forward (seeded random weights) on `rows` synthetic clips of that length

Every figure is host wall-clock per call around work that ends in a device synchronise.  A trial times `steps` calls of ONE
variant; the variants alternate within a trial round, `trials` rounds; reported are the median over the rounds and their
minimum and maximum.  Every variant is warmed up at its shape first (the first beam call also builds and uploads the trie).
The best hypothesis of every row is compared with the verse it spells before anything is timed.  One JSON line; --out also
writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import BEAM_ENTRY_DTYPE, BEAM_INFO_DTYPE, TRANSCRIPT_INFO_DTYPE, Engine
    from synth import frame_path, synth_audio

    B = args.rows
    shapes = {"10s": 160000, "30s": 480000}
    eng = Engine(device=0, with_model=True, max_batch=B, max_samples=max(shapes.values()))
    tab = eng.tables
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def spread(fns: dict) -> dict:
        """alternating trials; ms per call: median, min, max over the rounds"""
        for fn in fns.values():
            fn()
            fn()
        torch.cuda.synchronize()
        got = {k: [] for k in fns}
        for _ in range(args.trials):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                got[k].append((time.perf_counter() - t0) * 1e3 / args.steps)
        return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                for k, v in got.items()}

    out = {"rows": B, "steps": args.steps, "trials": args.trials, "max_span": 3, "k": 5, "shapes": {}}
    rng = np.random.default_rng(20260630)
    for tag, n_samples in shapes.items():
        T = eng.frames_for(n_samples)
        # the longest verses that still fit: 3 frames per token
        lens = np.array([len(tab.token_ids(v, 1)) for v in range(tab.n_verses)])
        fit = np.flatnonzero((lens * 3 <= T) & (lens > 0))
        verses = fit[np.argsort(-lens[fit], kind="stable")][:B]
        verses = np.resize(verses, B)
        lg = rng.standard_normal((B, T, 1025)).astype(np.float32)
        for b, v in enumerate(verses):
            lg[b, np.arange(T), frame_path(tab.token_ids(int(v), 1), T, 2)] += np.float32(12.0)
        lp = torch.log_softmax(torch.from_numpy(lg), -1).cuda().contiguous()
        frames = np.full(B, T, np.int32)
        lp_ptr = C.c_void_p(lp.data_ptr())
        b_info, b_ent = np.zeros(B, BEAM_INFO_DTYPE), np.zeros((B, 5), BEAM_ENTRY_DTYPE)
        b_ids = np.zeros((B, T), np.int32)
        t_info = np.zeros(B, TRANSCRIPT_INFO_DTYPE)
        t_ids = np.zeros((B, T), np.int32)

        def beam(W):
            rc = eng.lib.qv_beam_decode(eng.h, lp_ptr, p(frames), B, T, 3, W, 5, p(b_info), p(b_ent), p(b_ids), T, None)
            assert rc == 0, eng.lib.qv_last_error(eng.h)

        def greedy():
            rc = eng.lib.qv_transcribe(eng.h, lp_ptr, p(frames), B, T, p(t_info), p(t_ids), None, None, None, T, None)
            assert rc == 0

        res = {"frames": T, "mean_tokens": round(float(lens[verses].mean()), 1)}
        for W in (8, 32):
            beam(W)
            for b, v in enumerate(verses):
                want = tab.token_ids(int(v), 1).tolist()
                assert b_ent[b, 0]["flags"] & 1 and b_ids[b, : len(want)].tolist() == want and b_ids[b, len(want)] == -1, (tag, W, b)
            res[f"max_candidates_w{W}"] = int(b_info["max_candidates"].max())
        audio = torch.from_numpy(np.ascontiguousarray(synth_audio(B, n_samples), np.float32)).cuda()
        lengths = [n_samples] * B
        res.update(spread({"beam_w8": lambda: beam(8), "beam_w32": lambda: beam(32), "qv_transcribe": greedy,
                           "forward": lambda: eng.forward(audio, lengths)}))
        out["shapes"][tag] = res
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
