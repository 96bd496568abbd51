#!/usr/bin/env python
"""Cost of transcribing recordings longer than the engine's capacity (Engine.transcribe_long: qv_transcribe_long) next to the
same windows through the call that existed before it, in one process.

    python tools/long_bench.py [--steps 4] [--trials 5] [--max-batch 16] [--out FILE]

Two shapes, seeded random weights, the default engine capacity (30 s windows, 50 frames of margin):
    R = 1 recording of 10 minutes, R = 8 recordings of 5 minutes (synthetic audio resident in HBM).

  long      Engine.transcribe_long on the [R, N] audio: gather, forward and per-frame argmax per round of max_batch windows,
            one collapse, one record per recording back
  windows   the SAME windows, cut beforehand into a zero-padded [n_windows, window_samples] tensor in HBM, through
            Engine.transcribe_batch(confidence=True) max_batch at a time: what the library offered before (no stitching:
            one transcript per window) -- its code is unchanged, so this is the time the parent commit needs

Every figure is host wall-clock per call around work that ends in a device synchronise (both paths are synchronous).  A trial
times `steps` calls of ONE variant; the variants alternate within a trial round, `trials` rounds; reported are the median
over the rounds and their minimum and maximum (the spread), the same per window, and audio seconds per second.  Every variant
is warmed up at its shape first.  The share of a long call spent in its own three kernels comes from HIP events around
their launches (qv_profile_stages + qv_long_kernel_times) in a separate pass, so the events do not sit in the timed calls.
One JSON line; --out also writes it to a file.
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
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import QV_LONG_HOP, Engine
    from synth import synth_audio

    eng = Engine(device=0, with_model=True, max_batch=args.max_batch)
    B = eng.max_batch

    def spread(fns: dict) -> dict:
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
        return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
                for k, v in got.items()}

    out = {"max_batch": B, "max_samples": eng.max_samples, "steps": args.steps, "trials": args.trials, "shapes": {}}
    base = synth_audio(1, 16000 * 600)[0]
    for tag, rows, seconds in (("1x10min", 1, 600), ("8x5min", 8, 300)):
        n = 16000 * seconds
        lengths = [n - 777 * r for r in range(rows)]                         # ragged by a little
        host = np.stack([base[r * 1000: r * 1000 + n] * np.float32(1.0 - 0.03 * r) for r in range(rows)])
        for r, ln in enumerate(lengths):
            host[r, ln:] = 0.0
        audio = torch.from_numpy(np.ascontiguousarray(host, np.float32)).cuda()
        plans = [eng.long_plan(ln) for ln in lengths]
        window, hop = plans[0]["window_samples"], plans[0]["hop_frames"] * QV_LONG_HOP
        n_win = sum(p["n_windows"] for p in plans)
        cut = torch.zeros((n_win, window), dtype=torch.float32, device="cuda")
        cut_len, k = [], 0
        for r, (ln, p) in enumerate(zip(lengths, plans)):
            for w in range(p["n_windows"]):
                m = min(window, ln - w * hop)
                cut[k, :m] = audio[r, w * hop: w * hop + m]
                cut_len.append(max(m, 400))
                k += 1

        def long_call():
            return eng.transcribe_long(audio, lengths)

        def window_calls():
            res = []
            for s in range(0, n_win, B):
                res.extend(eng.transcribe_batch(cut[s: s + B], cut_len[s: s + B], confidence=True))
            return res

        got = long_call()
        assert [d["n_windows"] for d in got] == [p["n_windows"] for p in plans] and len(window_calls()) == n_win
        res = spread({"long": long_call, "windows": window_calls})
        for v in res.values():
            v["ms_per_window"] = round(v["median_ms"] / n_win, 3)
            v["audio_s_per_s"] = round(sum(lengths) / 16000 / (v["median_ms"] / 1e3), 1)
        eng.profile_stages(True)
        shares = []
        for _ in range(3):
            t0 = time.perf_counter()
            long_call()
            total = (time.perf_counter() - t0) * 1e3
            km = eng.long_kernel_times()
            shares.append({**{k: round(v, 4) for k, v in km.items()}, "call_ms": round(total, 3),
                           "share": round(sum(km.values()) / total, 5)})
        eng.profile_stages(False)
        res["long_kernels_ms"] = shares
        res.update({"rows": rows, "n_windows": n_win, "t_frames": [p["t_frames"] for p in plans], "window_samples": window,
                    "margin_frames": plans[0]["margin_frames"], "mean_tokens": round(float(np.mean([d["n_tokens"] for d in got])), 1)})
        out["shapes"][tag] = res
        del audio, cut
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
