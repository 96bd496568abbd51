#!/usr/bin/env python
"""Cost of the exhaustive CTC scan (qv_scan_logprobs) next to the forward of the same batch, and next to the scan restricted
to 10 surahs per row (the reference's brute-force workload), in one process.

    python tools/scan_bench.py [--rows 64] [--steps 5] [--trials 5] [--out FILE]

Two shapes: `rows` clips of 10 s (126 encoder frames) and of 30 s (376 frames).  The log-probs are verse-shaped and resident in
HBM: row b spells a verse (two frames per token, one blank between, blank behind; boost 12 over unit noise, float32
log-softmax) whose tokens fit the frames.

    scan_all       qv_scan_logprobs at the C ABI: no mask, max_span 6, k = 5, span penalty 0.5
    scan_10        the same with a mask of 10 surahs per row: the spelled verse's and the nine that follow it
    forward        Engine.forward (seeded random weights) on `rows` synthetic clips of that length

Every figure of the first table is host wall-clock per call around work that ends in a device synchronise.  A trial times
`steps` calls of ONE variant; the variants alternate within a trial round, `trials` rounds; reported are the median over the
rounds and their minimum and maximum.  Every variant is warmed up at its shape first (the first scan also allocates the
workspace).  Entry 0 of every row is compared with the verse it spells before anything is timed.
The per-kernel split (k_ctc_scan, k_scan_select) comes from HIP events around the two launches (qv_profile_stages +
qv_scan_kernel_times) in a separate pass of `trials` calls per variant, median; state_steps is qv_scan_stats' count for the
batch, and steps_per_s = state_steps / the scoring kernel's time.  One JSON line; --out also writes it to a file.
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import SCAN_ENTRY_DTYPE, SCAN_INFO_DTYPE, Engine, scan_stats, surah_mask
    from synth import frame_path, synth_audio

    B = args.rows
    shapes = {"10s": 160000, "30s": 480000}
    eng = Engine(device=0, with_model=True, max_batch=B, max_samples=max(shapes.values()))
    tab = eng.tables
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731

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

    out = {"rows": B, "steps": args.steps, "trials": args.trials, "max_span": 6, "k": 5, "span_penalty": 0.5, "shapes": {}}
    rng = np.random.default_rng(20260630)
    for tag, n_samples in shapes.items():
        T = eng.frames_for(n_samples)
        # the longest verses that still fit: 3 frames per token
        lens = np.array([len(tab.token_ids(v, 1)) for v in range(tab.n_verses)])
        fit = np.flatnonzero((lens * 3 <= T) & (lens > 0))
        verses = np.resize(fit[np.argsort(-lens[fit], kind="stable")][:B], B)
        lg = rng.standard_normal((B, T, 1025)).astype(np.float32)
        for b, v in enumerate(verses):
            lg[b, np.arange(T), frame_path(tab.token_ids(int(v), 1), T, 2)] += np.float32(12.0)
        lp = torch.log_softmax(torch.from_numpy(lg), -1).cuda().contiguous()
        frames = np.full(B, T, np.int32)
        lp_ptr = C.c_void_p(lp.data_ptr())
        info, ent = np.zeros(B, SCAN_INFO_DTYPE), np.zeros((B, 5), SCAN_ENTRY_DTYPE)
        ten = [[(int(tab.surah[v]) - 1 + j) % 114 + 1 for j in range(10)] for v in verses]
        mask10 = np.ascontiguousarray(np.stack([surah_mask(s) for s in ten]))

        def scan(mask):
            rc = eng.lib.qv_scan_logprobs(eng.h, lp_ptr, p(frames), B, T, 6, 0.5, 5, p(mask), p(info), p(ent), None, None)
            assert rc == 0, eng.lib.qv_last_error(eng.h)

        res = {"frames": T, "mean_tokens": round(float(lens[verses].mean()), 1)}
        for name, mask in (("scan_all", None), ("scan_10", mask10)):
            scan(mask)
            # entry 0 is the spelled verse, or an earlier verse with the same tokens
            for b, v in enumerate(verses):
                e = ent[b, 0]
                assert e["span"] == 1 and e["start_verse"] <= v and np.array_equal(tab.token_ids(int(e["start_verse"]), 1), tab.token_ids(int(v), 1)), (tag, name, b)
            per_mask = {s: scan_stats(T, 6, list(s))["state_steps"] for s in {tuple(x) for x in ten}} if mask is not None else {}
            steps = sum(per_mask[tuple(x)] for x in ten) if mask is not None else B * scan_stats(T, 6)["state_steps"]
            res[name + "_keys"] = int(info["n_feasible"].sum())
            res[name + "_recursions"] = int(info["n_recursions"].sum())
            res[name + "_state_steps"] = int(steps)
        audio = torch.from_numpy(np.ascontiguousarray(synth_audio(B, n_samples), np.float32)).cuda()
        lengths = [n_samples] * B
        res.update(spread({"scan_all": lambda: scan(None), "scan_10": lambda: scan(mask10), "forward": lambda: eng.forward(audio, lengths)}))
        # the kernels on their own: HIP events around the two launches
        eng.profile_stages(True)
        for name, mask in (("scan_all", None), ("scan_10", mask10)):
            ks = []
            for _ in range(max(args.trials, 3)):
                scan(mask)
                ks.append(eng.scan_kernel_times())
            score = statistics.median(k["score"] for k in ks)
            res[name]["k_ctc_scan_ms"] = round(score * 1e3, 4)
            res[name]["k_scan_select_ms"] = round(statistics.median(k["select"] for k in ks) * 1e3, 4)
            res[name]["steps_per_s"] = float(f"{res[name + '_state_steps'] / score:.4g}")
        eng.profile_stages(False)
        res["scan_all_over_forward"] = round(res["scan_all"]["median_ms"] / res["forward"]["median_ms"], 3)
        out["shapes"][tag] = res
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
