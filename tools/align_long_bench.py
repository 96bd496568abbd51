#!/usr/bin/env python
"""Cost of the long CTC alignment (qv_align_windows: k_long_keep + k_align_long) over a grid of (T, L) up to a whole-surah
shape, in one process.

    python tools/align_long_bench.py [--reps 3] [--small]

For each (frames T, tokens L) one recording is made ON THE DEVICE: noise around -9 with a planted path (token i over the
frames [i T / L, (i + 1) T / L), neighbours differ) lifted to about -0.5, cut into the window tensors of an engine of the
largest capacity (765-frame windows, the default margin).  qv_align_windows runs once to allocate the workspace, then `reps`
times with qv_profile_stages on; the figures are the engine's own HIP events around its kernels (best of the reps):
    keep_ms        k_long_keep over all rounds (owned rows to their global frame);
    d2d_ms         a plain device-to-device copy (hipMemcpyAsync through torch) of the same T * 4100 bytes, same events;
    align_ms       k_align_long: the recursion, the backward walk and the read-out;  us_per_frame = align_ms / T;
    call_ms        host wall-clock of the whole synchronous call (targets up, records back).
One JSON line per shape, with the workspace bytes of the header's formula and the instantiation (states per thread, threads).
The last shape is Al-Baqarah's 14,403 tokens over 2.5 hours (112,500 frames)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

GRID = [(2000, 383), (10000, 2047), (20000, 4095), (40000, 8191), (56250, 14403), (112500, 14403)]
SMALL = [(2000, 383), (4000, 2047), (9000, 4095)]
MAX_SAMPLES = 979200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="three small shapes only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import align_long_ref as A
    import long_ref as L
    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=False, max_batch=1, max_samples=MAX_SAMPLES)
    g = torch.Generator(device="cuda").manual_seed(11)
    for T, n_tok in (SMALL if args.small else GRID):
        n = (T - 1) * L.HOP + 640
        plan = L.plan(n, MAX_SAMPLES)
        ids = ((np.arange(n_tok) * 37 + 11) % 1024).astype(np.int64)
        path = torch.from_numpy(ids).cuda()[(torch.arange(T, device="cuda") * n_tok) // T]
        lp = torch.randn((T, 1025), generator=g, device="cuda") - 9.0
        lp[torch.arange(T, device="cuda"), path] += 8.5
        idx = torch.arange(plan.n_windows, device="cuda")[:, None] * plan.h + torch.arange(plan.kw + 1, device="cuda")[None, :]
        cut = lp[idx.clamp_(max=T - 1)].contiguous()          # (frames past the end of the last window: never read)
        want_first = -(-(np.arange(n_tok) * T) // n_tok)      # the first frame t with t * L // T == i
        eng.profile_stages(False)
        info, first, last, logp = eng.align_windows_raw(cut, [n], [ids])     # warm-up: workspace allocation, code load
        assert int(info[0]["flags"]) == 0 and int(info[0]["t_frames"]) == T and int(info[0]["n_windows"]) == plan.n_windows
        assert np.array_equal(first[0, :n_tok], want_first), "the planted path was not recovered"
        eng.profile_stages(True)
        keep, align, call = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eng.align_windows_raw(cut, [n], [ids])
            call.append((time.perf_counter() - t0) * 1e3)
            ms = eng.align_long_kernel_times()
            keep.append(ms["keep"])
            align.append(ms["align"])
        dst = torch.empty_like(lp)
        d2d = []
        for _ in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(lp)
            e1.record()
            torch.cuda.synchronize()
            d2d.append(e0.elapsed_time(e1))
        print(json.dumps({"T": T, "L": n_tok, "S": 2 * n_tok + 1, "states_per_thread": A.ns_of(n_tok), "threads": A.threads_of(n_tok),
                          "n_windows": plan.n_windows, "workspace_bytes": A.workspace_bytes([T], [n_tok]),
                          "keep_ms": round(min(keep), 4), "d2d_ms": round(min(d2d[1:]), 4), "kept_bytes": T * 4100,
                          "keep_GBps": round(2 * T * 4100 / min(keep) / 1e6, 1), "d2d_GBps": round(2 * T * 4100 / min(d2d[1:]) / 1e6, 1),
                          "align_ms": round(min(align), 3), "us_per_frame": round(min(align) * 1e3 / T, 4),
                          "call_ms": round(min(call), 3), "reps": args.reps}), flush=True)
        del lp, cut, dst
    eng.close()


if __name__ == "__main__":
    main()
