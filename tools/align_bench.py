#!/usr/bin/env python
"""Cost of the device forced alignment (qv_align) next to the nearest existing kernel, the CTC loss recursion
(qv_debug_ctc_loss: the same recursion with transcendentals, one wave per target), in one process.

    python tools/align_bench.py [--steps 200] [--rows 64]

For (T, L) = (126, 40) and (376, 120): `rows` planted-path log-prob matrices (tests/synth.py, noise 1.0, boost 12.0,
two frames per token), one target each.  qv_align aligns row b to target b; qv_debug_ctc_loss scores the same targets
against row 0 (it takes one matrix).  Both calls are synchronous and timed at the C ABI, so the figure is host wall-clock
per call, upload of the targets and copy-back of the results included (qv_debug_ctc_loss also allocates its staging
buffers per call); for kernel time alone run it under `rocprofv3 --kernel-trace --stats` (k_align / k_ctc_debug).  One JSON line per shape,
with the alignment workspace the engine allocated.
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
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import ALIGN_INFO_DTYPE, Engine
    from synth import synth_logits

    B = args.rows
    eng = Engine(device=0, with_model=False, max_batch=B, max_samples=480000)
    t_cap = eng.frames_for(480000) + 2
    for T, L in ((126, 40), (376, 120)):
        targets, rows = [], []
        for b in range(B):
            ids = ((np.arange(L) * 37 + 11 + 5 * b) % 1024).astype(np.int64)
            targets.append(ids)
            lg = synth_logits(ids.tolist(), T, seed=7000 + b, noise=1.0, boost=12.0, rep=2)
            rows.append(torch.log_softmax(torch.from_numpy(lg), -1))
        lp = torch.stack(rows).cuda().contiguous()
        lp0 = lp[0].contiguous()
        al = eng.align(lp, [T] * B, targets)                       # warm-up (first call: workspace allocation, code load)
        assert all(a["flags"] == 0 and a["first"].tolist() == (np.arange(L) * 3).tolist() for a in al)
        eng.debug_ctc_loss(lp0, targets)
        # the timed calls go straight to the C ABI on arrays built once: no Python result assembly in the figure
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        tg = np.ascontiguousarray(np.concatenate(targets).astype(np.uint16))
        lens, t = np.full(B, L, np.int32), np.full(B, T, np.int32)
        info = np.zeros(B, dtype=ALIGN_INFO_DTYPE)
        first, last = np.zeros((B, 383), np.int16), np.zeros((B, 383), np.int16)
        logp, loss = np.zeros((B, 383), np.float32), np.zeros(B, np.float32)
        stream = eng._stream()

        def align():
            assert eng.lib.qv_align(eng.h, C.c_void_p(lp.data_ptr()), p(t), B, T, p(tg), p(lens), p(info), p(first), p(last),
                                    p(logp), 383, stream) == 0

        def ctc_loss():
            assert eng.lib.qv_debug_ctc_loss(eng.h, C.c_void_p(lp0.data_ptr()), T, p(tg), p(lens), B, p(loss), stream) == 0

        torch.cuda.synchronize()
        ms = {}
        for name, fn in (("align", align), ("ctc_loss", ctc_loss), ("align_again", align), ("ctc_loss_again", ctc_loss)):
            fn()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            ms[name] = (time.perf_counter() - t0) * 1e3 / args.steps
        assert first[:, :L].tolist() == [(np.arange(L) * 3).tolist()] * B and np.isfinite(loss).all()
        print(json.dumps({"T": T, "L": L, "rows": B, "steps": args.steps,
                          "qv_align_ms_per_call": round(min(ms["align"], ms["align_again"]), 4),
                          "qv_align_ms_per_call_runs": [round(ms["align"], 4), round(ms["align_again"], 4)],
                          "qv_debug_ctc_loss_ms_per_call": round(min(ms["ctc_loss"], ms["ctc_loss_again"]), 4),
                          "qv_debug_ctc_loss_ms_per_call_runs": [round(ms["ctc_loss"], 4), round(ms["ctc_loss_again"], 4)],
                          "state_steps": B * T * (2 * L + 1),
                          "align_workspace_bytes": B * (t_cap * 256 + 3872 + 792)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
