#!/usr/bin/env python
"""Cost of transcription with confidence (qv_transcribe / qv_transcribe_batch) next to the path it replaces, in one process.

    python tools/transcribe_bench.py [--rows 64] [--steps 50] [--trials 7] [--out FILE]

Two shapes: `rows` chunks of 3 s (38 encoder frames) -- the streaming row's batch -- and `rows` clips of 10 s (126 frames).

  post-logits, log-probs resident in HBM (verse-shaped: random token paths at two frames per token, boost 12 over unit
  noise, float32 log-softmax):
    new   qv_transcribe at the C ABI on arrays built once, plus the per-row id lists (ids[b, :n].tolist())
    old   what Engine.transcribe_batch(confidence=False) does behind the forward: torch.argmax over [B, T, 1025], the
          [B, T] int64 copy to the host, the per-row collapse in numpy -- id lists only, no confidence figure
  end to end, seeded random weights (Engine.transcribe_batch on device-resident audio, forward included):
    confidence=True against confidence=False

Every figure is host wall-clock per call around work that ends in a device synchronise (both paths are synchronous).  A trial
times `steps` calls of ONE variant; the variants alternate within a trial round, `trials` rounds; reported are the median
over the rounds and their minimum and maximum (the spread).  Every variant is warmed up at its shape first.  The id lists
of old and new are compared before anything is timed.  One JSON line; --out also writes it to a file.
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import TRANSCRIPT_INFO_DTYPE, Engine
    from synth import synth_audio

    B = args.rows
    shapes = {"3s": 48000, "10s": 160000}
    eng = Engine(device=0, with_model=True, max_batch=B, max_samples=max(shapes.values()))
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

    out = {"rows": B, "steps": args.steps, "trials": args.trials, "shapes": {}}
    gen = torch.Generator(device="cpu").manual_seed(20260630)
    for tag, n_samples in shapes.items():
        T = eng.frames_for(n_samples)
        # verse-shaped log-probs: T // 2 random tokens at two frames each (equal neighbours collapse, as they would)
        lg = torch.randn((B, T, 1025), generator=gen)
        path = torch.randint(0, 1024, (B, (T + 1) // 2), generator=gen).repeat_interleave(2, dim=1)[:, :T]
        lg.scatter_add_(2, path.unsqueeze(-1), torch.full((B, T, 1), 12.0))
        lp = torch.log_softmax(lg, -1).cuda().contiguous()
        frames = np.full(B, T, np.int32)
        info = np.zeros(B, TRANSCRIPT_INFO_DTYPE)
        ids = np.zeros((B, T), np.int32)
        logp = np.zeros((B, T), np.float32)
        first, last = np.zeros((B, T), np.int16), np.zeros((B, T), np.int16)
        lp_ptr = C.c_void_p(lp.data_ptr())

        def new():
            rc = eng.lib.qv_transcribe(eng.h, lp_ptr, p(frames), B, T, p(info), p(ids), p(logp), p(first), p(last), T, None)
            assert rc == 0
            return [ids[b, : int(info[b]["n_tokens"])].tolist() for b in range(B)]

        def old():
            am = lp.argmax(-1).cpu().numpy()
            res = []
            for b in range(B):
                row = am[b, :T]
                keep = np.ones(T, bool)
                keep[1:] = row[1:] != row[:-1]
                res.append(row[keep & (row != 1024)].tolist())
            return res

        assert new() == old()
        audio = torch.from_numpy(np.ascontiguousarray(synth_audio(B, n_samples), np.float32)).cuda()
        lengths = [n_samples] * B
        with_conf = eng.transcribe_batch(audio, lengths, confidence=True)
        assert [d["text"] for d in with_conf] == eng.transcribe_batch(audio, lengths)
        res = spread({"qv_transcribe": new, "argmax_copy_collapse": old})
        res.update(spread({"transcribe_batch_confidence": lambda: eng.transcribe_batch(audio, lengths, confidence=True),
                           "transcribe_batch_plain": lambda: eng.transcribe_batch(audio, lengths)}))
        res["frames"] = T
        res["mean_tokens"] = round(float(info["n_tokens"].mean()), 1)
        res["record_bytes_per_call"] = B * (40 + 12 * ((T + 1) & ~1))
        res["old_copy_bytes_per_call"] = B * T * 8
        out["shapes"][tag] = res
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
