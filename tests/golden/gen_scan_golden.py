"""Fixture for the exhaustive CTC scan's ordering: the UNMODIFIED reference's brute-force scorer
(experiments/ctc-alignment/ctc_scorer.py::score_candidates) on one seeded clip.

Run ONLY in the build container (needs the reference checkout ref_import.py points at):

    python tests/golden/gen_scan_golden.py

Writes tests/golden/scan_bruteforce.npz: "logits" float32 [1, 24, 1025] (seeded noise, the greedy path of surah 112 ayah 1
boosted), and the list score_candidates returned, best first, as "verse" / "span" (the key of every candidate) and "score"
float64 (loss / L, +inf = the scorer's infeasible sentinel).  The candidates are every non-empty key of surahs 1 and 112-114,
spans 1..6, in ascending key order; tokenize_fn hands the scorer the shipped table's token list of the key.
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(ROOT))

from ref_import import REF  # noqa: E402

T, VOCAB, BLANK = 24, 1025, 1024
SURAHS = (1, 112, 113, 114)


def main():
    spec = importlib.util.spec_from_file_location("_ctc_scorer_ref", str(REF / "experiments/ctc-alignment/ctc_scorer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    from offline_tarteel_amd import TABLES_PATH
    from offline_tarteel_amd.tables import Tables
    from synth import frame_path

    tables = Tables(TABLES_PATH)
    planted = tables.verse_index(112, 1)
    logits = np.random.default_rng(20261021).standard_normal((1, T, VOCAB)).astype(np.float32)
    logits[0, np.arange(T), frame_path(tables.token_ids(planted, 1), T, 2)] += np.float32(6.0)

    cands = []
    for v in range(tables.n_verses):
        if int(tables.surah[v]) not in SURAHS:
            continue
        for sp in range(1, 7):
            if len(tables.token_ids(v, sp)):
                cands.append({"text_clean": f"{v}:{sp}", "verse": v, "span": sp})

    def tokenize(text):
        v, sp = map(int, text.split(":"))
        return [int(i) for i in tables.token_ids(v, sp)]

    res = mod.score_candidates(torch.from_numpy(logits), cands, tokenize, BLANK)
    assert len(res) == len(cands) and mod._IMPOSSIBLE == float("inf")
    out = HERE / "scan_bruteforce.npz"
    np.savez_compressed(out, logits=logits, verse=np.array([c["verse"] for c, _ in res], np.int32),
                        span=np.array([c["span"] for c, _ in res], np.int32), score=np.array([s for _, s in res], np.float64))
    print(f"{out.name}: {len(res)} candidates, {sum(np.isfinite(s) for _, s in res)} feasible, best "
          f"{res[0][0]['text_clean']} {res[0][1]:.4f}, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
