"""Fixtures for the correction rule: the UNMODIFIED reference's align_phonemes (shared/phoneme_aligner.py) on a few hundred
pairs of symbol sequences.

Run ONLY in the build container (needs the reference checkout ref_import.py points at):

    python tests/golden/gen_correction_golden.py

Writes tests/golden/correction_cases.json: per case {"name", "pred", "ref" (alphabet codes, no spaces), "alignment"
([ref symbol | null, pred symbol | null] per column) and "errors" ([type, position, expected | null, got | null] with type
1 substitution, 2 deletion, 3 insertion)}.  Random strings over 2, 3 and 40 symbols (small alphabets force ties in the DP),
lengths 1..40, and real verses of the shipped tables with random edits.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT))

from ref_import import REF  # noqa: E402

TYPES = {"substitution": 1, "deletion": 2, "insertion": 3}


def corrupt(rng, sym, n_edits, alphabet):
    out = list(sym)
    for _ in range(n_edits):
        kind = rng.integers(0, 3)
        at = int(rng.integers(0, len(out) + (kind == 2)))
        if kind == 0 and out:
            out[at] = int(rng.choice(alphabet))
        elif kind == 1 and len(out) > 1:
            del out[at]
        else:
            out.insert(at, int(rng.choice(alphabet)))
    return out


def main():
    # the module alone, by its path: the package's __init__ pulls in audio libraries this rule never touches
    import importlib.util

    spec = importlib.util.spec_from_file_location("_phoneme_aligner_ref", str(REF / "shared/phoneme_aligner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    align_phonemes = mod.align_phonemes

    from offline_tarteel_amd import TABLES_PATH
    from offline_tarteel_amd.tables import Tables

    rng = np.random.default_rng(20261020)
    pairs = []
    for size in (2, 3, 40):
        alphabet = np.arange(1, size + 1)
        for k in range(100):
            n, m = (int(x) for x in rng.integers(1, 41, 2))
            if k < 8:                                  # the corners: one symbol against many, equal lengths
                n, m = [(1, 1), (1, 40), (40, 1), (40, 40), (2, 2), (3, 2), (2, 3), (17, 16)][k]
            ref = rng.choice(alphabet, n).tolist()
            pred = rng.choice(alphabet, m).tolist() if k % 3 else corrupt(rng, ref, int(rng.integers(0, 6)), alphabet)
            pairs.append((f"a{size}-{k}", pred, ref))
    tb = Tables(TABLES_PATH)
    clean = tb.s["clean"]
    off = tb.s["clean_off"]
    for k, (s, a) in enumerate([(1, 1), (1, 2), (1, 7), (112, 1), (112, 4), (113, 2), (114, 6), (2, 1), (2, 2), (36, 1), (36, 9), (55, 13),
                                (67, 1), (78, 40), (93, 3), (94, 6), (96, 1), (97, 5), (103, 3), (108, 3), (109, 6), (110, 3)]):
        v = tb.verse_index(s, a)
        ref = [int(c) for c in clean[off[v]: off[v + 1]] if c]
        for e in (0, 1, 3, 7):
            pairs.append((f"v{s}:{a}-e{e}", corrupt(rng, ref, e, np.arange(1, 40)), ref))
    out = []
    for name, pred, ref in pairs:
        r = align_phonemes([str(x) for x in pred], [str(x) for x in ref])
        num = lambda t: None if t is None else int(t)  # noqa: E731
        out.append({"name": name, "pred": pred, "ref": ref,
                    "alignment": [[num(a), num(b)] for a, b in r["alignment"]],
                    "errors": [[TYPES[e["type"]], e["position"], num(e["expected"]), num(e["got"])] for e in r["errors"]]})
    path = HERE / "correction_cases.json"
    path.write_text(json.dumps(out, separators=(",", ":")) + "\n")
    print(len(out), "cases,", path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
