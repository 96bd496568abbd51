"""Reader of tests/golden/knob_cases.json.gz (the reference at non-default CTC_DIRECT_* knobs, written by
tests/golden/gen_golden.py knobs) shared by test_oracle_knobs.py and test_gpu_knobs.py, and the conditions the fixture
set has to keep meeting when it is regenerated."""

from __future__ import annotations

import gzip
import hashlib
import json

import numpy as np
import torch

from synth import synth_logits

CAND_CAP = 2048      # QV_CAND_CAP (csrc/qv_common.h): the device clips a candidate list there, the reference has no cap
DEFAULTS = {"top_text": 100, "top_span_refs": 80, "max_span": 6, "threshold": 0.80, "text_weight": 0.0,
            "span_penalty": 0.5}
FIELDS = ("top_text", "top_span_refs", "max_span", "span_penalty", "text_weight")


def lp_of(recipe) -> torch.Tensor:
    lg = synth_logits(recipe["ids"], recipe["T"], seed=recipe["seed"], noise=recipe["noise"], boost=recipe["boost"],
                      rep=recipe["rep"])
    return torch.log_softmax(torch.from_numpy(lg), dim=-1)


def digest(keys) -> str:
    return hashlib.sha1(json.dumps(keys, separators=(",", ":")).encode()).hexdigest()[:16]


def span_of(base) -> int:
    return 1 if base[2] is None else base[2] - base[1] + 1


def load(golden_dir) -> dict:
    """The file with every case completed: "knobs", "recipe", "transcript", "keys" ([surah, ayah, ayah_end] per
    candidate, in order) and "scores" (their text scores); K7's list is K6's (the generator checked that)."""
    from oracle.oracle import DEFAULT_TABLES, read_blob

    tables = read_blob(DEFAULT_TABLES)
    surah, ayah = tables["surah"], tables["ayah"]
    data = json.load(gzip.open(golden_dir / "knob_cases.json.gz"))
    by = {(c["set"], c["name"]): c for c in data["cases"]}
    for c in data["cases"]:
        src = by[(c["cand_of"], c["name"])]["cand"] if "cand_of" in c else c["cand"]
        start = np.cumsum(src["start_delta"], dtype=np.int64)      # first verse of each candidate, index in mushaf order
        c["keys"] = [[int(surah[v]), int(ayah[v]), int(ayah[v]) + n - 1] for v, n in zip(start, src["span"])]
        c["scores"] = src["score"]
        c["knobs"] = data["sets"][c["set"]]
        c["recipe"] = data["recipes"][c["name"]]["recipe"]
        c["transcript"] = data["recipes"][c["name"]]["transcript"]
        assert len(c["keys"]) == len(c["scores"]) == c["n_candidates"]
        if "rerank" in c:       # losses are stored in their shortest float32 spelling
            c["rerank"]["ctc_loss"] = [None if x is None else float(np.float32(x)) for x in c["rerank"]["ctc_loss"]]
    return data


def cases_of(data, set_name) -> list[dict]:
    return [c for c in data["cases"] if c["set"] == set_name]


def capped_winner(c):
    """What a device that clips the list at CAND_CAP has to answer when the rerank runs: the first maximum of the
    reference's own final_score over the first CAND_CAP candidates with a finite loss (a stable descending sort's head,
    c2c-direct/run.py:378-379).  Returns (candidate index, exp(-norm_loss) from the reference's float32 loss), or None
    when none of them is feasible.  Needs the case's "rerank" vectors."""
    fin = c["rerank"]["final_score"][:CAND_CAP]
    idx = [i for i, f in enumerate(fin) if f is not None]
    if not idx:
        return None
    w = max(idx, key=lambda i: (fin[i], -i))
    norm = np.float32(c["rerank"]["ctc_loss"][w]) / np.float32(c["rerank"]["ctc_len"][w])
    return w, float(np.exp(-np.float64(norm)))


def check_conditions(data) -> dict:
    """The properties the cases were chosen for; returns the K5 candidate counts."""
    sets, cases, defaults = data["sets"], data["cases"], data["defaults"]
    assert set(sets) == {"K1", "K2", "K3", "K4", "K5", "K6", "K7"}
    names = set(data["recipes"])
    assert len(names) >= 14 and all({c["name"] for c in cases_of(data, k)} == names for k in sets)
    # every max_span has a base that uses it up and one that does not
    for m in range(2, 7):
        at_m = [c for c in cases if c["knobs"]["max_span"] == m]
        assert any(span_of(c["base"]) == m for c in at_m), m
        assert any(span_of(c["base"]) < m for c in at_m), m
    # a smaller max_span changes a base
    assert any(c["base"][:3] != defaults[c["name"]]["base"][:3] for c in cases if c["knobs"]["max_span"] < 6)
    # every knob moves an outcome
    for field in FIELDS:
        moved = [c for c in cases if c["knobs"][field] != DEFAULTS[field]]
        assert any(digest(c["keys"]) != defaults[c["name"]]["cand_digest"] or
                   (c["winner"], c["source"]) != (defaults[c["name"]]["winner"], defaults[c["name"]]["source"])
                   for c in moved), field
    # K5 reaches the device's candidate cap from both sides
    counts = {c["name"]: c["n_candidates"] for c in cases_of(data, "K5")}
    over = [n for n in counts.values() if n > CAND_CAP]
    assert len(over) >= 3, counts
    assert any(n <= CAND_CAP + 100 for n in over), counts
    assert any(CAND_CAP - 100 <= n <= CAND_CAP for n in counts.values()), counts
    # the clipped cases can be judged: their per-candidate vectors are there
    assert sum("rerank" in c for c in cases_of(data, "K5") if c["n_candidates"] > CAND_CAP) >= 3
    return counts
