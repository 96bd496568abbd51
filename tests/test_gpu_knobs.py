"""The HIP post-logits path away from its default configuration (GPU): the reference's own outcomes at seven settings of
TOP_TEXT / TOP_SPAN_REFS / MAX_SPAN / SPAN_PENALTY / TEXT_WEIGHT (tests/golden/knob_cases.json.gz), the clip of the
candidate list at QV_CAND_CAP, the gate's threshold at its edges, literal mode (skip_unused_passes = 0), the
2,048-character kernel set at three of the settings, a differential fuzz against the oracle at five, and qv_create's
range checks."""

import gzip
import json
import math

import numpy as np
import pytest
import torch

import knob_cases as kc

pytestmark = pytest.mark.gpu

SETS = ["K1", "K2", "K3", "K4", "K5", "K6", "K7"]
WIDE_SETS = ["K1", "K4", "K5"]
CONFIGS = [(k, False) for k in SETS] + [(k, True) for k in WIDE_SETS]
CONFIG_IDS = [k + ("-wide" if w else "") for k, w in CONFIGS]
FORCE_CTC = math.nextafter(1.0, 2.0)      # no text score reaches it: the gate fails for every utterance


@pytest.fixture(scope="module")
def data(golden_dir):
    return kc.load(golden_dir)


@pytest.fixture(scope="module")
def e2e_cases(golden_dir):
    return json.load(gzip.open(golden_dir / "e2e_cases.json.gz"))


@pytest.fixture(scope="module")
def engines(data):
    """one engine per (knob set, kernel set), made on first use and kept for the module"""
    from offline_tarteel_amd.engine import Engine

    made = {}

    def get(set_name, wide=False):
        if (set_name, wide) not in made:
            made[(set_name, wide)] = Engine(device=0, with_model=False, max_batch=32,
                                            max_transcript=2048 if wide else 1024, **data["sets"][set_name])
        return made[(set_name, wide)]

    yield get
    for e in made.values():
        e.close()


def make_engine(**kw):
    from offline_tarteel_amd.engine import Engine

    return Engine(device=0, with_model=False, max_batch=32, **kw)


def run_batch(eng, lps):
    """log-prob matrices of different lengths as ONE ragged batch"""
    t_max = max(x.shape[0] for x in lps)
    batch = torch.full((len(lps), t_max, 1025), -50.0)
    for b, x in enumerate(lps):
        batch[b, : x.shape[0]] = x
    assert t_max <= 376 and len(lps) <= 32
    return eng.decode_retrieve_rerank(batch.cuda().contiguous(), [x.shape[0] for x in lps])


def rerank_expectation(c):
    """(key, exp(-norm_loss), clipped) of the candidate a rerank of case c's list has to pick on the device."""
    n = c["n_candidates"]
    if not c["ranked_keys"]:
        return None, 0.0, n > kc.CAND_CAP
    if n > kc.CAND_CAP and "rerank" in c:
        w, score = kc.capped_winner(c)
        return c["keys"][w], score, True
    # the first maximum of the whole list is the first maximum of any prefix that holds it
    i = c["keys"].index(c["ranked_keys"][0])
    assert i < kc.CAND_CAP, ("the fixture must carry the rerank vectors of this case", c["set"], c["name"])
    kn, span = c["knobs"], c["ranked_keys"][0][2] - c["ranked_keys"][0][1] + 1
    norm = -c["ranked_final"][0] + kn["text_weight"] * c["scores"][i] - kn["span_penalty"] * (span - 1)
    return c["ranked_keys"][0], math.exp(-norm), n > kc.CAND_CAP


def check_rows(cases, rows, forced=False):
    """rows of a batched call against their fixtures; forced: the engine's threshold makes every row rerank"""
    for c, r in zip(cases, rows):
        tag = (c["set"], c["name"])
        assert r["transcript"] == c["transcript"], tag
        n = c["n_candidates"]
        use_ctc = True if forced else c["use_ctc"]
        assert r["use_ctc"] == use_ctc, tag
        assert r["base_score"] == c["base"][3], tag
        key, score, clipped = rerank_expectation(c) if use_ctc else (None, 0.0, False)
        if use_ctc and key is not None:
            if clipped:
                print(f"{tag}: reference list of {n} clipped at {kc.CAND_CAP}; winner of the clipped list {key}, of the "
                      f"reference's whole list {c['ranked_keys'][0]}" + (" (differs)" if key != c["ranked_keys"][0] else ""))
            assert ([r["surah"], r["ayah"], r["ayah_end"]], r["source"]) == (key, "ctc"), (tag, r)
            assert abs(r["score"] - score) <= 1e-3 * max(score, 1e-3), (tag, r["score"], score)
        else:       # the gate passed, or no candidate can be aligned: the text match stands
            b = c["base"]
            assert ([r["surah"], r["ayah"], r["ayah_end"]], r["source"]) == ([b[0], b[1], b[2] or b[1]], "text"), (tag, r)
            assert r["score"] == b[3], tag
        # include/qverse.h: candidates scored by the rerank, 0 if the gate passed
        assert r["n_candidates"] == (min(n, kc.CAND_CAP) if use_ctc else 0), (tag, r["n_candidates"], n)
        assert bool(r["flags"] & 8) == (use_ctc and n > kc.CAND_CAP), (tag, r["flags"], n)


@pytest.mark.parametrize("set_name,wide", CONFIGS, ids=CONFIG_IDS)
def test_retrieval_at_knobs(data, engines, set_name, wide):
    """match_verse and the candidate assembly, one transcript at a time: base and score exact, the candidate list the
    reference's (its first 2,048 entries when it is longer), text scores bit for bit."""
    eng = engines(set_name, wide)
    tb = eng.tables
    for c in kc.cases_of(data, set_name):
        tag = (set_name, c["name"])
        r = eng.debug_retrieve(c["transcript"])
        s, a, e = tb.key_of(r["base_start"], r["base_span"])
        assert [s, a, e if r["base_span"] > 1 else None] == c["base"][:3], tag
        assert r["base_score"] == c["base"][3], tag
        keys = [list(tb.key_of(int(x), int(y))) for x, y in zip(r["cand_start"], r["cand_span"])]
        assert len(keys) == min(c["n_candidates"], kc.CAND_CAP), (tag, len(keys))
        assert keys == c["keys"][: kc.CAND_CAP], tag
        assert r["cand_score"].tolist() == c["scores"][: kc.CAND_CAP], tag


@pytest.mark.parametrize("set_name,wide", CONFIGS, ids=CONFIG_IDS)
def test_batched_decision_at_knobs(data, engines, set_name, wide):
    """every case of the set in ONE ragged batch: transcript, gate, winner, source, score, candidate count, flags"""
    cases = kc.cases_of(data, set_name)
    rows = run_batch(engines(set_name, wide), [kc.lp_of(c["recipe"]) for c in cases])
    check_rows(cases, rows)
    if set_name == "K5":
        print("K5 candidate counts:", {c["name"]: c["n_candidates"] for c in cases})
    else:
        assert all(c["n_candidates"] <= kc.CAND_CAP for c in cases)


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
def test_candidate_overflow_with_every_row_reranked(data, wide):
    """K5 with the gate closed for everyone: every list is built and scored, so QV_FLAG_CAND_OVERFLOW is set exactly for
    the cases whose reference list is longer than 2,048 -- gate-pass cases of the 0.80 threshold included -- the count is
    min(len, 2048), and the winner is the first maximum of the reference's final scores over the first 2,048."""
    cases = kc.cases_of(data, "K5")
    eng = make_engine(max_transcript=2048 if wide else 1024, **{**data["sets"]["K5"], "threshold": FORCE_CTC})
    try:
        rows = run_batch(eng, [kc.lp_of(c["recipe"]) for c in cases])
    finally:
        eng.close()
    check_rows(cases, rows, forced=True)
    over = {c["name"] for c, r in zip(cases, rows) if r["flags"] & 8}
    assert over == {c["name"] for c in cases if c["n_candidates"] > kc.CAND_CAP} and len(over) >= 3


def test_threshold_edges(e2e_cases):
    """The gate `base.score < threshold` at 1.0 + 1 ulp (everything reranks: the winner is the head of the reference's
    ranking, recorded for gate-pass cases too), at 1.0 (a perfect text match still passes) and at 0.0 (nothing fails)."""
    lps = [kc.lp_of(c["recipe"]) for c in e2e_cases]
    rows = {}
    for th in (FORCE_CTC, 1.0, 0.0):
        eng = make_engine(threshold=th)
        try:
            rows[th] = run_batch(eng, lps)
        finally:
            eng.close()
    checked = perfect = 0
    for i, c in enumerate(e2e_cases):
        if "cand_keys" not in c:
            assert all(rows[th][i]["surah"] == 0 and not rows[th][i]["use_ctc"] for th in rows), c["name"]
            continue
        base, top = c["base"], c["ranked_keys"]
        base_key = [base[0], base[1], base[2] or base[1]]
        r = rows[FORCE_CTC][i]
        assert r["use_ctc"] and r["n_candidates"] == c["n_candidates"], c["name"]
        if top:
            # (finals within 2e-3 of each other may swap below the head of the ranking, never at it)
            assert ([r["surah"], r["ayah"], r["ayah_end"]], r["source"]) == (top[0], "ctc"), (c["name"], r)
            checked += 1
        else:
            assert ([r["surah"], r["ayah"], r["ayah_end"]], r["source"]) == (base_key, "text"), (c["name"], r)
        r = rows[1.0][i]
        assert r["use_ctc"] == (base[3] < 1.0), c["name"]
        if base[3] == 1.0:
            assert ([r["surah"], r["ayah"], r["ayah_end"]], r["source"], r["score"]) == (base_key, "text", 1.0), c["name"]
            perfect += 1
        r = rows[0.0][i]
        assert not (r["flags"] & 4) and not r["use_ctc"] and r["n_candidates"] == 0, c["name"]
        assert ([r["surah"], r["ayah"], r["ayah_end"]], r["source"], r["score"]) == (base_key, "text", base[3]), c["name"]
    assert checked == sum(1 for c in e2e_cases if c.get("ranked_keys")) and checked >= 6 and perfect >= 2


def test_literal_mode_reports_what_the_default_mode_reports(data, e2e_cases, oracle):
    """skip_unused_passes = 0 runs search() / pass 3 / the candidate assembly for gate-pass utterances as well, as the
    reference does; nothing consumes their output, so every result field -- n_candidates and flags included -- equals the
    default engine's: on the e2e fixtures, on 64 fuzz recipes, and at K5, where the unused lists overflow."""
    from test_gpu_postlogits import _fuzz_recipe

    rng = np.random.default_rng(20261018)
    batches = [[kc.lp_of(c["recipe"]) for c in e2e_cases]]
    for _ in range(2):
        batches.append([kc.lp_of(_fuzz_recipe(rng, oracle)) for _ in range(32)])
    k5 = [kc.lp_of(c["recipe"]) for c in kc.cases_of(data, "K5")]
    got = {}
    for literal in (False, True):
        eng = make_engine(skip_unused_passes=not literal)
        eng5 = make_engine(skip_unused_passes=not literal, **data["sets"]["K5"])
        try:
            got[literal] = [run_batch(eng, lps) for lps in batches] + [run_batch(eng5, k5)]
        finally:
            eng.close()
            eng5.close()
    passed = 0
    for rows_d, rows_l in zip(got[False], got[True]):
        for d, l in zip(rows_d, rows_l):
            assert d == l, (d, l)
            if d["source"] == "text" and not d["use_ctc"]:
                assert d["n_candidates"] == 0 and not (d["flags"] & 8)
                passed += 1
    assert passed >= 5       # (gate-pass rows are where the two modes do different work)


@pytest.mark.parametrize("set_name", ["K1", "K2", "K3", "K4", "K7"])
def test_fuzz_at_knobs_against_the_oracle(data, engines, set_name):
    """32 corrupted recitations per set, batched on the device, against the oracle built with the same knobs
    (pinned to the reference at these knobs by test_oracle_knobs.py); no row is left out."""
    from oracle.oracle import Oracle
    from test_gpu_postlogits import _fuzz_recipe

    orc = Oracle(**data["sets"][set_name])
    rng = np.random.default_rng(20261018 + SETS.index(set_name))
    recipes = [_fuzz_recipe(rng, orc) for _ in range(32)]
    lps = [kc.lp_of(r) for r in recipes]
    rows = run_batch(engines(set_name), lps)
    for rcp, lp, got in zip(recipes, lps, rows):
        want = orc.predict_logprobs(lp.numpy())
        tag = (set_name, rcp["seed"], len(rcp["ids"]), rcp["T"])
        assert got["greedy_ids"] == want["greedy_ids"], tag
        assert len(want["transcript"]) <= 1024, tag
        assert (got["surah"], got["ayah"], got["ayah_end"], got["source"]) == (
            want["surah"], want["ayah"], want["ayah_end"], want["source"]), (tag, got, want)
        if want["source"] is None:
            continue
        assert got["use_ctc"] == want["use_ctc"], tag
        if want["use_ctc"]:
            assert got["n_candidates"] == want["n_candidates"], tag
        if want["source"] == "text":
            assert got["score"] == want["score_raw"], tag
        else:
            assert abs(got["score"] - want["score_raw"]) <= 1e-3 * max(want["score_raw"], 1e-3), tag


def test_create_refuses_knobs_out_of_range(e2e_cases):
    from offline_tarteel_amd.engine import QvError

    for bad in ({"max_span": 1}, {"max_span": 7}, {"top_text": 0}, {"top_text": 128}, {"top_span_refs": -1},
                {"top_span_refs": 129}, {"text_weight": float("inf")}, {"text_weight": float("nan")}):
        with pytest.raises(QvError):
            make_engine(**bad)
    # ... and the refusals leave nothing behind that a valid engine trips over
    c = next(x for x in e2e_cases if x["name"] == "corrupt_103_2")
    eng = make_engine()
    try:
        r = run_batch(eng, [kc.lp_of(c["recipe"])])[0]
    finally:
        eng.close()
    g = c["result"]
    assert r["transcript"] == c["transcript"] and r["use_ctc"] == c["use_ctc"]
    assert (r["surah"], r["ayah"], r["ayah_end"], r["source"]) == (g["surah"], g["ayah"], g["ayah_end"], g["source"])
    assert abs(r["score"] - g["score_raw"]) <= 1e-3 * max(g["score_raw"], 1e-3)
