"""The CPU oracle at non-default CTC_DIRECT_* knobs against the unmodified reference (tests/golden/knob_cases.json.gz):
TOP_TEXT 1 ... 127, TOP_SPAN_REFS 0 ... 128, MAX_SPAN 2 ... 6, SPAN_PENALTY 0 / 2, TEXT_WEIGHT -0.5.  The GPU tests at these
knobs (test_gpu_knobs.py) lean on the oracle for their differential fuzz, so it is pinned here first."""

import numpy as np
import pytest

import knob_cases as kc


@pytest.fixture(scope="module")
def data(golden_dir):
    return kc.load(golden_dir)


@pytest.fixture(scope="module")
def oracles(data):
    from oracle.oracle import Oracle

    return {k: Oracle(**kn) for k, kn in data["sets"].items()}


def test_fixture_set_keeps_its_conditions(data, golden_dir):
    counts = kc.check_conditions(data)
    print("K5 candidate counts of the reference:", counts)
    assert (golden_dir / "knob_cases.json.gz").stat().st_size < (golden_dir / "retrieval_cases.json.gz").stat().st_size


def test_sets_are_the_ones_the_tests_name(data):
    want = {"K1": (1, 0, 2), "K2": (3, 1, 3), "K3": (5, 80, 4), "K4": (6, 7, 5), "K5": (127, 128, 6), "K6": (100, 80, 6),
            "K7": (100, 80, 6)}
    for k, kn in data["sets"].items():
        assert (kn["top_text"], kn["top_span_refs"], kn["max_span"]) == want[k]
        assert kn["threshold"] == 0.80
        assert (kn["span_penalty"], kn["text_weight"]) == {"K6": (0.0, -0.5), "K7": (2.0, 0.0)}.get(k, (0.5, 0.0))


@pytest.mark.parametrize("set_name", ["K1", "K2", "K3", "K4", "K5", "K6", "K7"])
def test_oracle_equals_the_reference_at_knobs(data, oracles, set_name):
    orc = oracles[set_name]
    for c in kc.cases_of(data, set_name):
        tag = (set_name, c["name"])
        lp = kc.lp_of(c["recipe"]).numpy()
        assert orc.greedy_decode(lp) == c["transcript"], tag
        cs, cp, sc, m = orc.build_candidates(c["transcript"])
        # base and candidate list: exact
        s, a, e = orc.key_of(m.start, m.span)
        assert [s, a, e if m.span > 1 else None] == c["base"][:3], tag
        assert m.score == c["base"][3], tag
        keys = [list(orc.key_of(int(x), int(y))) for x, y in zip(cs, cp)]
        assert keys == c["keys"], tag
        assert sc.tolist() == c["scores"], tag
        assert (m.score < orc.threshold) == c["use_ctc"], tag
        # rerank
        win, loss, cl, fs = orc.ctc_rerank(lp, cs, cp, sc)
        if "rerank" in c:
            rr = c["rerank"]
            want = np.array([np.inf if x is None else x for x in rr["ctc_loss"]], dtype=np.float64)
            fin = np.isfinite(want)
            assert (np.isfinite(loss) == fin).all(), tag
            assert cl.tolist() == rr["ctc_len"], tag
            if fin.any():
                assert np.abs(loss[fin] - want[fin]).max() <= 1e-3, tag
                if len(cs) <= 400:     # (the reference's own F.ctc_loss call, on the short lists)
                    idl = [orc.token_ids(int(x), int(y)) for x, y, f in zip(cs, cp, fin) if f]
                    assert np.abs(orc.ctc_loss_torch(lp, idl) - want[fin]).max() <= 1e-4, tag
                wf = np.array([x for x in rr["final_score"] if x is not None])
                assert np.allclose(fs[fin], wf, atol=1e-6), tag
            assert [x is None for x in rr["final_score"]] == (~fin).tolist(), tag
        order = sorted((i for i in range(len(cs)) if np.isfinite(loss[i])), key=lambda i: -fs[i])
        assert [keys[i] for i in order[:20]] == c["ranked_keys"], tag
        assert np.allclose([fs[i] for i in order[:20]], c["ranked_final"], atol=1e-6), tag
        # decision
        res = orc.predict_logprobs(lp)
        assert [res["surah"], res["ayah"], res["ayah_end"]] == c["winner"] and res["source"] == c["source"], (tag, res)
        assert res["use_ctc"] == c["use_ctc"] and res["n_candidates"] == c["n_candidates"], tag
        if c["source"] == "text":
            assert res["score_raw"] == c["winner_score_raw"], tag
        else:
            assert abs(res["score_raw"] - c["winner_score_raw"]) <= 1e-6, tag


@pytest.mark.parametrize("field", kc.FIELDS)
def test_an_oracle_that_ignored_one_knob_would_fail(data, field):
    """Every knob on its own: with `field` put back to its default and the rest of the set kept, the oracle's candidate
    list or decision leaves the reference's for at least one case -- so the comparison above (and the device's against
    the same fixtures) holds every knob, not just their combination."""
    from oracle.oracle import Oracle

    orcs = {}
    for c in data["cases"]:
        if c["knobs"][field] == kc.DEFAULTS[field]:
            continue
        if c["set"] not in orcs:
            orcs[c["set"]] = Oracle(**{**c["knobs"], field: kc.DEFAULTS[field]})
        orc = orcs[c["set"]]
        cs, cp, sc, m = orc.build_candidates(c["transcript"])
        keys = [list(orc.key_of(int(x), int(y))) for x, y in zip(cs, cp)]
        if keys != c["keys"]:
            return
        res = orc.predict_logprobs(kc.lp_of(c["recipe"]).numpy())
        if ([res["surah"], res["ayah"], res["ayah_end"]], res["source"]) != (c["winner"], c["source"]):
            return
    pytest.fail(f"no case of the fixture set depends on {field}")


def test_clipped_winner_is_defined_by_the_fixture(data):
    """The device clips a list at 2,048 candidates; the reference does not.  For the clipped cases the expected device
    winner is derived from the fixture's own per-candidate final scores (knob_cases.capped_winner); here: that the
    derivation gives the reference's winner back when nothing is cut off."""
    checked = 0
    for c in data["cases"]:
        if "rerank" not in c or not c["ranked_keys"] or c["n_candidates"] > kc.CAND_CAP:
            continue
        w, score = kc.capped_winner(c)
        assert c["keys"][w] == c["ranked_keys"][0], (c["set"], c["name"])
        if c["use_ctc"]:
            assert score == c["winner_score_raw"], (c["set"], c["name"])
        checked += 1
    assert checked >= 40
