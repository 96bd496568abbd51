"""Ranked alternatives, host side (no GPU): the restatement the GPU tests compare the device with (tests/nbest_ref.py)
against the reference's own rankings, the plugin's "candidates" shaping, and the exported ABI."""

import ctypes
import gzip
import json
import re

import numpy as np
import pytest

import knob_cases as kc
import nbest_ref


@pytest.fixture(scope="module")
def knob_data(golden_dir):
    return kc.load(golden_dir)


@pytest.fixture(scope="module")
def e2e_cases(golden_dir):
    return json.load(gzip.open(golden_dir / "e2e_cases.json.gz"))


def test_restatement_reproduces_the_reference_rankings(knob_data):
    """every knob case that carries the reference's whole final_score vector: the stable ranking's first 20 are the
    reference's ranked_keys / ranked_final, exactly.  10 of the 71 rankings hold exact ties (6 of them within the first 20
    ranks): always one token list scored under two keys (2:1 / 3:1, ...), kept in candidate order"""
    import offline_tarteel_amd
    from offline_tarteel_amd.tables import Tables

    tb = Tables(offline_tarteel_amd.TABLES_PATH)
    checked = with_ties = in_top20 = 0
    for c in knob_data["cases"]:
        if "rerank" not in c:
            continue
        fin = c["rerank"]["final_score"]
        assert [f is None for f in fin] == [l is None for l in c["rerank"]["ctc_loss"]]
        order = nbest_ref.rank(fin)
        assert order == nbest_ref.rank(fin, c["rerank"]["ctc_loss"])
        top = order[:20]
        assert [c["keys"][i] for i in top] == c["ranked_keys"], (c["set"], c["name"])
        assert [fin[i] for i in top] == c["ranked_final"], (c["set"], c["name"])
        ties = [(a, b) for a, b in zip(order, order[1:]) if fin[a] == fin[b]]
        for a, b in ties:        # a tie is kept in candidate order, and comes from one token list scored twice
            assert a < b
            (s1, a1, e1), (s2, a2, e2) = c["keys"][a], c["keys"][b]
            assert tb.token_ids(tb.verse_index(s1, a1), e1 - a1 + 1).tolist() == tb.token_ids(tb.verse_index(s2, a2), e2 - a2 + 1).tolist()
        with_ties += bool(ties)
        in_top20 += any(a in top and b in top for a, b in ties)
        checked += 1
    assert (checked, with_ties, in_top20) == (71, 10, 6)


def test_selection_rules_on_hand_written_rows():
    inf, nan = float("inf"), float("nan")
    assert nbest_ref.select([1.0, 3.0, 2.0], [0.0, 0.0, 0.0], 2) == [1, 2]
    assert nbest_ref.select([1.0, 1.0, 1.0, 1.0], [0.0] * 4, 3) == [0, 1, 2]                 # ties: candidate order
    assert nbest_ref.select([0.0, -0.0, 0.0, -0.0], [0.0] * 4, 4) == [0, 1, 2, 3]            # -0.0 == +0.0
    assert nbest_ref.select([5.0, 4.0, 3.0], [inf, 1.0, inf], 5) == [1]                      # infinite loss: not ranked
    assert nbest_ref.select([5.0, 4.0], [inf, inf], 5) == [] and nbest_ref.select([], [], 5) == []
    assert nbest_ref.select([1.0, 2.0], [nan, 0.0], 5) == [1]
    # the text rows
    assert nbest_ref.text_row(7, 1, 0.9, [7, 3, 5], [0.9, 0.5, 0.4], k=5) == [{"start": 7, "span": 1, "score": 0.9}]
    assert [e["start"] for e in nbest_ref.text_row(7, 1, 0.9, [7, 3, 5], [0.9, 0.5, 0.4], k=5, runners=True)] == [7, 3, 5]
    assert [e["start"] for e in nbest_ref.text_row(7, 2, 0.9, [7, 3, 5], [0.6, 0.5, 0.4], k=3, runners=True)] == [7, 7, 3]
    # near-tie groups
    same = lambda i, j: (i, j) == (3, 4)  # noqa: E731
    assert nbest_ref.tie_groups([5.0, 4.0, 3.9995, 2.0, 2.0, 1.0, 1.0], same) == [0, 1, 1, 2, 3, 4, 4]


def test_candidates_shaping_on_the_e2e_fixtures(e2e_cases):
    """the plugin's "candidates" from an engine-shaped n-best list equal the reference's: ranked[:5] with
    round(final_score, 4) where the rerank decided, [result] where the text match did, [] for an empty prediction"""
    from offline_tarteel_amd import plugin

    seen = set()
    for c in e2e_cases:
        g = c["result"]
        if not g["surah"]:
            want, nbest = [], []
        elif g["source"] == "ctc":
            # the engine's list: every feasible candidate's final from the fixture's float32 losses, ranked
            fin = [None if l is None else nbest_ref.reference_final(l, n, span=k[2] - k[1] + 1)
                   for l, n, k in zip(c["ctc_loss"], c["ctc_len"], c["cand_keys"])]
            order = nbest_ref.rank(fin)
            assert [c["cand_keys"][i] for i in order[:20]] == c["ranked_keys"] and [fin[i] for i in order[:20]] == c["ranked_final"], c["name"]
            nbest = [{"surah": c["cand_keys"][i][0], "ayah": c["cand_keys"][i][1], "ayah_end": c["cand_keys"][i][2], "score": fin[i],
                      "source": "ctc"} for i in order[:5]]
            want = [{"surah": k[0], "ayah": k[1], "ayah_end": k[2], "score": round(f, 4)}
                    for k, f in zip(c["ranked_keys"][:5], c["ranked_final"][:5])]
            assert (want[0]["surah"], want[0]["ayah"], want[0]["ayah_end"]) == (g["surah"], g["ayah"], g["ayah_end"])
        else:
            b = c["base"]
            nbest = [{"surah": b[0], "ayah": b[1], "ayah_end": b[2] or b[1], "score": b[3], "source": "text"}]
            want = [{"surah": g["surah"], "ayah": g["ayah"], "ayah_end": g["ayah_end"], "score": g["score"]}]
        seen.add(g["source"])
        assert plugin.shape_candidates(nbest) == want == nbest_ref.shape_candidates(nbest), c["name"]
        raw = {"surah": g["surah"], "ayah": g["ayah"], "ayah_end": g["ayah_end"], "score": g.get("score_raw", 0.0),
               "source": g["source"], "transcript": c["transcript"], "nbest": nbest}
        d = plugin._finish(None, [raw], True, False, candidates=5)[0]
        assert d["candidates"] == want, c["name"]
        plain = plugin._finish(None, [raw], True, False)[0]
        assert ("candidates" in plain) == (not g["surah"]) and {k: v for k, v in d.items() if k != "candidates"} == {
            k: v for k, v in plain.items() if k != "candidates"}
    assert seen == {None, "text", "ctc"}


def test_nbest_symbols_are_exported_and_bound():
    import offline_tarteel_amd
    from offline_tarteel_amd import engine as E

    assert {"qv_nbest_results_ctx", "qv_nbest_select"} <= set(E.exported_symbols())
    h = ctypes.CDLL(str(offline_tarteel_amd.LIB_PATH))
    assert hasattr(h, "qv_nbest_results_ctx") and hasattr(h, "qv_nbest_select")
    hdr = (offline_tarteel_amd.LIB_PATH.parent.parent / "include" / "qverse.h").read_text()
    assert f"#define QV_NBEST_MAX {E.NBEST_MAX}" in hdr and E.NBEST_MAX == nbest_ref.NBEST_MAX
    assert f"QV_NBEST_TEXT_RUNNERS = {E.NBEST_TEXT_RUNNERS}" in hdr
    # the structures, field for field in the header's order
    for name, cls, dt in (("qv_nbest_entry", E.QvNbestEntry, E.NBEST_ENTRY_DTYPE), ("qv_nbest_info", E.QvNbestInfo, E.NBEST_INFO_DTYPE)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            words = decl.replace(",", " ").split()
            if words:
                fields += [(w, words[0]) for w in words[1:]]
        ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float}
        assert [(n, ctype[t]) for n, t in fields] == list(cls._fields_), name
        assert list(dt.names) == [n for n, _ in fields] and dt.itemsize == ctypes.sizeof(cls)
        assert all(dt.fields[n][1] == getattr(cls, n).offset for n in dt.names)
    # the argument lists the loader sets, against the header's prototypes
    lib = E.load_library()
    for fn in ("qv_nbest_results_ctx", "qv_nbest_select"):
        proto = re.search(r"\bint " + fn + r"\s*\(([^;]*)\);", hdr).group(1)
        params = [re.sub(r"/\*.*?\*/", "", p, flags=re.S).strip() for p in proto.split(",")]
        want = [ctypes.c_void_p if "*" in p else {"int32_t": ctypes.c_int32}[p.split()[0]] for p in params]
        assert list(getattr(lib, fn).argtypes) == want, fn
