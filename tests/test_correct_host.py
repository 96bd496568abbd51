"""The correction rule on the host: the restatement (tests/correct_ref.py) against the reference's own alignments
(tests/golden/correction_cases.json, written by gen_correction_golden.py from the unmodified align_phonemes), hand-written
known answers for the word rule and for prefix mode, the caps against the shipped tables, correction.fold, and the
library's exports.  No GPU."""

import ctypes
import json
import re

import numpy as np
import pytest

import correct_ref as cr

A, B, C_, D = 5, 9, 12, 20     # four alphabet codes
TYPES = {"substitution": 1, "deletion": 2, "insertion": 3}


@pytest.fixture(scope="module")
def tables():
    from offline_tarteel_amd import TABLES_PATH
    from offline_tarteel_amd.tables import Tables

    return Tables(TABLES_PATH)


def test_restatement_reproduces_every_fixture(golden_dir):
    cases = json.load(open(golden_dir / "correction_cases.json"))
    assert len(cases) >= 300 and {c["name"].split("-")[0] for c in cases} >= {"a2", "a3", "a40"}
    assert any(c["name"].startswith("v") for c in cases)
    ties = 0
    for c in cases:
        r = cr.correct(c["pred"], c["ref"])
        align, errors = cr.reference_shape(r, c["ref"], c["pred"])
        assert align == c["alignment"], c["name"]
        assert [[TYPES[e["type"]], e["position"], e["expected"], e["got"]] for e in errors] == c["errors"], c["name"]
        assert r["info"]["distance"] == len(c["errors"]) and r["info"]["n_match"] == sum(a == b for a, b in c["alignment"])
        assert cr.correct_plain(c["pred"], c["ref"]) == r, c["name"]
        assert cr.correct_plain(c["pred"], c["ref"], True) == cr.correct(c["pred"], c["ref"], True), c["name"]
        # the fixtures exercise the tie rule: some cell of the backtrace had more than one optimal move
        last, mv = cr.moves_plain(c["ref"], c["pred"])
        ties += any(x == 0 for x in r["ops"]) and len(set(c["pred"]) | set(c["ref"])) <= 3
    assert ties >= 100


def test_tie_rule_probes():
    # ab / ba: two substitutions, not a deletion and an insertion around a match
    assert cr.correct([A, B], [B, A])["ops"] == [cr.SUB, cr.SUB]
    # pred ab against ref aab: (2,1) ties between S and D and takes S, so the FIRST a is the deleted one
    assert cr.correct([A, B], [A, A, B])["ops"] == [cr.DEL, cr.MATCH, cr.MATCH]
    # pred aab against ref ab: the insertion comes first as well
    assert cr.correct([A, A, B], [A, B])["ops"] == [cr.INS, cr.MATCH, cr.MATCH]
    # one symbol each
    assert cr.correct([A], [A])["ops"] == [cr.MATCH] and cr.correct([A], [B])["ops"] == [cr.SUB]


def test_word_rule_known_answers():
    # ref "ab cd", pred "axd": at (3, 2) sub and del tie and S wins, so x stands for c (word 1) and b is the deletion (word 0)
    r = cr.correct([A, 30, D], [A, B, 0, C_, D])
    assert r["ops"] == [0, 2, 1, 0] and r["words"] == [(2, 1, 0, 1, 0, 2), (2, 1, 1, 0, 0, 1)]
    # the first error of word 0 is a deletion, a later substitution overrides it: ref "abc d", pred "bx d"
    r = cr.correct([B, 30, 0, D], [A, B, C_, 0, D])
    assert r["ops"] == [cr.DEL, cr.MATCH, cr.SUB, cr.MATCH] and r["words"][0] == (3, 1, 1, 1, 0, cr.SUB) and r["words"][1][5] == 0
    # without a substitution the first error decides: deletion then insertion -> 2; insertion then deletion -> 3
    r = cr.correct([B, C_, 30, 31], [A, B, C_])
    assert r["ops"] == [cr.DEL, 0, 0, cr.INS, cr.INS] and r["words"] == [(3, 2, 0, 1, 2, cr.DEL)]
    # a trailing insertion (position n) goes to the last word
    r = cr.correct([A, 0, B, 30], [A, 0, B])
    assert r["ops"] == [0, 0, cr.INS] and r["positions"] == [0, 1, 2] and r["words"] == [(1, 1, 0, 0, 0, 0), (1, 1, 0, 0, 1, cr.INS)]
    # an insertion in front of a word's first symbol goes to that word: ref "a b", pred "a xb"
    r = cr.correct([A, 0, 30, B], [A, 0, B])
    assert r["ops"] == [0, cr.INS, 0] and r["words"] == [(1, 1, 0, 0, 0, 0), (1, 1, 0, 0, 1, cr.INS)]
    # runs of spaces make words without symbols; spaces of the prediction mean nothing
    r = cr.correct([0, A, 0, 0, B], [A, 0, 0, B, 0])
    assert r["info"]["n_words"] == 4 and r["words"] == [(1, 1, 0, 0, 0, 0), (0,) * 6, (1, 1, 0, 0, 0, 0), (0,) * 6]


def test_prefix_mode_known_answers():
    ref = [A, B, 0, C_, D, 0, A, C_]
    for k, touched, flags in ((0, 0, 0), (1, 1, cr.LAST_WORD_OPEN), (2, 1, 0), (3, 2, cr.LAST_WORD_OPEN), (4, 2, 0), (6, 3, 0)):
        sym = [c for c in ref if c][:k]
        if not sym:
            continue                                   # (an empty prediction is NO_TRANSCRIPT, not a prefix)
        r = cr.correct(sym, ref, prefix=True)
        assert (r["info"]["n_ref_used"], r["info"]["distance"], r["info"]["words_touched"], r["info"]["flags"]) == (k, 0, touched, flags), k
        assert r["ops"] == [0] * k and sum(w[0] for w in r["words"]) == k
        assert all(w == (0,) * 6 for w in r["words"][touched:])
    # a tie between end rows picks the smaller i: pred "ax" against ref "ab c" -- dp[1][2] = dp[2][2] = 1
    r = cr.correct([A, 30], [A, B, 0, C_], prefix=True)
    assert r["info"]["n_ref_used"] == 1 and r["ops"] == [0, cr.INS] and r["info"]["flags"] == cr.LAST_WORD_OPEN
    assert r["words"] == [(1, 1, 0, 0, 1, cr.INS), (0,) * 6] and r["info"]["words_touched"] == 1
    # ... and at a word boundary the trailing insertion belongs to the word of symbol i*, which owns no aligned symbol
    r = cr.correct([A, 30], [A, 0, B, C_], prefix=True)
    assert r["info"]["n_ref_used"] == 1 and r["info"]["flags"] == 0 and r["words"] == [(1, 1, 0, 0, 0, 0), (0, 0, 0, 0, 1, cr.INS)]
    # without the flag the same pair is aligned to the end
    r = cr.correct([A, 30], [A, B, 0, C_])
    assert r["info"]["n_ref_used"] == 3 and r["info"]["distance"] == 2
    # i* = 0: nothing of the reference was said
    r = cr.correct([30], [A, B], prefix=True)
    assert r["info"]["n_ref_used"] == 0 and r["ops"] == [cr.INS] and r["info"]["words_touched"] == 0


def test_row_flags():
    assert cr.correct([A], [])["info"]["flags"] == cr.NO_TARGET and cr.correct([], [A])["info"]["flags"] == cr.NO_TRANSCRIPT
    assert cr.correct([0], [0, 0])["info"]["flags"] == cr.NO_TARGET | cr.NO_TRANSCRIPT
    r = cr.correct([A] * 5, [A] * (cr.MAX_REF + 1))
    assert r["info"] == {**dict.fromkeys(cr.INFO_FIELDS, 0), "flags": cr.TOO_LONG} and r["ops"] == [] and r["words"] == []
    assert cr.correct([A] * 1025, [A])["info"]["flags"] == cr.TOO_LONG and cr.correct([A] * 1025, [A], max_pred=2048)["info"]["flags"] == 0
    assert cr.correct([A], [A, 0] * cr.MAX_WORDS)["info"]["flags"] == cr.TOO_LONG
    assert cr.correct([A], ([A, 0] * cr.MAX_WORDS)[:-1])["info"]["flags"] == 0


def test_caps_hold_every_span_of_the_tables(tables):
    """every (verse, span 1..6) inside one surah fits QV_CORRECT_MAX_REF and QV_CORRECT_MAX_WORDS, and the word cap is the
    smallest multiple of 32 that does; span_codes is the text the token list was built from (single-spaced, no edge spaces)"""
    s = tables.s
    clen = np.diff(s["clean_off"].astype(np.int64))
    nlen = np.diff(s["nobsm_off"].astype(np.int64))
    cw, nw = s["clean_nw"].astype(np.int64), s["nobsm_nw"].astype(np.int64)
    csym, nsym = clen - (cw - 1), nlen - np.maximum(nw - 1, 0)          # spaceless lengths
    max_sym = max_words = max_raw = 0
    for v in range(tables.n_verses):
        su = int(tables.surah[v])
        last = int(s["surah_start"][su - 1]) + int(s["surah_len"][su - 1]) - 1
        for span in range(1, 7):
            if v + span - 1 > last:
                break
            head = span > 1 and nlen[v] > 0
            sym = int((nsym[v] if head else csym[v]) + csym[v + 1: v + span].sum())
            words = int((nw[v] if head else cw[v]) + cw[v + 1: v + span].sum())
            max_sym, max_words, max_raw = max(max_sym, sym), max(max_words, words), max(max_raw, sym + words - 1)
    assert max_sym <= cr.MAX_REF and max_words <= cr.MAX_WORDS and max_raw <= cr.MAX_RAW, (max_sym, max_words, max_raw)
    assert cr.MAX_WORDS % 32 == 0 and cr.MAX_WORDS - 32 < max_words
    assert int(csym.max()) == 551                                        # 2:282, the longest single verse
    for su, ay, span in ((2, 282, 1), (5, 1, 6), (97, 1, 2), (1, 1, 2), (114, 4, 3)):
        v = tables.verse_index(su, ay)
        codes = tables.span_codes(v, span)
        sym, word, n_words = cr.strip(codes)
        assert codes[0] != 0 and codes[-1] != 0 and not ((codes[1:] == 0) & (codes[:-1] == 0)).any()
        head = span > 1 and nlen[v] > 0
        assert n_words == int((nw[v] if head else cw[v]) + cw[v + 1: v + span].sum()) and word[-1] == n_words - 1
    assert nlen[tables.verse_index(97, 1)] > 0      # a span above starts behind a bismillah


def test_header_constants_match_the_bindings_and_the_restatement():
    from offline_tarteel_amd import engine as e
    from offline_tarteel_amd.engine import exported_symbols

    hdr = open(e.Path(e.__file__).resolve().parent.parent / "include" / "qverse.h").read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))  # noqa: E731
    assert (val("QV_CORRECT_MAX_REF"), val("QV_CORRECT_MAX_WORDS"), val("QV_CORRECT_MAX_RAW")) == (cr.MAX_REF, cr.MAX_WORDS, cr.MAX_RAW) == (
        e.CORRECT_MAX_REF, e.CORRECT_MAX_WORDS, e.CORRECT_MAX_RAW)
    flags = dict(re.findall(r"(QV_CORRECT_[A-Z_]+) = (\d+)", hdr))
    assert {k: int(v) for k, v in flags.items()} == {"QV_CORRECT_PREFIX": 1, "QV_CORRECT_NO_TARGET": 1, "QV_CORRECT_NO_TRANSCRIPT": 2,
                                                    "QV_CORRECT_TOO_LONG": 4, "QV_CORRECT_LAST_WORD_OPEN": 8}
    assert (e.CORRECT_NO_TARGET, e.CORRECT_NO_TRANSCRIPT, e.CORRECT_TOO_LONG, e.CORRECT_LAST_WORD_OPEN) == (
        cr.NO_TARGET, cr.NO_TRANSCRIPT, cr.TOO_LONG, cr.LAST_WORD_OPEN)
    assert tuple(e.CORRECT_INFO_FIELDS) == cr.INFO_FIELDS and tuple(e.CORRECT_WORD_FIELDS) == cr.WORD_FIELDS
    assert {"qv_correct", "qv_correct_results_ctx"} <= set(exported_symbols())


def test_library_exports_the_new_entries():
    from offline_tarteel_amd import LIB_PATH

    lib = ctypes.CDLL(str(LIB_PATH))
    for name in ("qv_correct", "qv_correct_results_ctx"):
        assert hasattr(lib, name), name


def device_row(r, pred, ref):
    """a restatement result as the dict Engine.correct returns"""
    from offline_tarteel_amd.engine import CORRECT_WORD_DTYPE

    d = dict(r["info"])
    d["ops"] = np.array(r["ops"], np.uint8)
    d["words"] = np.array(r["words"], CORRECT_WORD_DTYPE) if r["words"] else np.zeros(0, CORRECT_WORD_DTYPE)
    d["pred_codes"], d["ref_codes"] = np.array(pred, np.uint8), np.array(ref, np.uint8)
    return d


def test_fold_known_row(tables):
    from offline_tarteel_amd import correction

    v = tables.verse_index(112, 1)                                       # قل هو الله احد / الله الصمد
    ref = tables.span_codes(v, 2).tolist()
    text = tables.decode(ref).split(" ")
    assert len(text) == 6
    extra = text[0][0]
    wrong = text[5][-2]
    said = [text[0], text[2], text[3][:-1] + wrong, text[4][:2] + extra + text[4][2:], text[5]]   # a dropped word, a wrong letter, an extra letter
    pred = tables.encode(" ".join(said)).tolist()
    row = device_row(cr.correct(pred, ref, start_verse=v, span=2), pred, ref)
    got = correction.fold(tables, row)
    assert got["errors"] == [
        {"word_index": 1, "ayah": 1, "word": 2, "text": text[1], "expected": text[1], "got": "", "error_type": "deletion"},
        {"word_index": 3, "ayah": 1, "word": 4, "text": text[3], "expected": text[3][-1], "got": wrong, "error_type": "substitution"},
        {"word_index": 4, "ayah": 2, "word": 1, "text": text[4], "expected": "", "got": extra, "error_type": "insertion"}]
    assert got["distance"] == 2 + len(text[1]) and got["words_touched"] == 6 and got["flags"] == 0
    n = row["n_ref"]
    assert got["per"] == got["distance"] / n and got["correct_rate"] == (n - 1 - len(text[1])) / n
    assert correction.word_status(got) == {(1, 2): "deletion", (1, 4): "substitution", (2, 1): "insertion"}
    # explicit texts carry no verse: words count through the text
    plain = correction.fold(tables, device_row(cr.correct(pred, ref), pred, ref))
    assert [(e["ayah"], e["word"]) for e in plain["errors"]] == [(None, 2), (None, 4), (None, 5)]
    # prefix mode: the first two words and a half -- nothing wrong, the rate over what was compared
    half = tables.encode(" ".join(text[:2]) + " " + text[2][:2]).tolist()
    pre = correction.fold(tables, device_row(cr.correct(half, ref, True, start_verse=v, span=2), half, ref))
    assert pre == {"errors": [], "per": 0.0, "correct_rate": 1.0, "distance": 0, "words_touched": 3, "flags": cr.LAST_WORD_OPEN}
    # a row without an alignment
    none = correction.fold(tables, device_row(cr.correct([], ref), [], ref))
    assert none == {"errors": [], "per": 0.0, "correct_rate": 0.0, "distance": 0, "words_touched": 0, "flags": cr.NO_TRANSCRIPT}
    assert correction.word_places(tables, tables.verse_index(97, 1), 2, 10)[:6] == [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 1)]
