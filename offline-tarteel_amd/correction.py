"""Wrong words of a recitation from the device's symbol alignment (host only).

The device compares what was heard with the recognised verse symbol by symbol (Engine.correct / Engine.correct_results,
csrc/qv_correct.hip) and returns op codes per alignment column plus counters per reference word.  This module folds one such
row into the shape the reference's computeCorrection returns (web/frontend/src/lib/correction.ts:80-90: word_index, expected,
got, error_type), with the word's place in its ayah added the way words.py numbers the word timings, so the two join on
("ayah", "word").
"""

from __future__ import annotations

from .words import ayah_word_counts

MATCH, SUB, DEL, INS = 0, 1, 2, 3
ERROR_TYPES = {SUB: "substitution", DEL: "deletion", INS: "insertion"}
ROW_FLAGS = 1 | 2 | 4   # NO_TARGET | NO_TRANSCRIPT | TOO_LONG: the row holds no alignment


def _symbols(codes):
    """(symbols, word index of every symbol, symbols of every word)"""
    sym, word, words = [], [], [[]]
    for c in codes:
        c = int(c)
        if c == 0:
            words.append([])
        else:
            sym.append(c)
            word.append(len(words) - 1)
            words[-1].append(c)
    return sym, word, words


def word_places(tables, start, span, n_words: int) -> list[tuple]:
    """(ayah, word) of every word of the text (start, span), word 1-based within its ayah as words.words_from_alignment
    counts; start < 0 or None (explicit texts): (None, k + 1)."""
    if start is None or start < 0 or not span:
        return [(None, k + 1) for k in range(n_words)]
    first = int(tables.ayah[int(start)])
    out = []
    for a, cnt in enumerate(ayah_word_counts(tables, int(start), int(span))):
        out.extend((first + a, w + 1) for w in range(cnt))
    assert len(out) == n_words, (len(out), n_words)
    return out


def fold(tables, row: dict, pred_codes=None, ref_codes=None) -> dict:
    """row: one dict of Engine.correct / Engine.correct_results; the two texts as alphabet codes with their spaces (default:
    the row's own "pred_codes" / "ref_codes", which correct_results(texts=True) attaches).  Returns {"errors", "per",
    "correct_rate", "distance", "words_touched", "flags"}: errors lists the words with an error in word order, each
    {"word_index", "ayah", "word", "text" (the reference word), "expected" (reference symbols of its substitutions and
    deletions), "got" (heard symbols of its substitutions and insertions), "error_type" ("substitution" if it has any, else
    the type of its first error)}; per = distance / symbols compared, correct_rate = matches / symbols compared
    (shared/phoneme_aligner.py:150-152; with nothing compared per counts the edits and correct_rate is 0)."""
    flags = int(row["flags"])
    if flags & ROW_FLAGS:
        return {"errors": [], "per": 0.0, "correct_rate": 0.0, "distance": 0, "words_touched": 0, "flags": flags}
    pred, _, _ = _symbols(row["pred_codes"] if pred_codes is None else pred_codes)
    ref, word, words = _symbols(row["ref_codes"] if ref_codes is None else ref_codes)
    n = len(ref)
    assert n == row["n_ref"] and len(pred) == row["n_pred"] and len(words) == row["n_words"], "texts do not belong to this row"
    expected = [[] for _ in words]
    got = [[] for _ in words]
    i = j = 0
    for op in row["ops"]:
        op = int(op)
        w = word[i] if i < n else word[n - 1]
        if op in (SUB, DEL):
            expected[w].append(ref[i])
        if op in (SUB, INS):
            got[w].append(pred[j])
        i += op != INS
        j += op != DEL
    assert i == row["n_ref_used"] and j == len(pred)
    places = word_places(tables, row.get("start_verse"), row.get("span"), len(words))
    errors = []
    for k, rec in enumerate(row["words"]):
        t = int(rec["type"])
        if t:
            errors.append({"word_index": k, "ayah": places[k][0], "word": places[k][1], "text": tables.decode(words[k]),
                           "expected": tables.decode(expected[k]), "got": tables.decode(got[k]), "error_type": ERROR_TYPES[t]})
    used = int(row["n_ref_used"])
    return {"errors": errors,
            "per": row["distance"] / used if used else float(row["distance"]),
            "correct_rate": row["n_match"] / used if used else 0.0,
            "distance": int(row["distance"]), "words_touched": int(row["words_touched"]), "flags": flags}


def word_status(folded: dict) -> dict:
    """{(ayah, word): "substitution" | "deletion" | "insertion"} of a folded row: what the plugin joins onto the word timings"""
    return {(e["ayah"], e["word"]): e["error_type"] for e in folded["errors"]}
