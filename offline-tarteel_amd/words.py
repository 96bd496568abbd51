"""Word timings from a token-level forced alignment (host only).

The device aligns the SentencePiece ids of the recognised verse or span to the encoder frames
(Engine.align_results, csrc/qv_align.hip); this module folds tokens into words and words into ayat.
The reference reports `word_index / total_words` per verse in tracking mode (web/server.py:473-525) from a
fuzzy match of recognised words; here the positions are the frames of the Viterbi path itself.
"""

from __future__ import annotations

FRAME_SECONDS = 0.08   # one encoder frame = 1,280 samples at 16 kHz (three stride-2 stages over 10 ms mel frames)


def ayah_word_counts(tables, start: int, span: int) -> list[int]:
    """Words per ayah of the text the token list (start, span) was tokenised from (tools/build_tables.py:148-162:
    a single verse is its clean text; in a span the first ayah loses its bismillah where it has one)."""
    t = tables.s
    if span == 1:
        return [int(t["clean_nw"][start])]
    return [int(t["nobsm_nw"][start]) or int(t["clean_nw"][start])] + [int(t["clean_nw"][start + j]) for j in range(1, span)]


def words_from_alignment(tables, start, span, alignment) -> list[dict]:
    """alignment: {"ids", "first", "last", "logp"[, "flags"]} of one row (Engine.align_results / Engine.align).
    Returns one dict per word: {"ayah", "word" (1-based within the ayah's aligned text), "text", "start", "end"
    (seconds), "logp" (frame-weighted mean of its tokens' mean log-probs)}; [] when the row has no alignment.
    A word starts at a piece whose surface begins with a space and whose id is not 0; <unk> (id 0, surface ' ⁇ ')
    belongs to the word in progress.  start = None (explicit targets, no verse): "ayah" is None and "word" counts
    through the whole text."""
    if not alignment or alignment.get("flags", 0) or not len(alignment["ids"]):
        return []
    ids, first, last, logp = (alignment[k] for k in ("ids", "first", "last", "logp"))
    groups: list[list[int]] = []
    for i, tok in enumerate(ids):
        tok = int(tok)
        if not groups or (tok != 0 and tables.piece_surface[tok].startswith(" ")):
            groups.append([])
        groups[-1].append(i)
    counts = ayah_word_counts(tables, int(start), int(span)) if start is not None else None
    first_ayah = int(tables.ayah[int(start)]) if start is not None else None
    out = []
    ay, in_ay = 0, 0          # ayah of the span (0-based), words already placed in it
    for g in groups:
        if counts is not None:
            while ay < len(counts) - 1 and in_ay >= counts[ay]:
                ay, in_ay = ay + 1, 0
        in_ay += 1
        frames = [int(last[i]) - int(first[i]) + 1 for i in g]
        out.append({
            "ayah": first_ayah + ay if counts is not None else None,
            "word": in_ay,
            "text": "".join(tables.piece_surface[int(ids[i])] for i in g).strip(),
            "start": int(first[g[0]]) * FRAME_SECONDS,
            "end": (int(last[g[-1]]) + 1) * FRAME_SECONDS,
            "logp": sum(float(logp[i]) * n for i, n in zip(g, frames)) / sum(frames),
        })
    return out


def verses_from_alignment(tables, verses, verse_ends, alignment) -> list[dict]:
    """alignment: one row of Engine.align_long / align_windows for the target tables.range_token_ids built; verses: the
    global verse indices it covers, verse_ends: the running token count behind each.  Returns one dict per verse:
    {"surah", "ayah", "start", "end" (seconds), "logp" (frame-weighted mean of its tokens' mean log-probs), "words"
    (words_from_alignment on the verse's own tokens, span 1)}; [] when the row has no alignment."""
    if not alignment or alignment.get("flags", 0) or not len(alignment["ids"]):
        return []
    out, lo = [], 0
    for v, hi in zip(verses, verse_ends):
        v, hi = int(v), int(hi)
        part = {k: alignment[k][lo:hi] for k in ("ids", "first", "last", "logp")}
        words = words_from_alignment(tables, v, 1, part)
        frames = [int(l) - int(f) + 1 for f, l in zip(part["first"], part["last"])]
        out.append({
            "surah": int(tables.surah[v]), "ayah": int(tables.ayah[v]),
            "start": words[0]["start"] if words else None,
            "end": words[-1]["end"] if words else None,
            "logp": sum(float(x) * n for x, n in zip(part["logp"], frames)) / sum(frames) if frames else None,
            "words": words,
        })
        lo = hi
    return out
