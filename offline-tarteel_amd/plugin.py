"""Host-side mirror of the reference's plugin surface for this path
(experiments/c2c-direct-mixed/run.py and experiments/c2c-direct-mixed-tta/run.py):
``predict(audio_path) -> dict``, ``transcribe(audio_path) -> str``, ``model_size() -> int``,
plus the batched entry the throughput metric needs (``predict_batch``).

Same dict keys (surah, ayah, ayah_end, score, transcript, source; _empty on no match), same env
knobs (CTC_DIRECT_*, C2C_DIRECT_MIXED_PROFILE), same error behaviour (missing model ->
FileNotFoundError; any exception propagates to the runner, which records an empty prediction).

Model weights: ``QVERSE_WEIGHTS`` names the flat weight file produced by
tools/convert_weights.py from the reference's checkpoint.  Without it ``predict`` raises
FileNotFoundError like the reference does for a missing ONNX -- unless
``QVERSE_RANDOM_WEIGHTS=1`` explicitly asks for the seeded synthetic weights (throughput runs).
"""

from __future__ import annotations

import os
import time
from collections import Counter
from pathlib import Path

import numpy as np

from .audio import load_audio

_PROFILE = os.getenv("C2C_DIRECT_MIXED_PROFILE", "") not in ("", "0", "false", "False")
CONFIDENCE_SKIP_THRESHOLD = 0.5  # c2c-direct-mixed-tta/run.py:57
MAX_SAMPLES = int(os.getenv("QVERSE_MAX_SAMPLES", str(16000 * 60)))
MAX_BATCH = int(os.getenv("QVERSE_MAX_BATCH", "16"))
# matching window in normalised characters: 1024 (default) or 2048 (the wide kernel set; include/qverse.h qv_config.max_transcript)
MAX_TRANSCRIPT = int(os.getenv("QVERSE_MAX_TRANSCRIPT", "1024"))

# QVERSE_PRECISION: "fp16" (default), "mixed" (the engine's own W4A16 / W8A16 kernels) or "ort" -- the arithmetic
# onnxruntime runs on the reference's fastconformer_full_mixed.onnx (include/qverse.h QV_PREC_ORT_MIXED); with a weight
# file converted from that ONNX (marked pre-quantised) "ort" computes on the file's own integers
_PRECISIONS = {"fp16": 0, "mixed": 1, "ort": 2}
# QVERSE_WORDS=1: predict() adds "words" -- per-word timings of the recognised verse from the device's forced alignment
# (Engine.align_results + words.words_from_alignment); [] when there is no prediction or the alignment carries a flag
_WORDS = os.getenv("QVERSE_WORDS", "") not in ("", "0", "false", "False")
# QVERSE_CANDIDATES=K: predict() adds the reference's "candidates" list (c2c-direct/run.py:424-435) with up to K entries
# (1..32; the reference keeps 5) -- see predict_candidates
_CANDIDATES = int(os.getenv("QVERSE_CANDIDATES", "0") or 0) or None
# QVERSE_CORRECTIONS=1: predict() adds "correction" -- the words of the recognised verse the reciter got wrong, from the
# device's symbol alignment of the transcript with the verse (Engine.correct_results + correction.fold); see predict_corrections
_CORRECTIONS = os.getenv("QVERSE_CORRECTIONS", "") not in ("", "0", "false", "False")
_engine = None
_last_raw: list[dict] = []   # engine-level dicts of the most recent predict_arrays() call (profile line)


def weights_path() -> Path | None:
    p = os.getenv("QVERSE_WEIGHTS")
    return Path(p) if p else None


def _ensure_engine():
    global _engine
    if _engine is not None:
        return _engine
    from .engine import Engine

    wp = weights_path()
    if wp is None and os.getenv("QVERSE_RANDOM_WEIGHTS", "") not in ("1", "true", "True"):
        raise FileNotFoundError(
            "No model weights: set QVERSE_WEIGHTS to the flat file written by tools/convert_weights.py "
            "(from fastconformer_full_mixed.onnx / the .nemo checkpoint), or QVERSE_RANDOM_WEIGHTS=1 for "
            "seeded synthetic weights.")
    if wp is not None and not wp.exists():
        raise FileNotFoundError(f"No weight file at {wp}. Run `python tools/convert_weights.py` first.")
    device = int(os.getenv("LOCAL_RANK", "0"))
    prec_name = os.getenv("QVERSE_PRECISION", "fp16")
    if prec_name not in _PRECISIONS:
        raise ValueError(f"QVERSE_PRECISION={prec_name!r}: expected one of {sorted(_PRECISIONS)}")
    if MAX_TRANSCRIPT not in (1024, 2048):
        raise ValueError(f"QVERSE_MAX_TRANSCRIPT={MAX_TRANSCRIPT}: expected 1024 or 2048")
    print(f"[c2c-direct-mixed/qverse] loading {'synthetic weights' if wp is None else wp.name} on cuda:{device} ({prec_name})...")
    _engine = Engine(device=device, with_model=True, weights_path=str(wp) if wp else None, precision=_PRECISIONS[prec_name],
                     max_batch=MAX_BATCH, max_samples=MAX_SAMPLES, max_transcript=MAX_TRANSCRIPT)
    if _PROFILE:
        _engine.profile_stages(True)
    return _engine


def _empty(transcript: str = "") -> dict:
    return {"surah": 0, "ayah": 0, "ayah_end": None, "score": 0.0, "transcript": transcript, "candidates": []}


def _to_dict(r: dict, round_score: bool) -> dict:
    if not r["surah"]:
        return _empty(r.get("transcript", ""))
    score = r["score"]
    return {
        "surah": r["surah"], "ayah": r["ayah"], "ayah_end": r["ayah_end"] or r["ayah"],
        "score": round(score, 4) if round_score else score,
        "transcript": r.get("transcript", ""), "source": r["source"],
    }


def _words_of(eng, r: dict) -> list[dict]:
    from .words import words_from_alignment

    a = r.get("alignment")
    if not r["surah"] or not a or a["flags"]:
        return []
    return words_from_alignment(eng.tables, a["start"], a["span"], a)


def shape_candidates(nbest: list[dict]) -> list[dict]:
    """An engine n-best list as the reference's "candidates" (c2c-direct/run.py:424-435): ranked[:K] when the rerank ranked
    anything, [best] with the text score otherwise, [] for an empty prediction; scores rounded to 4 places."""
    return [{"surah": e["surah"], "ayah": e["ayah"], "ayah_end": e["ayah_end"] or e["ayah"], "score": round(float(e["score"]), 4)}
            for e in nbest]


def _finish(eng, raw: list[dict], round_score: bool, words: bool, candidates: int | None = None,
            corrections: bool = False) -> list[dict]:
    out = [_to_dict(r, round_score) for r in raw]
    if words:
        for d, r in zip(out, raw):
            d["words"] = _words_of(eng, r)
    if corrections:
        from .correction import fold, word_status

        for d, r in zip(out, raw):
            d["correction"] = fold(eng.tables, r["correction"])
            if words:   # the timings and the correction number the words of one text the same way
                status = word_status(d["correction"])
                for w in d["words"]:
                    w["status"] = status.get((w["ayah"], w["word"]), "ok")
    if candidates is not None:
        for d, r in zip(out, raw):
            d["candidates"] = shape_candidates(r["nbest"]) if r["surah"] else []
    return out


def trie_fallback_enabled() -> bool:
    """QVERSE_TRIE_FALLBACK=1 (off by default): a row predict() / predict_batch() would return without a prediction takes the
    best COMPLETE hypothesis of the verse-constrained beam search (Engine.beam_batch), provided it outranks every incomplete
    one.  Unset, every output is what it was."""
    return os.getenv("QVERSE_TRIE_FALLBACK", "") not in ("", "0", "false", "False")


def _trie_fallback(eng, out: list[dict], raw: list[dict], beam_rows) -> list[dict]:
    """beam_rows(indices) -> Engine.beam_batch rows of those clips.  A row without a prediction becomes the search's first
    hypothesis when that one is complete (so the best complete hypothesis outranks every incomplete one): "source": "trie",
    "score" the hypothesis' log-probability, unrounded."""
    missing = [i for i, r in enumerate(raw) if not r["surah"]]
    if not missing:
        return out
    for i, row in zip(missing, beam_rows(missing)):
        hyps = row["hypotheses"]
        if hyps and hyps[0]["complete"]:
            h = hyps[0]
            extra = {k: v for k, v in out[i].items() if k in ("words", "candidates", "correction")}
            out[i] = {"surah": h["surah"], "ayah": h["ayah"], "ayah_end": h["ayah_end"], "score": h["score"],
                      "transcript": out[i].get("transcript", ""), "source": "trie", **extra}
    return out


def scan_fallback_enabled() -> bool:
    """QVERSE_SCAN_FALLBACK=1 (off by default): a row predict() / predict_batch() would return without a prediction takes the
    first entry of the exhaustive CTC scan (Engine.scan_batch).  With QVERSE_TRIE_FALLBACK set as well the scan runs first and
    the rows it leaves empty go to the trie route.  Unset, every output is what it was."""
    return os.getenv("QVERSE_SCAN_FALLBACK", "") not in ("", "0", "false", "False")


def _scan_candidates(cands: list[dict]) -> list[dict]:
    """scan entries as "candidates": score = round(exp(-loss / L), 4), the reference's ctc_confidence; a single verse's
    ayah_end is its ayah, as everywhere in the plugin"""
    import math

    return [{"surah": e["surah"], "ayah": e["ayah"], "ayah_end": e["ayah_end"], "score": round(math.exp(-e["norm"]), 4)} for e in cands]


def _scan_fallback(eng, out: list[dict], raw: list[dict], scan_rows) -> tuple[list[dict], list[dict]]:
    """scan_rows(indices) -> Engine.scan_batch rows of those clips.  A row without a prediction becomes the scan's first entry:
    "source": "scan".  Returns (out, raw) with the filled rows marked in a copy of raw, so a later fallback skips them."""
    missing = [i for i, r in enumerate(raw) if not r["surah"]]
    if not missing:
        return out, raw
    raw = list(raw)
    for i, row in zip(missing, scan_rows(missing)):
        cands = _scan_candidates(row["candidates"])
        if cands:
            extra = {k: v for k, v in out[i].items() if k in ("words", "candidates", "correction")}
            out[i] = {**cands[0], "transcript": out[i].get("transcript", ""), "source": "scan", **extra}
            raw[i] = {**raw[i], "surah": cands[0]["surah"]}
    return out, raw


def _fallbacks(eng, part: list[dict], raw: list[dict], rows_of) -> list[dict]:
    """the opt-in routes for rows without a prediction, the scan before the trie; rows_of(indices) -> (audio rows, lengths)"""
    if scan_fallback_enabled():
        part, raw = _scan_fallback(eng, part, raw, lambda idx: eng.scan_batch(*rows_of(idx), k=1))
    if trie_fallback_enabled():
        part = _trie_fallback(eng, part, raw, lambda idx: eng.beam_batch(*rows_of(idx)))
    return part


def predict_arrays(arrays, round_score: bool = True, words: bool = False, candidates: int | None = None,
                   corrections: bool = False, prefix: bool = False) -> list[dict]:
    """audio arrays (float32, 16 kHz) -> predict()-shaped dicts, one engine call per <= MAX_BATCH.
    words=True: every dict gains "words" (see predict_words); candidates=K: "candidates" (see predict_candidates);
    corrections=True: "correction" (see predict_corrections; prefix=True: the recitation may stop mid-verse)."""
    import torch

    eng = _ensure_engine()
    out = []
    for s in range(0, len(arrays), eng.max_batch):
        chunk = arrays[s: s + eng.max_batch]
        lens = [len(a) for a in chunk]
        buf = np.zeros((len(chunk), max(lens)), dtype=np.float32)
        for i, a in enumerate(chunk):
            buf[i, : len(a)] = a
        dev = torch.from_numpy(buf).cuda(eng.device)
        raw = eng.predict_batch(dev, lens, align=words, nbest=candidates, correct=corrections, correct_prefix=prefix)
        _last_raw[:] = raw
        part = _finish(eng, raw, round_score, words, candidates, corrections)
        part = _fallbacks(eng, part, raw, lambda idx: (dev[idx].contiguous(), [lens[i] for i in idx]))
        out.extend(part)
    return out


def predict_device(dev, lens, round_score: bool = True, words: bool = False, candidates: int | None = None,
                   corrections: bool = False, prefix: bool = False) -> list[dict]:
    """a zero-padded float32 cuda matrix of 16 kHz clips -> predict()-shaped dicts, one engine call per <= MAX_BATCH rows"""
    eng = _ensure_engine()
    out = []
    for s in range(0, len(lens), eng.max_batch):
        chunk = lens[s: s + eng.max_batch]
        rows = dev[s: s + len(chunk), : max(chunk)].contiguous()
        raw = eng.predict_batch(rows, chunk, align=words, nbest=candidates, correct=corrections, correct_prefix=prefix)
        _last_raw[:] = raw
        part = _finish(eng, raw, round_score, words, candidates, corrections)
        part = _fallbacks(eng, part, raw, lambda idx, rows=rows, chunk=chunk: (rows[idx].contiguous(), [chunk[i] for i in idx]))
        out.extend(part)
    return out


def predict_batch(audio_paths, words: bool = False, candidates: int | None = None, corrections: bool = False,
                  prefix: bool = False) -> list[dict]:
    """files -> dicts.  The ingest (mix-down, resampling to 16 kHz) runs on the GPU (audio.load_audio_device: the same float32
    arithmetic as the host load_audio, bit for bit); QVERSE_INGEST=host keeps it on the host.
    words=True: every dict gains "words" (see predict_words); candidates=K: every dict carries "candidates" (see
    predict_candidates); corrections=True: every dict gains "correction" (see predict_corrections), and with words=True every
    entry of "words" a "status" ("ok", "substitution", "deletion" or "insertion"); without them the dicts are unchanged."""
    if os.getenv("QVERSE_INGEST", "device") == "host":
        return predict_arrays([load_audio(p) for p in audio_paths], words=words, candidates=candidates, corrections=corrections,
                              prefix=prefix)
    from .audio import load_audio_device

    dev, lens = load_audio_device(list(audio_paths), _ensure_engine())
    return predict_device(dev, lens, words=words, candidates=candidates, corrections=corrections, prefix=prefix)


def predict_corrections(audio_path: str, prefix: bool = False) -> dict:
    """predict() plus "correction": which words of the recognised verse or span were recited wrong.  {"errors": [{"word_index",
    "ayah", "word" (1-based within the ayah, as in predict_words), "text", "expected", "got", "error_type" ("substitution",
    "deletion" or "insertion")}], "per", "correct_rate", "distance", "words_touched", "flags"} from the device's Levenshtein
    alignment of the transcript with the verse's text (Engine.correct_results, correction.fold); no errors and flags != 0 when
    nothing was recognised.  prefix=True: the recitation may stop anywhere in the verse -- the unrecited rest is not an
    error, "words_touched" says how far it got."""
    return predict_arrays([load_audio(audio_path)], corrections=True, prefix=prefix)[0]


def predict_candidates(audio_path: str, k: int = 5) -> dict:
    """predict() plus the reference's "candidates" (c2c-direct/run.py:424-435): up to k {"surah", "ayah", "ayah_end",
    "score"} dicts, best first -- the head of the CTC rerank's ranking with its final scores when the rerank decided, the
    text match with its score when the gate passed, [] when nothing was recognised.  Selected on the device
    (Engine.nbest_results)."""
    return predict_arrays([load_audio(audio_path)], candidates=k)[0]


def predict_constrained(audio_path: str, beam: int = 8, k: int = 5) -> dict:
    """The verse-constrained route on its own (the reference's trie beam search, web/frontend/src/worker/beam-decode.ts): no
    greedy transcript, no text matching.  {"t_frames", "max_candidates", "hypotheses"}: up to k prefixes of real verses (or of
    up to three consecutive ones), best first, each {"surah", "ayah", "ayah_end", "score" (log-probability), "complete",
    "n_tokens", "text", "matches", "reachable", "first_reachable", ...} as Engine.beam_logprobs documents them.  A recitation
    that stops mid-verse comes back as an incomplete prefix with the verses still reachable."""
    import torch

    eng = _ensure_engine()
    audio = load_audio(audio_path)
    dev = torch.from_numpy(audio[None, :]).cuda(eng.device)
    return eng.beam_batch(dev, [len(audio)], beam=beam, k=k)[0]


def predict_exhaustive(audio_path: str, k: int = 5, surahs=None) -> dict:
    """The exhaustive route on its own (the reference's brute force, experiments/fastconformer-nbest-bruteforce/run.py, without
    its 10-surah limit): every verse and every span of up to six ayat -- of `surahs`, or of the whole Quran -- CTC-scored
    against the clip, no transcript, no text matching.  {"surah", "ayah", "ayah_end", "score", "source": "scan",
    "candidates": [up to k of {"surah", "ayah", "ayah_end", "score"}, best first]}; score = round(exp(-loss / L), 4), the
    reference's ctc_confidence; the ranking uses the engine's CTC_DIRECT_SPAN_PENALTY.  Empty (surah 0) when the clip has
    fewer frames than any verse's 2 L + 1 states."""
    import torch

    eng = _ensure_engine()
    audio = load_audio(audio_path)
    dev = torch.from_numpy(audio[None, :]).cuda(eng.device)
    cands = _scan_candidates(eng.scan_batch(dev, [len(audio)], k=k, surahs=surahs)[0]["candidates"])
    if not cands:
        return {"surah": 0, "ayah": 0, "ayah_end": None, "score": 0.0, "source": "scan", "candidates": []}
    return {**cands[0], "source": "scan", "candidates": cands}


def predict_words(audio_path: str) -> dict:
    """predict() plus "words": for every word of the recognised verse or span {"ayah", "word" (1-based within the ayah),
    "text", "start", "end" (seconds), "logp"} from the forced alignment of the verse's tokens to the encoder frames
    (0.08 s per frame); [] when nothing was recognised or no alignment exists (text longer than 383 tokens, fewer
    frames than tokens)."""
    return predict_arrays([load_audio(audio_path)], words=True)[0]


def predict(audio_path: str) -> dict:
    t0 = time.perf_counter()
    audio = load_audio(audio_path)
    t1 = time.perf_counter()
    res = predict_arrays([audio], words=_WORDS, candidates=_CANDIDATES, corrections=_CORRECTIONS)[0]
    if _PROFILE:
        # the reference's line (mixed/run.py:76-81,117-124): forward= decode= build= rerank= total=
        # candidates= use_ctc= source= -- stage times from HIP events around the device stages of this
        # file's batch of one; `forward` includes the audio load like the reference's _ctc_logprobs does
        t2 = time.perf_counter()
        st = _ensure_engine().stage_times()
        raw = _last_raw[0] if _last_raw else {}
        head = f"[c2c-direct-mixed profile] audio={Path(audio_path).name} "
        fwd = (t1 - t0) + st["forward"]
        if not res.get("transcript", "").strip():
            print(head + f"forward={fwd:.3f}s decode={st['decode']:.3f}s total={t2 - t0:.3f}s empty=1")
        elif not res["surah"]:
            print(head + f"forward={fwd:.3f}s decode={st['decode']:.3f}s build={st['build']:.3f}s "
                         f"total={t2 - t0:.3f}s no_candidates=1")
        else:
            use_ctc = int(bool(raw.get("use_ctc")))
            print(head + f"forward={fwd:.3f}s decode={st['decode']:.3f}s build={st['build']:.3f}s "
                         f"rerank={st['rerank'] if use_ctc else 0.0:.3f}s total={t2 - t0:.3f}s "
                         f"candidates={raw.get('n_candidates', 0)} use_ctc={use_ctc} source={res.get('source')}")
    return res


def transcribe(audio_path: str) -> str:
    import torch

    eng = _ensure_engine()
    audio = load_audio(audio_path)
    dev = torch.from_numpy(audio[None, :]).cuda(eng.device)
    if len(audio) > eng.max_samples:   # longer than the engine's capacity: overlapping windows, stitched on the device
        return eng.transcribe_long(dev, [len(audio)])[0]["text"]
    lp, T = eng.forward(dev, [len(audio)])
    ids = lp[0, : T[0]].argmax(-1).cpu().numpy().tolist()
    dedup, prev = [], -1
    for i in ids:
        if i != prev and i != 1024:
            dedup.append(i)
        prev = i
    return eng.transcript_of(dedup)


def transcribe_detailed(audio_path: str) -> dict:
    """transcribe() with confidence: {"text", "avg_logprob", "frame_avg_logprob", "min_token_logprob", "n_tokens",
    "t_frames", "tokens": [{"id", "first", "last", "logp"}], ...} from Engine.transcribe_batch(confidence=True) -- argmax,
    collapse and the confidence figures in one kernel on the device.  Usable as a reference-style ``transcribe_fn`` that
    returns a dict (shared/streaming.py:158-166 reads "text" and "avg_logprob")."""
    import torch

    eng = _ensure_engine()
    audio = load_audio(audio_path)
    dev = torch.from_numpy(audio[None, :]).cuda(eng.device)
    if len(audio) > eng.max_samples:   # as transcribe(): the same dict plus "n_windows", token frames of the whole recording
        return eng.transcribe_long(dev, [len(audio)])[0]
    return eng.transcribe_batch(dev, [len(audio)], confidence=True)[0]


def _align_verses(eng, audio_path, verses, ids=None, ends=None) -> tuple[dict, list[dict]]:
    """the recording against the single-verse token lists of `verses` (global indices, in recited order) as ONE target
    (ids, ends: that target where the caller has it already): (the alignment row of Engine.align_long,
    words.verses_from_alignment on it)"""
    import torch

    from .words import verses_from_alignment

    if ids is None:
        parts = [eng.tables.token_ids(int(v), 1) for v in verses]
        ids = np.concatenate(parts).astype(np.uint16) if parts else np.zeros(0, np.uint16)
        ends = np.cumsum([len(p) for p in parts], dtype=np.int64)
    audio = load_audio(audio_path) if isinstance(audio_path, (str, Path)) else np.asarray(audio_path, np.float32)
    dev = torch.from_numpy(np.ascontiguousarray(audio[None, :])).cuda(eng.device)
    row = eng.align_long(dev, [len(audio)], [ids])[0]
    return row, verses_from_alignment(eng.tables, verses, ends, row)


def align_recitation(audio_path: str, surah: int, ayah: int, ayah_end: int | None = None) -> dict:
    """Where in a recording of ANY length every ayah and every word of a KNOWN recitation was spoken: ayat `ayah` ..
    `ayah_end` of `surah` (None = to the end of the surah; up to 16,383 tokens -- the largest surah has 14,403) are aligned as
    one target to the frames of the whole recording (Engine.align_long).  Returns {"score", "flags", "t_frames", "n_windows",
    "verses": [{"surah", "ayah", "start", "end" (seconds), "logp", "words": [...]}]}; "verses" is [] when no alignment exists
    (flags: ALIGN_TOO_LONG, ALIGN_INFEASIBLE -- fewer frames than tokens)."""
    eng = _ensure_engine()
    n_ayat = int(eng.tables.s["surah_len"][surah - 1])
    ayah_end = n_ayat if ayah_end is None else int(ayah_end)
    if not (1 <= ayah <= ayah_end <= n_ayat):
        raise ValueError(f"align_recitation: ayat {ayah}..{ayah_end} outside surah {surah} (1..{n_ayat})")
    start = eng.tables.verse_index(surah, ayah)
    count = ayah_end - ayah + 1
    row, verses = _align_verses(eng, audio_path, list(range(start, start + count)), *eng.tables.range_token_ids(start, count))
    return {"score": row["score"], "flags": row["flags"], "t_frames": row["t_frames"], "n_windows": row["n_windows"], "verses": verses}


# QVERSE_LONG_TIMINGS=1: predict_long() adds "start" / "end" / "logp" to every emission
_LONG_TIMINGS = os.getenv("QVERSE_LONG_TIMINGS", "") not in ("", "0", "false", "False")


def predict_long(audio_path: str, timings: bool = False) -> list[dict]:
    """The verses of a recording of ANY length: the emissions of StreamingPipeline.run_on_full_transcript ({"surah", "ayah",
    "score"} per ayah, in order) on the engine's own transcript -- one forward for a clip the engine accepts, overlapping
    windows stitched on the device (Engine.transcribe_long) for a longer one.  Transcripts above 1,024 normalised characters
    need QVERSE_MAX_TRANSCRIPT=2048.
    timings=True (or QVERSE_LONG_TIMINGS=1): the emitted ayat, in emission order, are aligned to the recording as one target
    (Engine.align_long; the forward runs a second time) and every emission gains "start", "end" (seconds) and "logp" -- None
    when no alignment exists."""
    from .streaming import StreamingPipeline

    eng = _ensure_engine()
    out = StreamingPipeline(eng).run_on_full_transcript(audio_path)
    if not (timings or _LONG_TIMINGS) or not out:
        return out
    _, verses = _align_verses(eng, audio_path, [eng.tables.verse_index(e["surah"], e["ayah"]) for e in out])
    for k, e in enumerate(out):
        v = verses[k] if verses else {}
        e.update(start=v.get("start"), end=v.get("end"), logp=v.get("logp"))
    return out


def model_size() -> int:
    wp = weights_path()
    return wp.stat().st_size if wp is not None and wp.exists() else 0


# ------------------------------------------------------------------ TTA variant --------
def _tta_combine(p09: dict, anchor: dict, p11: dict) -> dict:
    """c2c-direct-mixed-tta/run.py:133-149: majority over (surah, ayah) of [0.9x, anchor, 1.1x],
    else the highest score."""
    preds = [p09, anchor, p11]
    keys = [(p["surah"], p["ayah"]) for p in preds]
    top, n = Counter(keys).most_common(1)[0]
    if n >= 2:
        for p in preds:
            if (p["surah"], p["ayah"]) == top:
                p["tta"] = "majority"
                p["tta_preds"] = keys
                return p
    best = max(preds, key=lambda p: p["score"])
    best["tta"] = "score_pick"
    best["tta_preds"] = keys
    best["tta_scores"] = [p["score"] for p in preds]
    return best


def tta_start(eng, audio, lengths, want_text: bool = True, anchor_ctx: int | None = None) -> dict:
    """First half of tta_device_batch: the anchor results (run here, or fetched from context `anchor_ctx` when the
    caller already launched the anchor pass with predict_batch_async), the 0.5 gate, and the 0.9x / 1.1x copies
    of the gated clips launched as further batches.  With one context those batches are finished here; with more
    they stay in flight until tta_finish() -- a serving loop can launch the next batch's anchor pass in between.

    Round 6: the copies of ALL gated clips of one speed are made by ONE launch (Engine.speed_perturb_rows ->
    qv_upfirdn_batch, straight into the engine's zero-padded input layout) and travel as one batch per speed -- rows of
    similar length, and only the slowed copies can exceed 384 frames -- instead of one launch + one row copy per clip and
    batches that interleave the two speeds."""
    if anchor_ctx is None:
        raw = eng.predict_batch(audio, lengths, want_text=want_text)
    else:
        raw = eng.fetch_results(anchor_ctx, len(lengths), eng.frames_for(max(lengths)), want_text=want_text)
    anchors = [_to_dict(r, False) for r in raw]
    hard = [i for i, a in enumerate(anchors) if a["score"] < CONFIDENCE_SKIP_THRESHOLD]
    st = {"anchors": anchors, "out": list(anchors), "tickets": [], "want_text": want_text, "parts": {}}
    for s0 in range(0, len(hard), eng.max_batch):
        idx = hard[s0: s0 + eng.max_batch]
        lens_in = [lengths[i] for i in idx]
        for factor in (0.9, 1.1):
            rows, lens = eng.speed_perturb_rows(audio, lens_in, factor, src_rows=idx)
            if eng.contexts > 1:
                # the perturbed batches do not depend on one another: keep them in flight (one context stays free for
                # the caller's next anchor pass when there are more than two)
                if len(st["tickets"]) >= max(1, eng.contexts - (1 if eng.contexts > 2 else 0)):
                    _tta_join(eng, st, st["tickets"].pop(0))
                st["tickets"].append((eng.predict_batch_async(rows, lens), idx, rows, eng.frames_for(max(lens)), factor))
                continue
            res = [_to_dict(r, False) for r in eng.predict_batch(rows, lens, want_text=want_text)]
            _tta_part(st, idx, factor, res)
    return st


def _tta_part(st: dict, idx, factor: float, res: list[dict]):
    """one speed's results of the clips `idx`; a clip is decided once both of its copies are in"""
    for k, i in enumerate(idx):
        part = st["parts"].setdefault(i, {})
        part[factor] = res[k]
        if len(part) == 2:
            st["out"][i] = _tta_combine(part[0.9], st["anchors"][i], part[1.1])
            del st["parts"][i]


def _tta_join(eng, st: dict, ticket):
    ctx, idx, rows, t_max, factor = ticket   # (rows: the batch's input, kept alive until it has run)
    res = [_to_dict(r, False) for r in eng.fetch_results(ctx, rows.shape[0], t_max, want_text=st["want_text"])]
    _tta_part(st, idx, factor, res)


def tta_finish(eng, st: dict) -> list[dict]:
    """Second half: join the perturbed batches still in flight and apply the majority / best-score rule."""
    while st["tickets"]:
        _tta_join(eng, st, st["tickets"].pop(0))
    return st["out"]


def tta_device_batch(eng, audio, lengths, want_text: bool = True) -> list[dict]:
    """c2c-direct-mixed-tta/run.py:117-149 for one batch already in HBM (float32 cuda [B, N], zero
    padded): anchor pass over every clip, gate 0.5 on the UNROUNDED score, then the 0.9x / 1.1x copies of
    the gated clips -- made on the GPU (qv_upfirdn, bit-identical to the reference's
    scipy.signal.resample_poly call) -- as further engine batches (the reference runs them as two
    threads on one session), and the majority / best-score rule."""
    return tta_finish(eng, tta_start(eng, audio, lengths, want_text))


def predict_tta_arrays(arrays) -> list[dict]:
    """tta_device_batch for a list of host clips (one engine batch per <= MAX_BATCH clips)."""
    import torch

    eng = _ensure_engine()
    out = []
    for s0 in range(0, len(arrays), eng.max_batch):
        chunk = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays[s0: s0 + eng.max_batch]]
        lens = [len(a) for a in chunk]
        buf = np.zeros((len(chunk), max(lens)), dtype=np.float32)
        for i, a in enumerate(chunk):
            buf[i, : len(a)] = a
        out.extend(tta_device_batch(eng, torch.from_numpy(buf).cuda(eng.device), lens))
    return out


def predict_tta(audio_path: str) -> dict:
    return predict_tta_arrays([load_audio(audio_path)])[0]


def predict_tta_batch(audio_paths) -> list[dict]:
    return predict_tta_arrays([load_audio(p) for p in audio_paths])
