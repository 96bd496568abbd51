"""Generate the golden fixtures that pin oracle/ against the reference.

Run ONLY in the build container (needs /root/reference):

    PYTHONHASHSEED=0 python tests/golden/gen_golden.py

It imports the unmodified reference post-logits code (ref_import.py) and writes

    tests/golden/normalizer_cases.json       shared/normalizer.py I/O pairs
    tests/golden/indel_known_answers.json    hand-computed + reference-shim LCS cases
    tests/golden/tokenizer_cases.json        SentencePiece decode/encode known answers
    tests/golden/retrieval_cases.json.gz     match_verse / search / pass-3 / candidate lists
    tests/golden/e2e_cases.json.gz           synthetic log-probs recipe -> greedy decode,
                                             per-candidate ctc_loss, ranking, predict() dict
    tests/golden/scoring_cases.json          runner.score_sequence known answers
    tests/golden/e2e_textweight_cases.json.gz  (section "textweight") the rerank and the decision with
                                             CTC_DIRECT_TEXT_WEIGHT = 0.35 / 2.0 on three of the e2e recipes
    tests/golden/knob_cases.json.gz          (section "knobs") candidate lists, rerank and decision at seven non-default
                                             settings of TOP_TEXT / TOP_SPAN_REFS / MAX_SPAN / SPAN_PENALTY / TEXT_WEIGHT

Fixtures are data (inputs + expected outputs); no reference source text is stored.
PYTHONHASHSEED is pinned because the reference's tie order follows set iteration
(SURVEY.md section 7 "Tie-breaking").
"""

from __future__ import annotations

import gzip
import json
import math
import os
import random
import sys
from pathlib import Path

if os.environ.get("PYTHONHASHSEED") != "0":
    os.environ["PYTHONHASHSEED"] = "0"
    os.execv(sys.executable, [sys.executable] + sys.argv)

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from ref_import import REF, indel_ratio, load_reference  # noqa: E402
from synth import synth_logits  # noqa: E402  (tests/synth.py: shared, reference-free)


def dump(name, obj, gz=False):
    txt = json.dumps(obj, ensure_ascii=False, separators=(",", ":"))
    path = HERE / name
    if gz:
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(txt.encode("utf-8"))
    else:
        path.write_text(txt, encoding="utf-8")
    print(f"wrote {name}: {path.stat().st_size} bytes")


def main():
    cd = load_reference()
    db = cd._db
    tok = cd._model.tokenizer
    rng = random.Random(20260630)
    sections = set(sys.argv[1:]) or {"small", "retrieval", "e2e"}
    if sections == {"textweight"}:
        return textweight_section(cd, tok, db)
    if sections == {"knobs"}:
        return knobs_section(cd, tok, db)

    # ---------------- normalizer -------------------------------------------
    from shared.normalizer import normalize_arabic

    norm_inputs = []
    for idx in (0, 1, 6, 7, 261, 292, 1000, 2000, 3000, 4444, 6000, 6235):
        norm_inputs.append(db.verses[idx]["text_uthmani"])
    norm_inputs += [
        "",
        "   ",
        "﻿بِسْمِ  ٱللَّهِ‏ ٱلرَّحْمَٰنِ",
        "قَالَ، رَبِّ؟ ... إِنِّي!",
        "آمَنَ ٲ ٳ اٰ ٰ یے ک ـــ ﴿١٢٣﴾ ۝ ۞",
        "hello, world: 123 ١٢٣ ۱۲۳",
        " ⁇ ا ⁇ ",
    ]
    dump(
        "normalizer_cases.json",
        [{"in": s, "out": normalize_arabic(s)} for s in norm_inputs],
    )

    # ---------------- Indel ratio known answers ----------------------------
    hand = [
        # (a, b, lcs) -- LCS worked out by hand
        ("", "", 0),
        ("a", "", 0),
        ("abc", "abc", 3),
        ("abc", "abd", 2),
        ("kitten", "sitting", 4),  # i,t,t,n
        ("lewenstein", "levenshtein", 9),  # l e e n s t e i n
        ("abcdef", "fedcba", 1),
        ("aaaa", "aa", 2),
        ("abab", "baba", 3),
        ("x" * 70, "x" * 65 + "y" * 5, 65),  # crosses a 64-bit word
    ]
    ka = []
    for a, b, lcs in hand:
        r = indel_ratio(a, b)
        la, lb = len(a), len(b)
        expect = 1.0 if la + lb == 0 else 1.0 - (la + lb - 2 * lcs) / (la + lb)
        assert r == expect, (a, b, r, expect)
        ka.append({"a": a, "b": b, "lcs": lcs, "ratio": r, "hand": True})
    # published golden: retasy_005 -> 103:2 @ 0.9444 = 1 - 2/36
    assert round(1.0 - 2 / 36, 4) == 0.9444
    for _ in range(40):
        va = db.verses[rng.randrange(6236)]["text_clean"]
        vb = db.verses[rng.randrange(6236)]["text_clean_alt"]
        r = indel_ratio(va, vb)
        lcs = round((r * (len(va) + len(vb))) / 2)
        ka.append({"a": va, "b": vb, "lcs": lcs, "ratio": r, "hand": False})
    dump("indel_known_answers.json", ka)

    # ---------------- tokenizer --------------------------------------------
    tk = []
    for _ in range(40):
        n = rng.randrange(1, 40)
        ids = [rng.randrange(0, 1024) for _ in range(n)]
        tk.append({"ids": ids, "text": tok.ids_to_text(ids)})
    tk.append({"ids": [0], "text": tok.ids_to_text([0])})
    tk.append({"ids": [10, 10, 9], "text": tok.ids_to_text([10, 10, 9])})
    enc = []
    for idx in (0, 1, 7, 261, 6230, 6235):
        t = db.verses[idx]["text_clean"]
        enc.append({"text": t, "ids": tok.text_to_ids(t)})
    dump("tokenizer_cases.json", {"decode": tk, "encode": enc})

    # ---------------- retrieval cases ---------------------------------------
    def verse(s, a):
        return db.get_verse(s, a)

    def perturb(text, rate, seed):
        r = random.Random(seed)
        alphabet = "ابتثجحخدذرزسشصضطظعغفقكلمنهوي "
        out = []
        for ch in text:
            x = r.random()
            if x < rate / 3:
                continue
            if x < 2 * rate / 3:
                out.append(r.choice(alphabet))
                continue
            out.append(ch)
            if x < rate:
                out.append(r.choice(alphabet))
        return normalize_arabic("".join(out))

    def span_text(s, a0, a1):
        return " ".join(verse(s, a)["text_clean"] for a in range(a0, a1 + 1))

    transcripts = {
        "exact_1_1": verse(1, 1)["text_clean"],
        "exact_112_2": verse(112, 2)["text_clean"],
        "exact_36_1": verse(36, 1)["text_clean"],
        "exact_2_255": verse(2, 255)["text_clean"],
        "refrain_55_13_p": perturb(verse(55, 13)["text_clean"], 0.10, 1),
        "bsm_stripped_78_1": verse(78, 1)["text_clean_no_bsm"],
        "with_bsm_97_1": verse(97, 1)["text_clean"],
        "p05_103_2": perturb(verse(103, 2)["text_clean"], 0.05, 2),
        "p15_3_23": perturb(verse(3, 23)["text_clean"], 0.15, 3),
        "p30_59_23": perturb(verse(59, 23)["text_clean"], 0.30, 4),
        "p45_24_35": perturb(verse(24, 35)["text_clean"], 0.45, 5),
        "span_112_1_4": span_text(112, 1, 4),
        "span_103_1_3_p": perturb(span_text(103, 1, 3), 0.12, 6),
        "span_36_1_5_p": perturb(span_text(36, 1, 5), 0.2, 7),
        "span_114_1_6_p": perturb(span_text(114, 1, 6), 0.35, 8),
        "frag3_2_102": " ".join(verse(2, 102)["text_clean"].split()[5:8]),
        "frag6_2_282": " ".join(verse(2, 282)["text_clean"].split()[20:26]),
        "half_2_282_p": perturb(" ".join(verse(2, 282)["text_clean"].split()[:60]), 0.08, 9),
        "spaceless_67_1": verse(67, 1)["text_clean_no_bsm"].replace(" ", ""),
        "short_2w": "قل هو",
        "one_char": "ق",
        "two_char": "قل",
        "garbage_40": perturb("ا" * 40, 1.0, 10),
        "garbage_words": "زلط كبع شثق ضغظ خذج فقن ملك يوم",
        "unk_marks": "الحمد ⁇ لله رب ⁇ العالمين",
    }

    def keyfloat(x):
        return float(x)

    ret_cases = []
    for name, t in (transcripts.items() if "retrieval" in sections else ()):
        base = db.match_verse(
            t, threshold=0.0, max_span=6, return_top_k=100, use_trigram_index=True
        )
        tri = db._trigram_candidates(normalize_arabic(t), top_k=50)
        srch = db.search(t, top_k=100)
        norm = t
        spaceless = norm.replace(" ", "")
        scored = []
        for v in db.verses:
            s = max(
                indel_ratio(norm, v["text_clean"]),
                indel_ratio(spaceless, v["text_clean"].replace(" ", "")),
            )
            scored.append((s, v))
        p3 = sorted(scored, key=lambda x: x[0], reverse=True)[:100]
        cands, base2 = cd._build_candidates(t)
        case = {
            "name": name,
            "transcript": t,
            "trigram_top50": [int(i) for i in tri],
            "match": None
            if base is None
            else {
                "surah": base["surah"],
                "ayah": base["ayah"],
                "ayah_end": base.get("ayah_end"),
                "score": keyfloat(base["score"]),
                "raw_score": keyfloat(base["raw_score"]),
                "runners_up": [
                    [r["surah"], r["ayah"], keyfloat(r["score"])] for r in base["runners_up"]
                ],
            },
            "search100": [[v["surah"], v["ayah"], keyfloat(v["score"])] for v in srch],
            "pass3_100": [[v["surah"], v["ayah"], keyfloat(s)] for s, v in p3],
            "candidates": [[c["surah"], c["ayah"], c["ayah_end"]] for c in cands],
            "cand_scores": [keyfloat(c.get("score") or 0.0) for c in cands],
        }
        ret_cases.append(case)
        print(
            name,
            len(t),
            None if base is None else (base["surah"], base["ayah"], base.get("ayah_end"), round(base["score"], 4)),
            len(cands),
        )
    if "retrieval" in sections:
        dump("retrieval_cases.json.gz", ret_cases, gz=True)

    # ---------------- end-to-end: logits recipe -> predict ---------------------
    import torch  # noqa: F401

    def run_e2e(name, ids_path, T, seed, noise, boost, rep):
        logits = synth_logits(ids_path, T, seed=seed, noise=noise, boost=boost, rep=rep)
        lp = torch.log_softmax(torch.from_numpy(logits), dim=-1).numpy()
        transcript = cd._greedy_decode(lp)
        am = lp.argmax(-1)
        dedup, prev = [], -1
        for i in am:
            i = int(i)
            if i != prev and i != 1024:
                dedup.append(i)
            prev = i
        out = {
            "name": name,
            "recipe": {"ids": ids_path, "T": T, "seed": seed, "noise": noise, "boost": boost, "rep": rep},
            "greedy_ids": dedup,
            "transcript": transcript,
        }
        if not transcript.strip():
            out["result"] = {"surah": 0, "ayah": 0, "ayah_end": None, "score": 0.0, "source": None}
            return out
        cands, base = cd._build_candidates(transcript)
        use_ctc = base is None or float(base.get("score", 0.0)) < cd.FALLBACK_THRESHOLD
        # always record the rerank so the kernel is pinned on gate-pass cases too
        ranked = cd._ctc_rerank(lp, cands)
        out["base"] = None if base is None else [base["surah"], base["ayah"], base.get("ayah_end"), float(base["score"])]
        out["use_ctc"] = bool(use_ctc)
        out["n_candidates"] = len(cands)
        out["cand_keys"] = [[c["surah"], c["ayah"], c["ayah_end"]] for c in cands]
        out["ctc_loss"] = [
            (float(c["ctc_loss"]) if math.isfinite(c["ctc_loss"]) else None) for c in cands
        ]
        out["ctc_len"] = [int(c["ctc_len"]) for c in cands]
        out["ranked_keys"] = [[c["surah"], c["ayah"], c["ayah_end"]] for c in ranked[:20]]
        out["ranked_final"] = [float(c["final_score"]) for c in ranked[:20]]
        if use_ctc and ranked:
            best = ranked[0]
            score = math.exp(-best["ctc_norm_loss"]) if math.isfinite(best["ctc_norm_loss"]) else 0.0
            src = "ctc"
        elif base:
            best, score, src = base, float(base.get("score", 0.0)), "text"
        else:
            best = None
        if best is None:
            out["result"] = {"surah": 0, "ayah": 0, "ayah_end": None, "score": 0.0, "source": None}
        else:
            out["result"] = {
                "surah": best["surah"],
                "ayah": best["ayah"],
                "ayah_end": best.get("ayah_end") or best["ayah"],
                "score": round(score, 4),
                "score_raw": float(score),
                "source": src,
            }
        print(name, T, len(dedup), out["result"], "use_ctc", use_ctc, "ncand", len(cands))
        return out

    def ids_of(text):
        return [int(i) for i in tok.text_to_ids(text)]

    def corrupt_ids(ids, rate, seed):
        r = random.Random(seed)
        out = []
        for i in ids:
            x = r.random()
            if x < rate / 2:
                continue
            if x < rate:
                out.append(r.randrange(1, 1024))
            else:
                out.append(i)
        return out

    e2e = []
    if "e2e" not in sections:
        return
    e2e.append(run_e2e("clean_1_1", ids_of(verse(1, 1)["text_clean"]), 40, 1, 1.0, 8.0, 2))
    e2e.append(run_e2e("clean_112_2", ids_of(verse(112, 2)["text_clean"]), 20, 2, 1.0, 8.0, 2))
    e2e.append(run_e2e("corrupt_103_2", corrupt_ids(ids_of(verse(103, 2)["text_clean"]), 0.35, 3), 48, 3, 1.0, 7.0, 2))
    e2e.append(run_e2e("corrupt_114_1_6", corrupt_ids(ids_of(span_text(114, 1, 6)), 0.3, 4), 150, 4, 1.0, 6.0, 2))
    e2e.append(run_e2e("corrupt_36_1_5", corrupt_ids(ids_of(span_text(36, 1, 5)), 0.35, 5), 126, 5, 1.0, 6.0, 3))
    e2e.append(run_e2e("corrupt_55_1_4", corrupt_ids(ids_of(span_text(55, 1, 4)), 0.4, 6), 90, 6, 1.0, 6.0, 3))
    e2e.append(run_e2e("noise_only", [], 63, 7, 1.0, 0.0, 1))
    e2e.append(run_e2e("all_blank", [], 30, 8, 0.0, 0.0, 1))
    e2e.append(run_e2e("long_2_255", corrupt_ids(ids_of(verse(2, 255)["text_clean"]), 0.3, 9), 251, 9, 1.0, 6.0, 2))
    e2e.append(run_e2e("tight_T_103_1", ids_of(verse(103, 1)["text_clean_no_bsm"]), 2 * len(ids_of(verse(103, 1)["text_clean_no_bsm"])) + 1, 10, 1.0, 8.0, 1))
    dump("e2e_cases.json.gz", e2e, gz=True)


def textweight_section(cd, tok, db):
    """CTC_DIRECT_TEXT_WEIGHT != 0 (c2c-direct/run.py:62-74,371-373): final = -norm_loss + TEXT_WEIGHT * text_score -
    penalty, where text_score is whatever `score` the candidate carries (match_verse's unrounded best, the runners-up
    rounded to 3 dp, search()'s fragment scores, pass 3's ratios, 0.0 for expanded spans)."""
    import torch

    def verse(s, a):
        return db.get_verse(s, a)

    def span_text(s, a0, a1):
        chunk = [verse(s, a) for a in range(a0, a1 + 1)]
        first = chunk[0].get("text_clean_no_bsm") or chunk[0]["text_clean"]
        return " ".join([first] + [v["text_clean"] for v in chunk[1:]])

    def ids_of(text):
        return [int(i) for i in tok.text_to_ids(text)]

    def corrupt_ids(ids, rate, seed):   # (same recipe as the e2e section)
        r = random.Random(seed)
        out = []
        for i in ids:
            x = r.random()
            if x < rate / 2:
                continue
            if x < rate:
                out.append(r.randrange(1, 1024))
                continue
            out.append(i)
        return out

    recipes = [
        ("corrupt_103_2", corrupt_ids(ids_of(verse(103, 2)["text_clean"]), 0.35, 3), 48, 3, 1.0, 7.0, 2),
        ("corrupt_36_1_5", corrupt_ids(ids_of(span_text(36, 1, 5)), 0.35, 5), 126, 5, 1.0, 6.0, 3),
        ("corrupt_55_1_4", corrupt_ids(ids_of(span_text(55, 1, 4)), 0.4, 6), 90, 6, 1.0, 6.0, 3),
    ]
    out = []
    for name, ids_path, T, seed, noise, boost, rep in recipes:
        logits = synth_logits(ids_path, T, seed=seed, noise=noise, boost=boost, rep=rep)
        lp = torch.log_softmax(torch.from_numpy(logits), dim=-1).numpy()
        transcript = cd._greedy_decode(lp)
        cands, base = cd._build_candidates(transcript)
        use_ctc = base is None or float(base.get("score", 0.0)) < cd.FALLBACK_THRESHOLD
        for tw in (0.35, 2.0):
            keep = cd.TEXT_WEIGHT
            cd.TEXT_WEIGHT = tw
            try:
                ranked = cd._ctc_rerank(lp, [dict(c) for c in cands])
            finally:
                cd.TEXT_WEIGHT = keep
            best = ranked[0]
            out.append({
                "name": name, "text_weight": tw,
                "recipe": {"ids": ids_path, "T": T, "seed": seed, "noise": noise, "boost": boost, "rep": rep},
                "transcript": transcript, "use_ctc": bool(use_ctc), "n_candidates": len(cands),
                "ranked_keys": [[c["surah"], c["ayah"], c["ayah_end"]] for c in ranked[:20]],
                "ranked_final": [float(c["final_score"]) for c in ranked[:20]],
                "ranked_text_score": [float(c.get("score") or 0.0) for c in ranked[:20]],
                "winner": [best["surah"], best["ayah"], best["ayah_end"]],
                "winner_score_raw": float(math.exp(-best["ctc_norm_loss"])),
            })
            print(name, tw, out[-1]["winner"], out[-1]["ranked_final"][:3])
    dump("e2e_textweight_cases.json.gz", out, gz=True)

    # ---------------- score_sequence known answers -----------------------------
    # inputs are the six hand cases of tests/test_scoring.py:8-59 (data), outputs
    # computed by the reference's own function.
    import importlib

    sys.modules.setdefault("shared.streaming", importlib.import_module("types").ModuleType("shared.streaming"))
    sys.modules["shared.streaming"].StreamingPipeline = object
    runner_spec = importlib.util.spec_from_file_location("_ref_runner", str(REF / "benchmark/runner.py"))
    runner = importlib.util.module_from_spec(runner_spec)
    runner_spec.loader.exec_module(runner)
    E = lambda *p: [{"surah": s, "ayah": a} for s, a in p]  # noqa: E731
    sc_in = [
        (E((103, 1), (103, 2), (103, 3)), E((103, 1), (103, 2), (103, 3))),
        (E((103, 1), (103, 2), (103, 3)), E((103, 1), (103, 3))),
        (E((1, 1)), E((2, 1))),
        (E((2, 255)), E((2, 255))),
        (E((1, 1)), []),
        (E((1, 1)), E((1, 1), (1, 2))),
        ([], E((1, 1))),
        (E((1, 1), (1, 2)), E((1, 2), (1, 1))),
    ]
    sc = [{"expected": e, "predicted": p, "out": runner.score_sequence(e, p)} for e, p in sc_in]
    em_in = [
        {"surah": 112, "ayah": 2, "ayah_end": 3, "score": 0.9811},
        {"surah": 1, "ayah": 1, "ayah_end": None, "score": 1.0},
        {"surah": 0, "ayah": 0, "ayah_end": None, "score": 0.0},
        {},
    ]
    em = [{"in": r, "out": runner._predict_to_emissions(r)} for r in em_in]
    dump("scoring_cases.json", {"score_sequence": sc, "emissions": em})


# ---------------- non-default knobs ---------------------------------------------
KNOB_DEFAULTS = {"top_text": 100, "top_span_refs": 80, "max_span": 6, "threshold": 0.80, "text_weight": 0.0,
                 "span_penalty": 0.5}
KNOB_SETS = {
    "K1": {"top_text": 1, "top_span_refs": 0, "max_span": 2},
    "K2": {"top_text": 3, "top_span_refs": 1, "max_span": 3},
    "K3": {"top_text": 5, "top_span_refs": 80, "max_span": 4},
    "K4": {"top_text": 6, "top_span_refs": 7, "max_span": 5},
    "K5": {"top_text": 127, "top_span_refs": 128, "max_span": 6},
    "K6": {"span_penalty": 0.0, "text_weight": -0.5},
    "K7": {"span_penalty": 2.0},
}
KNOB_GLOBALS = {"top_text": "TOP_TEXT", "top_span_refs": "TOP_SPAN_REFS", "max_span": "MAX_SPAN",
                "threshold": "FALLBACK_THRESHOLD", "text_weight": "TEXT_WEIGHT", "span_penalty": "SPAN_PENALTY"}
KNOB_CAP = 2048          # QV_CAND_CAP of the device (csrc/qv_common.h); the reference has no cap
KNOB_FULL_K5 = 5         # K5 cases that keep their per-candidate rerank vectors (file size)
KNOB_FULL_BELOW = 400    # ... and every case of any set whose list is no longer than this


_knob_run = None


def _knob_job(job):
    return _knob_run(job)


def knobs_section(cd, tok, db):
    """The reference at non-default TOP_TEXT / TOP_SPAN_REFS / MAX_SPAN / SPAN_PENALTY / TEXT_WEIGHT.  The reference
    reads them as module globals at call time (c2c-direct/run.py:258-309,366-379); they are set on the imported module
    and restored afterwards.  QV_GEN_JOBS=n spreads the (knob set, recipe) pairs over n forked workers."""
    import hashlib

    import torch

    torch.set_num_threads(1)

    def verse(s, a):
        return db.get_verse(s, a)

    def span_text(s, a0, a1):      # the e2e section's: ayah 1 keeps its bismillah
        return " ".join(verse(s, a)["text_clean"] for a in range(a0, a1 + 1))

    def run_text(s, a0, a1):       # a recitation of the run alone: what the reference's spans are made of
        chunk = [verse(s, a) for a in range(a0, a1 + 1)]
        first = chunk[0].get("text_clean_no_bsm") or chunk[0]["text_clean"]
        return " ".join([first] + [v["text_clean"] for v in chunk[1:]])

    def ids_of(text):
        return [int(i) for i in tok.text_to_ids(text)]

    def corrupt_ids(ids, rate, seed):   # (same recipe as the e2e section)
        r = random.Random(seed)
        out = []
        for i in ids:
            x = r.random()
            if x < rate / 2:
                continue
            if x < rate:
                out.append(r.randrange(1, 1024))
            else:
                out.append(i)
        return out

    def rcp(name, ids, T, seed, noise, boost, rep):
        return name, {"ids": ids, "T": T, "seed": seed, "noise": noise, "boost": boost, "rep": rep}

    # the nine non-empty e2e recipes, same synth_logits parameters
    t103 = ids_of(verse(103, 1)["text_clean_no_bsm"])
    recipes = dict([
        rcp("clean_1_1", ids_of(verse(1, 1)["text_clean"]), 40, 1, 1.0, 8.0, 2),
        rcp("clean_112_2", ids_of(verse(112, 2)["text_clean"]), 20, 2, 1.0, 8.0, 2),
        rcp("corrupt_103_2", corrupt_ids(ids_of(verse(103, 2)["text_clean"]), 0.35, 3), 48, 3, 1.0, 7.0, 2),
        rcp("corrupt_114_1_6", corrupt_ids(ids_of(span_text(114, 1, 6)), 0.3, 4), 150, 4, 1.0, 6.0, 2),
        rcp("corrupt_36_1_5", corrupt_ids(ids_of(span_text(36, 1, 5)), 0.35, 5), 126, 5, 1.0, 6.0, 3),
        rcp("corrupt_55_1_4", corrupt_ids(ids_of(span_text(55, 1, 4)), 0.4, 6), 90, 6, 1.0, 6.0, 3),
        rcp("noise_only", [], 63, 7, 1.0, 0.0, 1),
        rcp("long_2_255", corrupt_ids(ids_of(verse(2, 255)["text_clean"]), 0.3, 9), 251, 9, 1.0, 6.0, 2),
        rcp("tight_T_103_1", t103, 2 * len(t103) + 1, 10, 1.0, 8.0, 1),
    ])
    # lightly corrupted recitations of whole runs of 2 ... 6 ayat (rates chosen so that some pass the 0.80 gate at
    # max_span 6 and fail it under a smaller one); rep + 1 frames per token, T <= 150
    for i, (s, a0, a1, rate, rep) in enumerate([(36, 2, 3, 0.15, 2), (2, 2, 3, 0.15, 2), (103, 1, 3, 0.08, 2),
                                                (108, 1, 3, 0.15, 2), (112, 1, 4, 0.08, 2), (97, 1, 5, 0.08, 1),
                                                (95, 1, 6, 0.15, 1)]):
        ids = corrupt_ids(ids_of(run_text(s, a0, a1)), rate, 20 + i)
        T = (rep + 1) * len(ids) + 3
        assert T <= 150, (s, a0, T)
        name, r = rcp(f"run{a1 - a0 + 1}_{s}_{a0}_{a1}", ids, T, 20 + i, 1.0, 7.0, rep)
        recipes[name] = r

    sets = {"K0": dict(KNOB_DEFAULTS)}
    for k, d in KNOB_SETS.items():
        sets[k] = {**KNOB_DEFAULTS, **d}

    def run_case(job):
        kname, rname = job
        kn, r = sets[kname], recipes[rname]
        logits = synth_logits(r["ids"], r["T"], seed=r["seed"], noise=r["noise"], boost=r["boost"], rep=r["rep"])
        lp = torch.log_softmax(torch.from_numpy(logits), dim=-1).numpy()
        keep = {g: getattr(cd, g) for g in KNOB_GLOBALS.values()}
        for k, g in KNOB_GLOBALS.items():
            setattr(cd, g, kn[k])
        try:
            transcript = cd._greedy_decode(lp)
            cands, base = cd._build_candidates(transcript)
            use_ctc = base is None or float(base.get("score", 0.0)) < cd.FALLBACK_THRESHOLD
            ranked = cd._ctc_rerank(lp, cands)      # recorded on gate-pass cases too, like the e2e section
        finally:
            for g, v in keep.items():
                setattr(cd, g, v)
        if use_ctc and ranked:
            best, src = ranked[0], "ctc"
            score = math.exp(-best["ctc_norm_loss"])
        else:
            best, src, score = base, "text", float(base["score"])
        out = {
            "set": kname, "name": rname, "transcript": transcript,
            "base": [base["surah"], base["ayah"], base.get("ayah_end"), float(base["score"])],
            "use_ctc": bool(use_ctc), "n_candidates": len(cands),
            "cand_keys": [[c["surah"], c["ayah"], c["ayah_end"]] for c in cands],
            "cand_scores": [float(c.get("score") or 0.0) for c in cands],
            "ctc_loss": [(float(c["ctc_loss"]) if math.isfinite(c["ctc_loss"]) else None) for c in cands],
            "ctc_len": [int(c["ctc_len"]) for c in cands],
            "final_score": [(float(c["final_score"]) if math.isfinite(c["final_score"]) else None) for c in cands],
            "ranked_keys": [[c["surah"], c["ayah"], c["ayah_end"]] for c in ranked[:20]],
            "ranked_final": [float(c["final_score"]) for c in ranked[:20]],
            "winner": [best["surah"], best["ayah"], best.get("ayah_end") or best["ayah"]],
            "source": src, "winner_score_raw": float(score),
        }
        print(kname, rname, out["base"], "use_ctc", use_ctc, "ncand", len(cands), out["winner"], src, flush=True)
        return out

    jobs = [(k, r) for k in sets for r in recipes]
    n_jobs = int(os.getenv("QV_GEN_JOBS", "1"))
    if n_jobs > 1:
        import multiprocessing as mp

        global _knob_run
        _knob_run = run_case            # forked workers inherit it
        with mp.get_context("fork").Pool(n_jobs) as pool:
            raw = pool.map(_knob_job, jobs, chunksize=1)
    else:
        raw = [run_case(j) for j in jobs]
    return knobs_encode(sets, recipes, raw, dict(db._ref_to_idx))


def knobs_encode(sets, recipes, raw, verse_index):
    """Check the conditions the fixture set has to meet and write it.  Layout: "sets" (the six knobs of every set),
    "recipes" (synth_logits parameters + the reference's transcript), "defaults" (the outcome at the default knobs: base,
    winner, candidate count and a digest of the candidate keys) and "cases".  A case's candidate list is stored by
    column ("cand": the first verse as its index in mushaf order, 0 ... 6235, each as the difference from the one before
    it; the number of ayat; the text score -- this spelling is what keeps the file small); K6 and K7 build the list of
    the default knobs, so K7 points at K6's ("cand_of").  The per-candidate rerank vectors ("ctc_loss", "ctc_len", "final_score") are kept for every case
    of at most KNOB_FULL_BELOW candidates and for KNOB_FULL_K5 cases of K5 (the clipped ones first); all the others keep
    the ranking's top 20 and the winner."""
    import hashlib

    def digest(keys):
        return hashlib.sha1(json.dumps(keys, separators=(",", ":")).encode()).hexdigest()[:16]

    def span_of(base):
        return 1 if base[2] is None else base[2] - base[1] + 1

    by = {(c["set"], c["name"]): c for c in raw}
    for c in raw:       # the transcript does not depend on the knobs
        assert c["transcript"] == by[("K0", c["name"])]["transcript"]
    defaults = {n: {"base": by[("K0", n)]["base"], "winner": by[("K0", n)]["winner"], "source": by[("K0", n)]["source"],
                    "n_candidates": by[("K0", n)]["n_candidates"], "cand_digest": digest(by[("K0", n)]["cand_keys"])}
                for n in recipes}
    cases = [c for c in raw if c["set"] != "K0"]

    # ---- conditions on the set (asserted again by tests/test_oracle_knobs.py)
    for m in range(2, 7):
        at_m = [c for c in cases if sets[c["set"]]["max_span"] == m]
        assert any(span_of(c["base"]) == m for c in at_m), m
        assert any(span_of(c["base"]) < m for c in at_m), m
    assert any(c["base"][:3] != defaults[c["name"]]["base"][:3] for c in cases if sets[c["set"]]["max_span"] < 6)
    for field in ("top_text", "top_span_refs", "max_span", "span_penalty", "text_weight"):
        moved = [c for c in cases if sets[c["set"]][field] != KNOB_DEFAULTS[field]]
        assert any(digest(c["cand_keys"]) != defaults[c["name"]]["cand_digest"] or
                   (c["winner"], c["source"]) != (defaults[c["name"]]["winner"], defaults[c["name"]]["source"])
                   for c in moved), field
    k5 = sorted((c for c in cases if c["set"] == "K5"), key=lambda c: -c["n_candidates"])
    print("K5 candidate counts:", {c["name"]: c["n_candidates"] for c in k5})
    assert sum(c["n_candidates"] > KNOB_CAP for c in k5) >= 3
    assert any(KNOB_CAP < c["n_candidates"] <= KNOB_CAP + 100 for c in k5)
    assert any(KNOB_CAP - 100 <= c["n_candidates"] <= KNOB_CAP for c in k5)

    # the K5 cases that keep their rerank vectors: the one nearest above the cap, the largest, the one nearest below it,
    # then further clipped ones
    over = [c for c in k5 if c["n_candidates"] > KNOB_CAP]
    under = [c for c in k5 if c["n_candidates"] <= KNOB_CAP]
    pick = [over[-1]["name"], over[0]["name"], under[0]["name"]] + [c["name"] for c in over[1:-1]]
    full_k5 = set(pick[:KNOB_FULL_K5])

    out_cases = []
    for c in cases:
        d = {k: c[k] for k in ("set", "name", "base", "use_ctc", "n_candidates", "ranked_keys", "ranked_final",
                               "winner", "source", "winner_score_raw")}
        if c["set"] == "K7":
            assert (c["cand_keys"], c["cand_scores"]) == (by[("K6", c["name"])]["cand_keys"], by[("K6", c["name"])]["cand_scores"])
            d["cand_of"] = "K6"
        else:
            start = [verse_index[(k[0], k[1])] for k in c["cand_keys"]]
            d["cand"] = {"start_delta": start[:1] + [b - a for a, b in zip(start, start[1:])],
                         "span": [k[2] - k[1] + 1 for k in c["cand_keys"]], "score": c["cand_scores"]}
        if c["n_candidates"] <= KNOB_FULL_BELOW or (c["set"] == "K5" and c["name"] in full_k5):
            # ctc_loss is a float32 (F.ctc_loss), stored in its shortest float32 spelling: np.float32(stored) is the loss
            loss = [None if x is None else float(str(np.float32(x))) for x in c["ctc_loss"]]
            assert [None if x is None else float(np.float32(x)) for x in loss] == c["ctc_loss"]
            d["rerank"] = {"ctc_loss": loss, "ctc_len": c["ctc_len"], "final_score": c["final_score"]}
        out_cases.append(d)
    dump("knob_cases.json.gz", {
        "sets": {k: v for k, v in sets.items() if k != "K0"},
        "recipes": {n: {"recipe": r, "transcript": by[("K0", n)]["transcript"]} for n, r in recipes.items()},
        "defaults": defaults, "cases": out_cases}, gz=True)
    size = (HERE / "knob_cases.json.gz").stat().st_size
    assert size < (HERE / "retrieval_cases.json.gz").stat().st_size, size


if __name__ == "__main__":
    main()
