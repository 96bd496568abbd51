"""The opt-in matching window of 2,048 normalised characters (Engine(max_transcript=2048): the wide set of post-logits
kernels -- 17..32-word LCS patterns, the span pass over half a wave per walk) on the MI355X, against the reference's own
long fixtures and against the CPU oracle, which has no length limit and reproduces those fixtures
(tests/test_oracle_long_transcript.py).  Every integer and fp64 score is compared with ==; CTC scores with the relative
1e-3 of tests/test_gpu_postlogits.py.  The default window (1,024) does not move: it still withholds what the wide engine
matches, and below 1,024 characters both engines reproduce the reference fixtures alike."""

import ctypes as C
import gzip
import json
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from synth import BLANK, VOCAB, hash_noise, synth_logits

pytestmark = pytest.mark.gpu

T_LONG = 763          # qv_frames_for_samples(976000): the 61 s an engine can be created for


@pytest.fixture(scope="module")
def wide():
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=False, max_batch=16, max_samples=976000, max_transcript=2048)
    assert eng.max_transcript == 2048 and eng.frames_for(976000) == T_LONG
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def default_engine():
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=False, max_batch=16, max_samples=976000)
    assert eng.max_transcript == 1024
    yield eng
    eng.close()


@pytest.fixture(params=["default", "wide"])
def either(request, default_engine, wide):
    return default_engine if request.param == "default" else wide


@pytest.fixture(scope="module")
def long_cases(golden_dir):
    return json.loads((golden_dir / "longtx_cases.json").read_text(encoding="utf-8"))


@pytest.fixture(scope="module")
def tracker_oracle(oracle):
    from oracle.tracker_ref import TrackerOracle

    return TrackerOracle(oracle)


@pytest.fixture(scope="module")
def mv_oracle(oracle):
    from oracle.tracker_ref import MatchVerseOracle

    return MatchVerseOracle(oracle)


# ------------------------------------------------------------------ inputs ---------------------------------------------

def oracle_map(fn, jobs):
    """the oracle's answers for a list of inputs, several at a time: one long text costs it 4-6 s, all of it inside its C
    library (no shared state, called without the interpreter lock)"""
    with ThreadPoolExecutor(max_workers=12) as ex:
        return list(ex.map(fn, jobs))


def glued_text(o, rng, lo, hi, alphabet):
    """consecutive ayat glued until the text is long enough, some words dropped, ~10 % of the characters replaced (one of
    the replacements is outside the verse alphabet) -- the recipe of test_track_match_vs_oracle_random, stretched to
    lo..hi characters."""
    target = rng.randrange(lo, hi + 1)
    while True:
        v = rng.randrange(6236 - 40)
        words, k = [], 0
        while sum(len(w) + 1 for w in words) < target + 200 and k < 40:
            words += o.verse_text(v + k).split()
            k += 1
        words = [w for w in words if rng.random() > 0.05]
        chars = list(" ".join(words))
        for i in range(len(chars)):
            if chars[i] != " " and rng.random() < 0.10:
                chars[i] = rng.choice(alphabet + ["x"])          # "x": outside the verse alphabet
        t = " ".join("".join(chars).split())[:target].strip()
        if lo <= len(t) <= hi:
            return t, v


def dense_logprobs(ids, T, seed, noise=1.0, boost=12.0):
    """float32 [T, 1025] log-probs whose greedy path is `ids` with a blank ONLY between equal neighbours (CTC needs no
    other): one frame per token, blank padding behind.  hash_noise is bounded by 3.45, so a boost of 12 decides every
    frame."""
    path = []
    for tok in ids:
        if path and path[-1] == int(tok):
            path.append(BLANK)
        path.append(int(tok))
    assert len(path) <= T, (len(path), T)
    path += [BLANK] * (T - len(path))
    lg = hash_noise((T, VOCAB), seed) * np.float32(noise)
    lg[np.arange(T), np.asarray(path)] += np.float32(boost)
    return torch.log_softmax(torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32)), dim=-1)


def corrupted(ids, rate, seed):
    rng = np.random.default_rng(seed)
    return [int(rng.integers(1, 1024)) if rng.random() < rate else int(t) for t in ids]


@pytest.fixture(scope="module")
def hot_cases(oracle):
    """(name, log-probs [T, 1025], frames) -- six long recitations and two short ones, and the oracle's answer for each"""
    a = oracle.token_ids(oracle.verse_index(2, 282), 5).tolist()          # 2:282-286, 618 tokens
    b = oracle.token_ids(oracle.verse_index(5, 1), 6).tolist()            # 5:1-6
    cases = [("2:282-286", dense_logprobs(a, T_LONG, 11), T_LONG),
             ("5:1-6", dense_logprobs(b, T_LONG, 12), T_LONG),
             ("2:282-286 20% replaced", dense_logprobs(corrupted(a, 0.20, 5), T_LONG, 13), T_LONG),
             ("5:1-6 35% replaced", dense_logprobs(corrupted(b, 0.35, 2), T_LONG, 14), T_LONG),
             ("2:282-286 50% replaced", dense_logprobs(corrupted(a, 0.50, 3), T_LONG, 15), T_LONG),
             # (another 20 % draw stays just above the gate, 0.803 against the threshold of 0.80: the text branch decides)
             ("2:282-286 20% replaced, gate passes", dense_logprobs(corrupted(a, 0.20, 4), T_LONG, 13), T_LONG)]
    for (s, ay), T, seed in (((112, 1), 24, 16), ((1, 2), 40, 17)):       # W = 1 next to W = 32 in one batch
        ids = oracle.token_ids(oracle.verse_index(s, ay), 1).tolist()
        cases.append((f"{s}:{ay}", torch.log_softmax(torch.from_numpy(synth_logits(ids, T, seed=seed, noise=1.0, boost=8.0, rep=2)), -1), T))
    want = oracle_map(lambda c: oracle.predict_logprobs(c[1][: c[2]].numpy()), cases)
    return cases, want


def batch_of(cases):
    t_max = max(T for _, _, T in cases)
    batch = torch.full((len(cases), t_max, VOCAB), -50.0)
    for i, (_, lp, T) in enumerate(cases):
        batch[i, :T] = lp[:T]
    return batch.cuda().contiguous(), [T for _, _, T in cases]


def check_hot(got, want, tag):
    """the comparisons and tolerances of test_fuzz_batched_path_against_the_oracle"""
    assert got["greedy_ids"] == want["greedy_ids"], tag
    assert got["transcript"] == want["transcript"], tag
    assert (got["surah"], got["ayah"], got["ayah_end"], got["source"]) == (
        want["surah"], want["ayah"], want["ayah_end"], want["source"]), (tag, got, want)
    assert want["source"] is not None, tag
    assert got["use_ctc"] == want["use_ctc"], tag
    if want["use_ctc"]:
        assert got["n_candidates"] == want["n_candidates"], tag
    if want["source"] == "text":
        assert got["score"] == want["score_raw"], tag
    else:
        assert abs(got["score"] - want["score_raw"]) <= 1e-3 * max(want["score_raw"], 1e-3), tag


# ------------------------------------------------------------------ the wide window -------------------------------------

def test_run_on_full_transcript_equals_the_reference_beyond_1024_characters(wide, long_cases):
    """tests/golden/longtx_cases.json: the reference's own run_on_full_transcript on 1,378 and 1,556 characters -- the whole
    emission lists, scores included (the default window answers the second one differently: it matches a front window)."""
    from offline_tarteel_amd.streaming import StreamingPipeline

    assert [c["chars"] for c in long_cases] == [1378, 1556]
    pipe = StreamingPipeline(wide)
    for c in long_cases:
        assert pipe.run_on_full_transcript("x.wav", lambda p, t=c["text"]: t) == c["emissions"], c["chars"]


def test_match_verse_vs_oracle_on_long_texts(wide, oracle, mv_oracle):
    """qv_match_verse (full scan, fragment scores with windows on either side, hint scores, spans up to 3 and 8 ayat) on 40
    seeded texts of 1,025..2,048 characters: verse, span, word count equal, fp64 score ==."""
    rng = random.Random(2048)
    alphabet = [ch for ch in oracle.alphabet if ch != " "]
    lengths, jobs = [], []
    for k in range(40):
        lo, hi = ((1025, 1100), (1100, 1600), (1600, 2000), (2000, 2048))[k % 4]
        text, v = glued_text(oracle, rng, lo, hi, alphabet)
        assert 1025 <= len(text) <= 2048
        lengths.append(len(text))
        s, a = int(oracle.surah[v]), int(oracle.ayah[v])
        hint = (None, (s, a - 1) if a > 1 else (s, a), None, (s, a))[k % 4]
        jobs += [(k, text, hint, 3), (k, text, hint, 8)]
    want = oracle_map(lambda j: mv_oracle.match_verse(j[1], threshold=0.0, max_span=j[3], hint=j[2]), jobs)
    for (k, text, hint, max_span), w in zip(jobs, want):
        r = wide.match_verse(text, threshold=0.0, max_span=max_span, hint=hint)
        assert (r["verse"], r["span"], r["n_words"]) == (w["verse"], w["span"], w["n_words"]), (k, len(text), hint, max_span, r, w)
        assert r["score"] == w["score"], (k, len(text), hint, max_span, r["score"], w["score"])
    assert {(n + 63) // 64 for n in lengths} >= {17, 32} and len({(n + 63) // 64 for n in lengths}) >= 8


def test_track_match_vs_oracle_on_long_texts(wide, tracker_oracle):
    """qv_tracker_match on 80 seeded texts of 1,025..2,048 characters with the `last` choices of the short random test, plus
    one repeated letter and real text cut to the lengths around the word boundaries of the pattern: verse, variant, word
    count equal, fp64 score ==."""
    rng = random.Random(7)
    o = tracker_oracle.o
    alphabet = [ch for ch in o.alphabet if ch != " "]
    texts, lasts = [], []
    for k in range(80):
        lo, hi = ((1025, 1100), (1100, 1600), (1600, 2000), (2000, 2048))[k % 4]
        t, v = glued_text(o, rng, lo, hi, alphabet)
        texts.append(t)
        s, a = int(o.surah[v]), int(o.ayah[v])
        lasts.append(rng.choice([None, (s, a - 1) if a > 1 else None, (s, a), (114, 6), (3, 999)]))
    real = " ".join(o.verse_text(o.verse_index(2, 270) + j) for j in range(17))          # 2:270-286
    assert len(real) >= 2048
    starts = [0] + [i + 1 for i, ch in enumerate(real) if ch == " "]
    for n in (1024, 1025, 1088, 1089, 1536, 2047, 2048):
        cut = next(real[i: i + n] for i in starts if real[i + n - 1] != " ")     # exactly n characters from a word start
        assert len(cut) == n and cut == cut.strip()
        texts += ["ا" * n, cut]
        lasts += [None, (2, 281)]
    assert all(len(t) <= 2048 for t in texts) and sum(len(t) > 1024 for t in texts) >= 90
    got = wide.track_match(texts, lasts)
    want = oracle_map(lambda j: tracker_oracle.best_raw(*j), list(zip(texts, lasts)))
    for t, last, g, w in zip(texts, lasts, got, want):
        assert (g is None) == (w is None), (len(t), t[:40])
        if g:
            assert (g["verse"], g["variant"], g["n_words"]) == (w[0], w[1], w[2]), (len(t), t[:40], g, w)
            assert g["score"] == w[3], (len(t), t[:40], g["score"], w[3])


def test_track_match_capacity_of_the_wide_window(wide, tracker_oracle):
    """2,049 codes: the binding matches the longest whole-word front window of 2,048, the C entry points still refuse."""
    from offline_tarteel_amd.engine import QvTrackMatch, front_window

    o = tracker_oracle.o
    from oracle.oracle import normalize_arabic

    # (normalised first, as match_verse does itself: the window is cut from the NORMALISED text, and the verse texts
    # carry a few marks the normaliser drops)
    words = normalize_arabic(" ".join(o.verse_text(o.verse_index(2, 270) + j) for j in range(17)))         # 2:270-286
    assert len(words) > 2049 and normalize_arabic(words) == words
    win = front_window(words, 2048)
    assert 1024 < len(win) <= 2048 and words.startswith(win) and words[len(win)] == " "
    got, want = wide.track_match([words])[0], wide.track_match([win])[0]
    assert got == want and got is not None
    w = tracker_oracle.best_raw(win, None)
    assert (got["verse"], got["variant"], got["n_words"], got["score"]) == w
    assert wide.match_verse(words) == wide.match_verse(win)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nw, bonus, out = np.array([1], np.int32), np.array([-1], np.int32), (QvTrackMatch * 1)()
    for n, rc_want in ((2048, 0), (2049, 4)):                                 # QV_ERR_CAPACITY = 4
        codes, off = np.ones(n, np.uint8), np.array([0, n], np.int32)
        assert wide.lib.qv_tracker_match(wide.h, p(codes), p(off), p(nw), p(bonus), 1, C.cast(out, C.c_void_p), None) == rc_want, n
        bv, bb = np.zeros(3, np.int32), np.zeros(3, np.float64)
        st, sp, sc = C.c_int32(), C.c_int32(), C.c_double()
        assert wide.lib.qv_match_verse(wide.h, p(codes), n, 0, p(bv), p(bb), 3, C.byref(st), C.byref(sp), C.byref(sc), None) == rc_want, n


def test_hot_path_matches_long_transcripts_the_default_window_withholds(wide, default_engine, hot_cases):
    """decode -> trigram -> match_verse -> search -> pass 3 -> candidates -> rerank -> decision on 61 s worth of frames whose
    greedy paths decode to more than 1,024 characters: clean recitations (text branch) and corrupted ones (CTC branch),
    two short utterances in the same batch (W = 1 next to W = 32), against the oracle.  The default engine still returns
    surah 0 with the TRUNCATED flag for the long ones and the same answers for the short ones."""
    from offline_tarteel_amd.engine import FLAG_TRUNC

    cases, want = hot_cases
    for (name, _, T), w in zip(cases, want):
        print(name, "chars", len(w["transcript"]), "source", w["source"], "use_ctc", w.get("use_ctc"), "n_cand", w.get("n_candidates"),
              "score", w.get("score_raw"))
    n_long = 6
    for (name, _, _), w in zip(cases[:n_long], want):
        assert 1024 < len(w["transcript"]) <= 2048, (name, len(w["transcript"]))
    assert [w["use_ctc"] for w in want[:n_long]] == [False, False, True, True, True, False]
    assert (want[0]["surah"], want[0]["ayah"], want[0]["ayah_end"]) == (2, 282, 286)
    assert all(len(w["transcript"]) <= 64 for w in want[n_long:])
    lp, frames = batch_of(cases)
    res = wide.decode_retrieve_rerank(lp, frames)
    for (name, _, _), g, w in zip(cases, res, want):
        print(name, "got", g["surah"], g["ayah"], g["ayah_end"], g["source"], g["score"], g["n_candidates"], g["flags"])
    for (name, _, _), g, w in zip(cases, res, want):
        assert not g["flags"] & FLAG_TRUNC, name
        check_hot(g, w, name)
    res = default_engine.decode_retrieve_rerank(lp, frames)
    for (name, _, _), g, w in zip(cases[:n_long], res, want):
        assert g["greedy_ids"] == w["greedy_ids"], name
        assert g["flags"] & FLAG_TRUNC and (g["surah"], g["ayah"], g["source"]) == (0, 0, None), (name, g)
    for (name, _, _), g, w in zip(cases[n_long:], res[n_long:], want[n_long:]):
        assert not g["flags"] & FLAG_TRUNC, name
        check_hot(g, w, name)


@pytest.fixture(scope="module")
def readout_case(oracle):
    """2:282 alone (298 tokens, 597 states) with 35 % of its ids replaced: fails the gate, fits the default window, and every
    candidate near it is a target of more than 384 states"""
    ids = oracle.token_ids(oracle.verse_index(2, 282), 1).tolist()
    assert 384 < 2 * len(ids) + 1 <= T_LONG
    return ("2:282 35% replaced", dense_logprobs(corrupted(ids, 0.35, 7), T_LONG, 21), T_LONG)


def test_member_readouts_of_long_targets_against_torch(either, oracle, hot_cases, readout_case):
    """k_ctc<true, .> on the hot path: one alpha recursion per leader, and the losses of its members read off the same
    alpha row at their own lengths.  Every entry of the reranked rows' n-best lists (k = 32): the token count is the
    table's, the loss is F.ctc_loss of that token list within 1e-3 max(1, |want| / 100) -- targets of more than 384 and of
    more than 512 states among them, which the per-target entry point reaches only through k_ctc_debug."""
    cases = hot_cases[0] + [readout_case]
    lp, frames = batch_of(cases)
    res = either.decode_retrieve_rerank(lp, frames, want_text=False)
    info, ent = either.nbest_raw(batch=len(cases), k=32)
    n = n384 = n512 = 0
    worst = 0.0
    for b, ((name, x, T), r) in enumerate(zip(cases, res)):
        if r["source"] != "ctc":
            continue
        rows = ent[b, : int(info[b]["n_entries"])]
        id_lists = [either.tables.token_ids(int(e["start_verse"]), int(e["span"])).tolist() for e in rows]
        want = oracle.ctc_loss_torch(x[:T].numpy(), id_lists)
        for e, ids, w in zip(rows, id_lists, want):
            assert int(e["n_tokens"]) == len(ids) and 2 * len(ids) + 1 <= T, (name, int(e["cand_index"]))
            d = abs(float(e["ctc_loss"]) - float(w))
            assert d <= 1e-3 * max(1.0, abs(float(w)) / 100), (name, int(e["cand_index"]), len(ids), float(e["ctc_loss"]), float(w))
            worst = max(worst, d / max(1.0, abs(float(w)) / 100))
            n, n384, n512 = n + 1, n384 + (2 * len(ids) + 1 > 384), n512 + (2 * len(ids) + 1 > 512)
    print(f"window {either.max_transcript}: {n} entries compared, {n384} of more than 384 states, {n512} of more than 512; "
          f"largest scaled distance {worst:.3g}")
    assert n384 >= 10 and n512 >= 1


def retrieve_vs_oracle(eng, oracle, t, want):
    r = eng.debug_retrieve(t)
    (cs, cp, sc, m), mv = want
    assert (r["base_start"], r["base_span"], r["base_score"]) == (m.start, m.span, m.score), len(t)
    assert r["cand_start"].tolist() == cs.tolist() and r["cand_span"].tolist() == cp.tolist(), len(t)
    assert r["cand_score"].tolist() == sc.tolist(), len(t)
    # (the oracle keeps the runners-up rounded to 3 places, as the reference does; the device rounds where it consumes them)
    run = [(int(eng.tables.surah[i]), int(eng.tables.ayah[i]), round(float(s), 3)) for i, s in zip(r["runner_idx"], r["runner_score"])]
    assert run == [(s, a, float(x)) for s, a, x in mv["runners_up"]], len(t)
    return r


def test_debug_retrieve_vs_oracle_on_long_transcripts(wide, oracle, hot_cases, long_cases):
    """base match, candidate list in order with its text scores, runners-up: == the oracle's match_verse /
    build_candidates, for two of the hot path's long transcripts and the two long fixtures"""
    _, want = hot_cases
    from oracle.oracle import normalize_arabic

    # (the device entry takes normalised transcripts -- what greedy decode always produces; the fixtures' texts are raw)
    texts = [want[0]["transcript"], want[3]["transcript"], normalize_arabic(long_cases[0]["text"]), normalize_arabic(long_cases[1]["text"])]
    assert all(len(t) > 1024 and normalize_arabic(t) == t for t in texts)
    answers = oracle_map(lambda j: j[0](j[1]), [(f, t) for t in texts for f in (oracle.build_candidates, oracle.match_verse)])
    for i, t in enumerate(texts):
        retrieve_vs_oracle(wide, oracle, t, (answers[2 * i], answers[2 * i + 1]))
    with pytest.raises(Exception):
        wide.debug_retrieve("ا" * 2049)


def test_span_pass_variants_agree_on_the_wide_engine(wide, oracle, hot_cases, long_cases):
    """QVERSE_SPANS: one walk per span (k_spans, carry per code) against one walk per start verse (k_spans2, carry per
    chunk), both with the 17..32 pattern words spread over 32 lanes: identical retrieval, hot-path results and
    match_verse answers (spans up to 8) on the long cases."""
    cases, want = hot_cases
    from oracle.oracle import normalize_arabic

    texts = [w["transcript"] for w in want[:6]] + [normalize_arabic(c["text"]) for c in long_cases]
    rng = random.Random(5)
    alphabet = [ch for ch in oracle.alphabet if ch != " "]
    texts += [normalize_arabic(glued_text(oracle, rng, lo, hi, alphabet)[0]) for lo, hi in ((1025, 1088), (1089, 1300), (1500, 1600), (1985, 2048))]
    assert all(1024 < len(t) <= 2048 for t in texts)
    lp, frames = batch_of(cases)
    got = {}
    try:
        for var in (0, 1):
            wide.kernel_variant(2, var)
            got[var] = ([wide.debug_retrieve(t) for t in texts], wide.decode_retrieve_rerank(lp, frames),
                        [wide.match_verse(t, threshold=0.0, max_span=8) for t in texts])
    finally:
        wide.kernel_variant(2, -1)
    for t, a, c in zip(texts, got[0][0], got[1][0]):
        assert (a["base_start"], a["base_span"], a["base_score"]) == (c["base_start"], c["base_span"], c["base_score"]), len(t)
        assert a["cand_start"].tolist() == c["cand_start"].tolist() and a["cand_span"].tolist() == c["cand_span"].tolist(), len(t)
        assert a["cand_score"].tolist() == c["cand_score"].tolist(), len(t)
    assert got[0][1] == got[1][1]
    assert got[0][2] == got[1][2] and all(g is not None for g in got[1][2])
    # the winners of the long texts are spans: the pass under test decided them
    assert sum(a["base_span"] > 1 for a in got[1][0]) >= 6


# ------------------------------------------------------------------ both windows, same answers below 1,024 -------------

def lp_of(recipe):
    lg = synth_logits(recipe["ids"], recipe["T"], seed=recipe["seed"], noise=recipe["noise"], boost=recipe["boost"], rep=recipe["rep"])
    return torch.log_softmax(torch.from_numpy(lg), dim=-1)


def test_e2e_fixtures_on_either_window(either, golden_dir):
    e2e_cases = json.load(gzip.open(golden_dir / "e2e_cases.json.gz"))
    lps = [lp_of(c["recipe"]) for c in e2e_cases]
    t_max = max(x.shape[0] for x in lps)
    batch = torch.full((len(lps), t_max, 1025), -50.0)
    for b, x in enumerate(lps):
        batch[b, : x.shape[0]] = x
    rows = []
    for lo in range(0, len(lps), either.max_batch):
        rows += either.decode_retrieve_rerank(batch[lo: lo + either.max_batch].cuda().contiguous(),
                                              [x.shape[0] for x in lps[lo: lo + either.max_batch]])
    assert len(rows) == len(e2e_cases)
    for c, r in zip(e2e_cases, rows):
        g = c["result"]
        assert r["greedy_ids"] == c["greedy_ids"], c["name"]
        assert r["transcript"] == c["transcript"], c["name"]
        assert (r["surah"], r["ayah"], r["ayah_end"], r["source"]) == (g["surah"], g["ayah"], g["ayah_end"], g["source"]), c["name"]
        if g["source"] == "text":
            assert r["score"] == g["score_raw"], c["name"]
        elif g["source"] == "ctc":
            assert abs(r["score"] - g["score_raw"]) <= 1e-3 * max(g["score_raw"], 1e-3), c["name"]
            assert round(r["score"], 4) == g["score"] or abs(r["score"] - g["score_raw"]) < 1e-6, c["name"]
        if "use_ctc" in c:
            assert r["use_ctc"] == c["use_ctc"], c["name"]
            if c["use_ctc"]:
                assert r["n_candidates"] == c["n_candidates"], c["name"]


def test_retrieval_fixtures_on_either_window(either, golden_dir):
    from oracle.oracle import normalize_arabic

    ret_cases = json.load(gzip.open(golden_dir / "retrieval_cases.json.gz"))
    checked = 0
    for c in ret_cases:
        t = c["transcript"]
        if normalize_arabic(t) != t or c["name"] == "garbage_40":
            continue  # device entry takes normalised transcripts (greedy decode output always is)
        r = either.debug_retrieve(t)
        g = c["match"]
        key = either.tables.key_of(r["base_start"], r["base_span"])
        want_end = g["ayah_end"] if g["ayah_end"] is not None else g["ayah"]
        assert key == (g["surah"], g["ayah"], want_end), c["name"]
        assert r["base_score"] == g["score"], c["name"]
        run = [[int(either.tables.surah[i]), int(either.tables.ayah[i]), round(float(s), 3)]
               for i, s in zip(r["runner_idx"], r["runner_score"])]
        assert run == g["runners_up"], c["name"]
        keys = [list(either.tables.key_of(int(a), int(b))) for a, b in zip(r["cand_start"], r["cand_span"])]
        assert keys == c["candidates"], c["name"]
        assert r["cand_score"].tolist() == c["cand_scores"], c["name"]
        checked += 1
    assert checked >= 18


def test_tracker_fixtures_on_either_window(either, golden_dir):
    from offline_tarteel_amd.streaming import StreamingPipeline

    with gzip.open(golden_dir / "tracker_cases.json.gz", "rt", encoding="utf-8") as f:
        cases = json.load(f)
    cs = cases["best_match"]
    got = either.track_match([c["text"] for c in cs], [tuple(c["last"]) if c["last"] else None for c in cs])
    assert len(got) == len(cs) >= 300
    for c, g in zip(cs, got):
        m = g if c["text"].strip() and not (c["streaming"] and len(c["text"].split()) < 2) and g is not None \
            and g["score"] >= (0.4 if c["streaming"] else 0.3) else None
        w = c["match"]
        assert (m is None) == (w is None), c["text"]
        if m:
            assert (m["surah"], m["ayah"], m["n_words"]) == (w["surah"], w["ayah"], w["n_words"]), c["text"]
            assert m["score"] == w["score"], (c["text"], m["score"], w["score"])
    pipe = StreamingPipeline(either)
    for c in cases["run_on_text"]:
        assert pipe.run_on_text(c["snapshots"]) == c["emissions"]


def test_full_transcript_fixtures_on_either_window(either, golden_dir):
    from offline_tarteel_amd.streaming import StreamingPipeline

    with gzip.open(golden_dir / "fulltx_cases.json.gz", "rt", encoding="utf-8") as f:
        fx = json.load(f)
    for c in fx["match"]:
        r = either.match_verse(c["text"], max_span=8, hint=tuple(c["hint"]) if c["hint"] else None)
        w = c["result"]
        assert (r is None) == (w is None), c["text"]
        if r:
            for k in ("surah", "ayah", "ayah_end", "score", "n_words"):
                assert r[k] == w[k], (c["text"], k, r[k], w[k])
    pipe = StreamingPipeline(either)
    for c in fx["full"]:
        assert pipe.run_on_full_transcript("x.wav", lambda p, t=c["text"]: t) == c["emissions"], c["text"]
