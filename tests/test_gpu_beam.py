"""Verse-constrained CTC prefix beam search (csrc/qv_beam.hip, k_trie_beam; include/qverse.h qv_beam_decode / qv_beam_batch)
on the MI355X.

The reference of every figure is tests/beam_ref.py (pinned by tests/test_beam_host.py against torch's CTC loss and a brute-force
sum): the kernel's node list, its order and every integer field must equal the restatement's exactly, the three scores within
1e-7.  That bound is derived, not measured: a frame costs one add and one lae on values of magnitude <= 766 x 30 (the inputs keep
their log-probs above -30, asserted), about 4 ulp of 3.6e-12; over at most 766 frames about 1.1e-8, passed on through lae with
weights that sum to 1; asserted with a 10x margin.  A comparison of node lists is only meaningful where the restatement's own
decisions are not within round-off of a tie: every case must have a prune margin and a final gap of at least 1e-5 (asserted on
the CPU first; a case under that is a bad input and fails).  Inputs use continuous noise: synth.hash_noise is quantised and
would manufacture exact ties."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import beam_ref as R
from synth import BLANK, VOCAB, frame_path, synth_audio

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-7
MIN_MARGIN = 1e-5
# (verse, span, T, noise, boost, W)
CASES = [(0, 1, 40, 1, 6, 8), (1, 1, 40, 1, 2, 8), (261, 1, 300, 1, 4, 8), (2, 3, 120, 1, 3, 4), (100, 2, 96, 2, 3, 16),
         (6230, 1, 30, 1, 1, 32), (50, 1, 12, 1, 3, 8), (10, 1, 64, 3, 0, 64), (10, 1, 1, 1, 0, 8)]


def make_lp(tables, verse, span, T, noise, boost):
    lg = np.random.default_rng(1000 + verse).standard_normal((T, VOCAB)).astype(np.float32) * np.float32(noise)
    if boost:
        lg[np.arange(T), frame_path(tables.token_ids(verse, span), T, 2)] += np.float32(boost)
    x = lg.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))).astype(np.float32)


@pytest.fixture(scope="module")
def eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=16, max_samples=480000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(eng):
    return eng.tables


@pytest.fixture(scope="module")
def trie3(tables):
    return R.Trie.from_tables(tables, 3)


@pytest.fixture(scope="module")
def case_lp(tables):
    return [make_lp(tables, *c[:5]) for c in CASES]


@pytest.fixture(scope="module")
def case_ref(trie3, case_lp):
    return [R.beam_search(trie3, lp, c[5], BLANK) for c, lp in zip(CASES, case_lp)]


def batch_of(lps, pad=0.0, extra=0):
    t_max = max(max(len(x) for x in lps), 1) + extra
    out = np.full((len(lps), t_max, VOCAB), pad, np.float32)
    for b, x in enumerate(lps):
        out[b, : len(x)] = x
    return torch.from_numpy(out).cuda().contiguous(), [len(x) for x in lps]


def check_margins(ref, tag):
    print(f"{tag}: prune_margin {ref['prune_margin']:.3e} final_gap {ref['final_gap']:.3e} max_candidates {ref['max_candidates']}")
    assert ref["prune_margin"] >= MIN_MARGIN and ref["final_gap"] >= MIN_MARGIN, (tag, ref["prune_margin"], ref["final_gap"])


def check_row(info, ent, ref, trie, tables, T, k, tag):
    """one row of a qv_beam_decode call against the restatement: integers exactly, scores within SCORE_TOL"""
    hyps = ref["hyps"][:k]
    assert (int(info["n_entries"]), int(info["t_frames"]), int(info["max_candidates"]), int(info["reserved"])) == \
        (len(hyps), T, ref["max_candidates"], 0), tag
    assert ent["node"][: len(hyps)].tolist() == [h[0] for h in hyps], tag
    worst = 0.0
    for e, (node, tot, pb, pnb) in zip(ent, hyps):
        want = R.entry_fields(trie, tables, node)
        assert {f: int(e[f]) for f in want} == want, (tag, node)
        for got, ref_v in ((e["score"], tot), (e["blank_score"], pb), (e["nonblank_score"], pnb)):
            if ref_v == -math.inf:
                assert got == -math.inf, (tag, node)
            else:
                worst = max(worst, abs(float(got) - ref_v))
    print(f"{tag}: worst score difference {worst:.3e}")
    assert worst <= SCORE_TOL, (tag, worst)
    assert not ent[len(hyps):].tobytes().strip(b"\0"), tag          # entries past n_entries are zeroed


def test_cases_in_one_ragged_batch_and_alone(eng, tables, trie3, case_lp, case_ref):
    for c, lp, ref in zip(CASES, case_lp, case_ref):
        assert lp.min() > -30.0, c                                    # the premise of SCORE_TOL
        check_margins(ref, c)
    lp_all, frames = batch_of(case_lp)
    for W in sorted({c[5] for c in CASES}):
        info, ent, ids = eng.beam_raw(lp_all, frames, beam=W, k=W, max_span=3)
        for b, (c, ref) in enumerate(zip(CASES, case_ref)):
            if c[5] != W:
                continue
            check_row(info[b], ent[b], ref, trie3, tables, c[2], W, ("batch", c))
            assert ids[b, : ent[b, 0]["n_tokens"]].tolist() == trie3.tokens_of(int(ent[b, 0]["node"])) and (ids[b, ent[b, 0]["n_tokens"]:] == -1).all()
            one, frames1 = batch_of([case_lp[b]])
            info1, ent1, ids1 = eng.beam_raw(one, frames1, beam=W, k=W, max_span=3)
            # the bits of a row do not depend on the batch it travels in
            assert info1[0].tobytes() == info[b].tobytes() and ent1[0].tobytes() == ent[b].tobytes(), c
            assert ids1[0, : c[2]].tolist() == ids[b, : c[2]].tolist()
    # what the first and the third case decode to
    first = eng.beam_logprobs(*batch_of([case_lp[0]]), beam=8, k=5)[0]["hypotheses"][0]
    assert (first["surah"], first["ayah"], first["ayah_end"], first["complete"]) == (1, 1, 1, True)
    assert first["ids"] == tables.token_ids(0, 1).tolist() and first["text"] == tables.ids_to_text(first["ids"]) and first["matches"] >= 1
    third = eng.beam_logprobs(*batch_of([case_lp[2]]), beam=8, k=5)[0]["hypotheses"][0]
    assert not third["complete"] and third["n_tokens"] == 100 and third["surah"] == 0 and third["ayah_end"] is None
    assert third["ids"] == tables.token_ids(261, 1)[:100].tolist() and third["reachable"] >= 1
    v = tables.verse_index(*third["first_reachable"][:2])
    assert tables.token_ids(v, third["first_reachable"][2] - third["first_reachable"][1] + 1)[:100].tolist() == third["ids"]


def test_row_at_the_frame_capacity(tables, trie3):
    """T = 766 on an engine of 61 s, W = 8"""
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=1, max_samples=976640)
    try:
        assert e.frames_for(976640) + 2 == 766
        lp = make_lp(tables, 261, 1, 766, 1, 4)
        assert lp.min() > -30.0
        ref = R.beam_search(trie3, lp, 8, BLANK)
        check_margins(ref, "T=766")
        info, ent, _ = e.beam_raw(*batch_of([lp]), beam=8, k=8, max_span=3)
        check_row(info[0], ent[0], ref, trie3, tables, 766, 8, "T=766")
        with pytest.raises(Exception, match="frame capacity"):
            e.beam_raw(*batch_of([lp], extra=1), beam=8, k=8)
    finally:
        e.close()


def test_span_six_and_the_narrowest_and_widest_beam(eng, tables, trie3):
    ids6 = tables.token_ids(1, 6)
    assert 0 < len(ids6) * 3 + 6 <= 376
    lp6 = make_lp(tables, 1, 6, len(ids6) * 3 + 6, 1, 3)
    trie6 = R.Trie.from_tables(tables, 6)
    ref6 = R.beam_search(trie6, lp6, 8, BLANK)
    check_margins(ref6, "S=6")
    info, ent, _ = eng.beam_raw(*batch_of([lp6]), beam=8, k=8, max_span=6)
    check_row(info[0], ent[0], ref6, trie6, tables, len(lp6), 8, "S=6")
    assert (int(ent[0, 0]["start_verse"]), int(ent[0, 0]["span"]), int(ent[0, 0]["flags"])) == (1, 6, 1)
    assert eng.trie_node_tokens(int(ent[0, 0]["node"]), 6) == ids6.tolist()
    # ... and back to the trie of three spans, at W = 1 and W = 64 (k below W: the head of the list)
    lp = make_lp(tables, 50, 1, 60, 1, 3)
    for W, k in ((1, 1), (64, 64), (64, 5)):
        ref = R.beam_search(trie3, lp, W, BLANK)
        check_margins(ref, f"W={W}")
        info, ent, _ = eng.beam_raw(*batch_of([lp]), beam=W, k=k, max_span=3)
        check_row(info[0], ent[0], ref, trie3, tables, 60, k, f"W={W} k={k}")
    assert R.beam_search(trie3, lp, 64, BLANK)["max_candidates"] > 256         # more than one chunk of candidates per frame


def test_frames_past_the_length_are_never_read(eng, case_lp):
    clean = eng.beam_raw(*batch_of(case_lp), beam=8, k=8)
    lp_nan, frames = batch_of(case_lp, pad=float("nan"), extra=3)
    assert torch.isnan(lp_nan[0, frames[0]:]).all() and lp_nan.shape[1] == max(frames) + 3
    dirty = eng.beam_raw(lp_nan, frames, beam=8, k=8)
    assert clean[0].tobytes() == dirty[0].tobytes() and clean[1].tobytes() == dirty[1].tobytes()
    assert (clean[2] == dirty[2][:, : clean[2].shape[1]]).all() and (dirty[2][:, clean[2].shape[1]:] == -1).all()


def test_minus_infinity_follows_the_rules(eng, tables, trie3):
    """a frame with -inf on 1,000 tokens, and a frame that forbids the blank: dropped candidates, -inf blank scores"""
    lp = make_lp(tables, 50, 1, 36, 1, 3).copy()
    ids = tables.token_ids(50, 1).tolist()
    keep = set(frame_path(ids, 36, 2).tolist()) | {BLANK}
    dead = [k for k in range(1024) if k not in keep][:1000]
    lp[4, dead] = -np.inf
    lp[7, dead] = -np.inf
    lp[1, BLANK] = -np.inf
    ref = R.beam_search(trie3, lp, 8, BLANK)
    check_margins(ref, "-inf")
    info, ent, _ = eng.beam_raw(*batch_of([lp]), beam=8, k=8)
    check_row(info[0], ent[0], ref, trie3, tables, 36, 8, "-inf")
    # one frame, the blank forbidden: every survivor has a blank score of -inf; all of it forbidden but one token: one survivor
    one = make_lp(tables, 10, 1, 1, 1, 0).copy()
    one[0, BLANK] = -np.inf
    ref = R.beam_search(trie3, one, 8, BLANK)
    check_margins(ref, "no blank")
    info, ent, _ = eng.beam_raw(*batch_of([one]), beam=8, k=8)
    check_row(info[0], ent[0], ref, trie3, tables, 1, 8, "no blank")
    assert np.isneginf(ent[0]["blank_score"]).all() and 0 not in ent[0]["node"].tolist()
    first_tok = int(trie3.tok[1])
    one[:] = -np.inf
    one[0, first_tok] = 0.0
    info, ent, _ = eng.beam_raw(*batch_of([one]), beam=8, k=8)
    assert int(info[0]["n_entries"]) == 1 and int(ent[0, 0]["node"]) == 1 and float(ent[0, 0]["score"]) == 0.0


def test_score_of_a_complete_verse_against_the_ctc_kernel(eng, tables, trie3):
    """an independent kernel (the float32 alpha recursion behind the rerank, pinned to 1e-3): pruning can only lose mass"""
    lp = make_lp(tables, 0, 1, 40, 1, 12)
    ids = tables.token_ids(0, 1).tolist()
    node = trie3.walk(ids)
    dev, frames = batch_of([lp])
    loss = float(eng.debug_ctc_loss(dev[0, :40].contiguous(), [ids])[0])
    ref = {W: {h[0]: h[1] for h in R.beam_search(trie3, lp, W, BLANK)["hyps"]} for W in (8, 64)}
    lost = ref[64][node] - ref[8][node]
    assert lost >= 0.0
    for W in (8, 64):
        info, ent, _ = eng.beam_raw(dev, frames, beam=W, k=1)
        assert int(ent[0, 0]["node"]) == node and int(ent[0, 0]["flags"]) == 1
        score = float(ent[0, 0]["score"])
        print(f"W={W}: beam {score:.6f}  -ctc_loss {-loss:.6f}  lost mass (restatement, W=8 against 64) {lost:.3e}")
        assert score <= -loss + 1e-3
        assert abs(score + loss) <= 1e-3 + lost


def test_complete_entries_walk_back_to_the_table(eng, tables, case_lp):
    info, ent, _ = eng.beam_raw(*batch_of(case_lp), beam=16, k=16)
    seen = 0
    for b in range(len(case_lp)):
        for e in ent[b, : int(info[b]["n_entries"])]:
            toks = eng.trie_node_tokens(int(e["node"]), 3)
            assert len(toks) == int(e["n_tokens"])
            if e["flags"] & 1:
                assert toks == tables.token_ids(int(e["start_verse"]), int(e["span"])).tolist()
                seen += 1
    assert seen >= 3
    with pytest.raises(Exception, match="no such node"):
        eng.trie_node_tokens(523170, 3)
    with pytest.raises(Exception):
        eng.trie_node_tokens(-1, 3)
    assert eng.trie_node_tokens(0, 3) == []


def test_forward_entry_equals_forward_then_decode():
    from offline_tarteel_amd.engine import BEAM_ENTRY_DTYPE, BEAM_INFO_DTYPE, Engine

    e = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=32000)
    try:
        audio = torch.from_numpy(synth_audio(2, 32000)).cuda()
        audio[1, 24000:] = 0
        lens = [32000, 24000]
        lp, T = e.forward(audio, lens)
        info, ent, ids = e.beam_raw(lp, T, beam=8, k=5)
        rows = e.beam_batch(audio, lens, beam=8, k=5)
        assert [r["t_frames"] for r in rows] == T == info["t_frames"].tolist()
        for b, r in enumerate(rows):
            assert r["max_candidates"] == int(info[b]["max_candidates"]) and len(r["hypotheses"]) == int(info[b]["n_entries"]) >= 1
            for h, x in zip(r["hypotheses"], ent[b]):
                assert (h["node"], h["n_tokens"], h["matches"], h["start"], h["span"], h["surah"], h["ayah"], h["reachable"]) == \
                    tuple(int(x[f]) for f in ("node", "n_tokens", "n_ends", "start_verse", "span", "surah", "ayah", "below_count"))
                assert (h["score"], h["blank_score"], h["nonblank_score"]) == (float(x["score"]), float(x["blank_score"]), float(x["nonblank_score"]))
            assert r["hypotheses"][0]["ids"] == ids[b, : int(ent[b, 0]["n_tokens"])].tolist()
        assert BEAM_ENTRY_DTYPE.itemsize == 72 and BEAM_INFO_DTYPE.itemsize == 16
    finally:
        e.close()
    e = Engine(device=0, with_model=False, max_batch=2, max_samples=32000)
    try:
        with pytest.raises(Exception, match=r"\(5\)"):                # QV_ERR_NO_MODEL
            e.beam_batch(audio, lens)
    finally:
        e.close()


def test_bad_arguments_are_refused(eng, case_lp):
    dev, frames = batch_of(case_lp[:2])
    B, t_max = 2, dev.shape[1]
    info = np.zeros(B, dtype=[("a", "<i4", 4)])
    ent = np.zeros((B, 64), dtype=[("a", "u1", 72)])
    ids = np.zeros((B, t_max), np.int32)
    t = np.asarray(frames, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    lpp = C.c_void_p(dev.data_ptr())

    def call(lp=lpp, t_=t, batch=B, tm=t_max, span=3, beam=8, k=5, info_=info, ent_=ent, ids_=ids, pitch=t_max):
        return eng.lib.qv_beam_decode(eng.h, lp, p(t_), batch, tm, span, beam, k, p(info_), p(ent_), p(ids_), pitch, eng._stream())

    assert call() == 0 and call(ids_=None, pitch=0) == 0 and call(beam=64, k=64) == 0 and call(beam=1, k=1) == 0
    for bad in (dict(lp=None), dict(t_=None), dict(info_=None), dict(ent_=None), dict(batch=0), dict(tm=0), dict(span=0), dict(span=7),
                dict(beam=0), dict(beam=65, k=5), dict(k=0), dict(k=9), dict(pitch=t_max - 1),
                dict(t_=np.asarray([frames[0], t_max + 1], np.int32)), dict(t_=np.asarray([-1, frames[1]], np.int32))):
        assert call(**bad) == 1, bad                                   # QV_ERR_ARG
    wide = np.zeros(17, np.int32)
    assert call(t_=wide, batch=17, info_=np.zeros(17, info.dtype), ent_=np.zeros((17, 64), ent.dtype), ids_=None) == 4   # QV_ERR_CAPACITY
    assert call(tm=379, ids_=None) == 4                                # 376 + 2 frames: the engine's capacity
    assert eng.lib.qv_beam_decode(None, lpp, p(t), B, t_max, 3, 8, 5, p(info), p(ent), None, 0, None) == 1
    assert call() == 0                                                  # and the engine still works


def test_fallback_is_opt_in_and_takes_the_best_complete_hypothesis(tables, case_lp, monkeypatch):
    from offline_tarteel_amd import plugin
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=64000)   # 52 frames: room for the spelled rows
    try:
        monkeypatch.setattr(plugin, "_engine", e)
        monkeypatch.delenv("QVERSE_TRIE_FALLBACK", raising=False)
        audio = torch.from_numpy(synth_audio(2, 32000)).cuda()
        lens = [32000, 24000]
        base = plugin._finish(e, e.predict_batch(audio, lens), True, False, None)
        assert plugin.predict_device(audio, lens) == base and not plugin.trie_fallback_enabled()
        # set: rows that have a prediction stay as they are
        monkeypatch.setenv("QVERSE_TRIE_FALLBACK", "1")
        assert plugin.trie_fallback_enabled() and plugin.predict_device(audio, lens) == base
        # ... and a row without one is given to the search.  Injected: the batch comes back with two empty transcripts; the
        # log-probs the search sees spell 1:1 for row 0 and the first tokens of a verse for row 1
        real = e.predict_batch(audio, lens)
        empty = [dict(r, surah=0, ayah=0, ayah_end=None, score=0.0, source=None, flags=1, transcript="", greedy_ids=[]) for r in real]
        spelled = {0: case_lp[0], 1: case_lp[6]}
        asked = []

        def beam_batch(rows, ln, **kw):
            asked.append((tuple(rows.shape), list(ln)))
            return [e.beam_logprobs(*batch_of([spelled[i]]), **kw)[0] for i in range(len(ln))]

        monkeypatch.setattr(e, "predict_batch", lambda *a, **kw: [dict(r) for r in empty])
        monkeypatch.setattr(e, "beam_batch", beam_batch)
        got = plugin.predict_device(audio, lens)
        assert asked == [((2, 32000), lens)]
        assert (got[0]["surah"], got[0]["ayah"], got[0]["ayah_end"], got[0]["source"], got[0]["transcript"]) == (1, 1, 1, "trie", "")
        want = e.beam_logprobs(*batch_of([case_lp[0]]))[0]["hypotheses"][0]["score"]
        assert got[0]["score"] == want < 0.0                            # the log-probability, unrounded
        assert got[1] == plugin._empty("")                              # an incomplete prefix on top: still no prediction
        monkeypatch.delenv("QVERSE_TRIE_FALLBACK")
        assert plugin.predict_device(audio, lens) == [plugin._empty(""), plugin._empty("")] and len(asked) == 1
    finally:
        e.close()
