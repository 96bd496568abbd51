"""Device CTC forced alignment (csrc/qv_align.hip: qv_align, qv_align_results_ctx) against its numpy restatement
(tests/align_ref.py), through the C ABI, the engine binding and the plugin (GPU).

Paths (ids, first, last) and flags must be EQUAL, the path score bit-equal (one float32 add per state and frame on both
sides); the per-token mean log-prob is a float32 sum on the device and a float64 sum in the restatement: n_frames * 2**-23
relative, the worst case of a sequential float32 sum of same-signed terms plus the division.

Engine capacity: the cases reach T = 768 frames.  A post-logits-only engine for 976,000 samples holds 763 + 2 = 765, so the
engine here is created for 979,200 samples: 766 + 2 = 768 rows, the most qv_create allows.
"""

import gzip
import json
import struct

import numpy as np
import pytest
import torch

import align_ref
from align_ref import PLANTED, planted_case
from synth import hash_noise, synth_audio, synth_logits

pytestmark = pytest.mark.gpu

LADDER = [31, 32, 33, 63, 64, 95, 96, 127, 128, 191, 192, 255, 256, 383]   # 2L+1 around every states-per-lane step


@pytest.fixture(scope="module")
def engine():
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=False, max_batch=16, max_samples=979200)
    yield eng
    eng.close()


def noise_lp(T, seed):
    return torch.log_softmax(torch.from_numpy(hash_noise((T, 1025), seed) * np.float32(2.0)), -1).numpy()


def quantised_lp(T, seed):
    """multiples of 0.25: ties between the three predecessors are everywhere, the tie rule decides the path"""
    return (np.round(hash_noise((T, 1025), seed) * np.float32(2.0)) / np.float32(4.0) - np.float32(3.0)).astype(np.float32)


def ladder_ids(L, seed):
    """random ids with adjacent repeats: at the front, the back, and across every boundary between two lanes' states for
    each states-per-lane count the kernel is instantiated for (state 2i+1 | 2i+3 straddles lanes when NS divides 2i+2)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 1024, size=L)
    for i in sorted({1, 2, 31, 32, 47, 63, 64, 95, 96, 127, 191, 255, L - 1}):
        if 1 <= i < L:
            ids[i] = ids[i - 1]
    return ids.astype(np.int64)


def run_rows(engine, lps, targets):
    """one qv_align call over the rows (padded with -50 like the post-logits tests pad)"""
    Ts = [x.shape[0] for x in lps]
    t_max = max(max(Ts), 1)
    batch = np.full((len(lps), t_max, 1025), -50.0, np.float32)
    for b, x in enumerate(lps):
        batch[b, : x.shape[0]] = x
    return engine.align(torch.from_numpy(batch).cuda().contiguous(), Ts, targets)


def check_row(got, lp, ids, tag):
    want = align_ref.viterbi(lp, ids)
    assert got["flags"] == want["flags"], (tag, got["flags"], want["flags"])
    assert got["t_frames"] == lp.shape[0]
    if want["flags"]:
        assert len(got["ids"]) == len(got["first"]) == len(got["last"]) == len(got["logp"]) == 0 and got["score"] == 0.0, tag
        return want
    assert got["n_tokens"] == len(ids) and got["ids"].tolist() == list(map(int, ids)), tag
    assert got["first"].tolist() == want["first"].tolist(), tag
    assert got["last"].tolist() == want["last"].tolist(), tag
    assert np.float32(got["score"]).view(np.uint32) == np.float32(want["score"]).view(np.uint32), (tag, got["score"], want["score"])
    n = want["last"] - want["first"] + 1
    err = np.abs(got["logp"].astype(np.float64) - want["logp"])
    assert (err <= n * 2.0 ** -23 * np.abs(want["logp"])).all(), (tag, float(err.max()))
    return want


def test_degenerate_shapes_and_flags(engine):
    lp = noise_lp(6, 5)
    cases = [([9], lp[:1]), ([9], lp[:2]), ([3, 1000, 17, 512, 0], lp[:5]), ([7, 7, 7, 9], lp[:6]),
             ([], lp[:6]), ([7, 7, 7, 9], lp[:5]), ([5] * 384, lp[:6])]
    got = run_rows(engine, [c[1] for c in cases], [c[0] for c in cases])
    for k, (g, (ids, x)) in enumerate(zip(got, cases)):
        check_row(g, x, ids, k)
    assert [g["flags"] for g in got] == [0, 0, 0, 0, align_ref.NO_TARGET, align_ref.INFEASIBLE, align_ref.TOO_LONG]
    assert got[3]["first"].tolist() == [0, 2, 4, 5]            # T = 6 leaves [7,7,7,9] exactly one path
    assert got[2]["first"].tolist() == got[2]["last"].tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("kind", ["noise", "quantised"])
@pytest.mark.parametrize("L", LADDER)
def test_every_register_ladder_edge(engine, L, kind):
    T = min(768, 2 * L + 5)
    lp = noise_lp(T, 100 + L) if kind == "noise" else quantised_lp(T, 200 + L)
    ids = ladder_ids(L, L)
    got = run_rows(engine, [lp], [ids])[0]
    want = check_row(got, lp, ids, (L, kind))
    assert want["flags"] == 0
    if kind == "quantised":   # the scores really do tie: a different rule gives a different path
        assert float(want["score"]) * 4 == round(float(want["score"]) * 4)


@pytest.mark.parametrize("L,T,rep", PLANTED)
def test_planted_paths_come_back(engine, L, T, rep):
    ids, lp = planted_case(L, T, rep)
    got = run_rows(engine, [lp], [ids])[0]
    check_row(got, lp, ids, (L, T, rep))
    want_first = np.arange(L) * (rep + 1)
    assert got["first"].tolist() == want_first.tolist() and got["last"].tolist() == (want_first + rep - 1).tolist()


def test_batch_invariance_on_a_ragged_batch(engine):
    """7 rows, T in {1, 16, 126, 127, 376}, one row without a target and one without a path: every row of the batch
    call carries the bits of its own single-row call"""
    shapes = [(1, 1), (5, 16), (40, 126), (0, 126), (50, 127), (120, 376), (20, 16)]   # (L, T); (20, 16): infeasible
    lps = [noise_lp(T, 300 + k) for k, (_, T) in enumerate(shapes)]
    targets = [ladder_ids(L, 400 + k) if L else np.zeros(0, np.int64) for k, (L, _) in enumerate(shapes)]
    together = run_rows(engine, lps, targets)
    assert [g["flags"] for g in together] == [0, 0, 0, align_ref.NO_TARGET, 0, 0, align_ref.INFEASIBLE]
    for k, g in enumerate(together):
        check_row(g, lps[k], targets[k], k)
        alone = run_rows(engine, [lps[k]], [targets[k]])[0]
        for key in ("ids", "first", "last"):
            assert g[key].tolist() == alone[key].tolist(), (k, key)
        assert g["logp"].view(np.uint32).tolist() == alone["logp"].view(np.uint32).tolist(), k
        assert (g["score"], g["flags"], g["n_tokens"], g["t_frames"]) == (alone["score"], alone["flags"], alone["n_tokens"], alone["t_frames"])


def test_through_the_pipeline_on_the_e2e_fixtures(engine, golden_dir):
    """decode_retrieve_rerank(align=True) on the e2e fixtures' log-probs: the aligned ids are the table's token list of the
    winner, the path is the restatement's on the same log-probs -- for text-matched and CTC-reranked winners alike"""
    cases = json.load(gzip.open(golden_dir / "e2e_cases.json.gz"))
    lps = []
    for c in cases:
        r = c["recipe"]
        lg = synth_logits(r["ids"], r["T"], seed=r["seed"], noise=r["noise"], boost=r["boost"], rep=r["rep"])
        lps.append(torch.log_softmax(torch.from_numpy(lg), dim=-1))
    t_max = max(x.shape[0] for x in lps)
    batch = torch.full((len(lps), t_max, 1025), -50.0)
    for b, x in enumerate(lps):
        batch[b, : x.shape[0]] = x
    dev = batch.cuda().contiguous()
    Ts = [x.shape[0] for x in lps]
    res = engine.decode_retrieve_rerank(dev, Ts, align=True)
    plain = engine.decode_retrieve_rerank(dev, Ts)
    tb = engine.tables
    aligned = set()
    for c, r, p, x in zip(cases, res, plain, lps):
        a = r.pop("alignment")
        assert r == p, c["name"]                      # the prediction itself is untouched
        if not r["surah"]:
            assert a["flags"] == align_ref.NO_TARGET and len(a["ids"]) == 0, c["name"]
            continue
        assert tb.key_of(a["start"], a["span"]) == (r["surah"], r["ayah"], r["ayah_end"]), c["name"]
        ids = tb.token_ids(a["start"], a["span"]).astype(np.int64)
        assert a["n_tokens"] == len(ids)
        want = check_row(a, x.numpy(), ids, c["name"])
        if not want["flags"]:
            aligned.add(r["source"])
    assert aligned == {"text", "ctc"}, aligned


def test_alignment_belongs_to_its_context():
    """two contexts, two batches in flight: the alignment of context 0 asked for AFTER the second launch is the first
    batch's -- winner and log-probs are the context's.  Seeded random weights recognise nothing, so the post-logits
    stages read injected verse-shaped log-probs (qv_profile_inject_logprobs), a different tensor per batch."""
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=32000, contexts=2)
    try:
        tb = eng.tables
        T = 24

        def verse_lp(refs, seed):
            rows = []
            for k, (s, a) in enumerate(refs):
                ids = tb.token_ids(tb.verse_index(s, a), 1).tolist()
                assert 2 * len(ids) <= T
                rows.append(torch.log_softmax(torch.from_numpy(synth_logits(ids, T, seed=seed + k, noise=1.0, boost=8.0, rep=1)), -1))
            return torch.stack(rows)

        lp_a, lp_b = verse_lp([(112, 2), (112, 1)], 1), verse_lp([(112, 3), (112, 4)], 5)
        dev_a, dev_b = lp_a.cuda().contiguous(), lp_b.cuda().contiguous()
        audio = torch.from_numpy(synth_audio(2, 32000)).cuda()
        lens = [32000, 32000]
        eng.inject_logprobs(dev_a, [T, T])
        ctx0 = eng.predict_batch_async(audio, lens)
        eng.inject_logprobs(dev_b, [T, T])
        ctx1 = eng.predict_batch_async(audio, lens)
        assert ctx0 != ctx1
        al0 = eng.align_results(ctx0, 2)
        res0 = eng.fetch_results(ctx0, 2, T)
        al1 = eng.align_results(ctx1, 2)
        res1 = eng.fetch_results(ctx1, 2, T)
        eng.inject_logprobs(None)
        keys0 = [(r["surah"], r["ayah"]) for r in res0]
        keys1 = [(r["surah"], r["ayah"]) for r in res1]
        assert all(k[0] for k in keys0 + keys1) and not set(keys0) & set(keys1), (keys0, keys1)
        for al, res, lp in ((al0, res0, lp_a), (al1, res1, lp_b)):
            for b in range(2):
                assert tb.key_of(al[b]["start"], al[b]["span"]) == (res[b]["surah"], res[b]["ayah"], res[b]["ayah_end"])
                want = check_row(al[b], lp[b].numpy(), tb.token_ids(al[b]["start"], al[b]["span"]).astype(np.int64), b)
                assert want["flags"] == 0
        # nothing to align once the context's workspace has been reused by a single-text call
        from offline_tarteel_amd.engine import QvError

        eng.match_verse("قل هو الله احد")
        with pytest.raises(QvError):
            eng.align_results(int(eng.lib.qv_last_context(eng.h)), 2)
    finally:
        eng.close()


def test_argument_errors(engine):
    import ctypes as C

    from offline_tarteel_amd.engine import ALIGN_INFO_DTYPE, QvError

    lp = torch.from_numpy(noise_lp(8, 1)[None]).cuda().contiguous()
    t, lens, tg = np.array([8], np.int32), np.array([2], np.int32), np.array([3, 4], np.uint16)
    info = np.zeros(1, ALIGN_INFO_DTYPE)
    first, last, logp = np.zeros(400, np.int16), np.zeros(400, np.int16), np.zeros(400, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(t_max, pitch):
        return engine.lib.qv_align(engine.h, C.c_void_p(lp.data_ptr()), p(t), 1, t_max, p(tg), p(lens), p(info), p(first), p(last),
                                   p(logp), pitch, None)

    assert call(8, 382) == 1            # QV_ERR_ARG: pitch < QV_ALIGN_MAX_TOKENS
    assert call(769, 383) == 4          # QV_ERR_CAPACITY: t_max above the engine's frame capacity
    assert call(8, 400) == 0 and info[0]["flags"] == 0 and first[:3].tolist() != [0, 0, 0]
    assert first[2:400].tolist() == [-1] * 398 and logp[2:].tolist() == [0.0] * 398   # entries past n_tokens, past 383 too
    with pytest.raises(QvError):
        engine.align(lp, [8], [[3, 1024]])   # the blank is no target id


def test_plugin_words(tmp_path, monkeypatch):
    """predict_batch(paths, words=True) on the small synthetic WAV corpus of the plugin test: [] where nothing is
    recognised (seeded random weights), well-formed words where a verse is (injected verse-shaped log-probs); without
    words= the dicts are the same as before"""
    from offline_tarteel_amd import plugin
    from offline_tarteel_amd.words import ayah_word_counts

    paths = []
    for i, n in enumerate((24000, 36000, 30000)):
        data = (synth_audio(1, n, seed=50 + i)[0] * 20000).astype("<i2").tobytes()
        hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack(
            "<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", len(data))
        (tmp_path / f"s{i}.wav").write_bytes(hdr + data)
        paths.append(str(tmp_path / f"s{i}.wav"))
    monkeypatch.setenv("QVERSE_RANDOM_WEIGHTS", "1")
    monkeypatch.setattr(plugin, "_engine", None)
    monkeypatch.setattr(plugin, "MAX_SAMPLES", 64000)
    monkeypatch.setattr(plugin, "MAX_BATCH", 4)
    try:
        plain = plugin.predict_batch(paths)
        with_words = plugin.predict_batch(paths, words=True)
        assert all("words" not in d for d in plain)
        for a, b in zip(plain, with_words):
            assert {k: v for k, v in b.items() if k != "words"} == a
            if not a["surah"]:
                assert b["words"] == []
        eng = plugin._engine
        tb = eng.tables
        T = 24
        refs = [(112, 2), (112, 1), (112, 3)]
        lp = torch.stack([torch.log_softmax(torch.from_numpy(synth_logits(
            tb.token_ids(tb.verse_index(s, a), 1).tolist(), T, seed=9 + k, noise=1.0, boost=8.0, rep=1)), -1)
            for k, (s, a) in enumerate(refs)]).cuda().contiguous()
        eng.inject_logprobs(lp, [T] * 3)
        seen = plugin.predict_batch(paths, words=True)
        monkeypatch.setattr(plugin, "_WORDS", True)
        # (a clip with at least T frames: under the injection hook the engine copies the greedy ids back with the INJECTED
        # frame count as pitch, and the binding sizes that buffer from the clip; a batch of one reads injected row 0)
        one = plugin.predict(paths[1])
        eng.inject_logprobs(None)
        assert one["words"] == seen[0]["words"]
        assert any(d["surah"] for d in seen)
        for d in seen:
            if not d["surah"]:
                assert d["words"] == []
                continue
            v, span = tb.verse_index(d["surah"], d["ayah"]), d["ayah_end"] - d["ayah"] + 1
            words = d["words"]
            assert len(words) == sum(ayah_word_counts(tb, v, span)) > 0
            assert set(words[0]) == {"ayah", "word", "text", "start", "end", "logp"}
            assert all(d["ayah"] <= w["ayah"] <= d["ayah_end"] and w["word"] >= 1 and w["text"] and w["logp"] <= 0 for w in words)
            assert all(0 <= w["start"] < w["end"] <= T * 0.08 + 1e-9 for w in words)
            assert all(b["start"] >= a["end"] for a, b in zip(words, words[1:]))
    finally:
        if plugin._engine is not None:
            plugin._engine.close()
        monkeypatch.setattr(plugin, "_engine", None)
