"""Recitation correction on the device (csrc/qv_correct.hip: qv_correct, qv_correct_results_ctx) against the restatement
(tests/correct_ref.py), through the C ABI, the engine binding and the plugin (GPU).  Every compared field is an integer:
info, op codes and word records have to be the restatement's exactly."""

import ctypes as C
import json
import struct

import numpy as np
import pytest
import torch

import correct_ref as cr
from synth import synth_audio, synth_logits

pytestmark = pytest.mark.gpu

GRID = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257]   # the 16-row ownership of a thread, the wave, the 128-thread block


def make_engine(**kw):
    from offline_tarteel_amd.engine import Engine

    kw.setdefault("max_batch", 64)
    return Engine(device=0, with_model=False, **kw)


@pytest.fixture(scope="module")
def engine():
    eng = make_engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def wide():
    eng = make_engine(max_transcript=2048)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def cases(golden_dir):
    return json.load(open(golden_dir / "correction_cases.json"))


def spaced(rng, sym, n_spaces):
    """the symbols with n_spaces single spaces at distinct inner positions"""
    sym = list(sym)
    n_spaces = min(n_spaces, max(len(sym) - 1, 0))
    cuts = set((rng.choice(len(sym) - 1, n_spaces, replace=False) + 1).tolist()) if n_spaces else set()
    out = []
    for k, c in enumerate(sym):
        if k in cuts:
            out.append(0)
        out.append(int(c))
    return out


def same(got, want, tag):
    """one device row (Engine._corrections dict) against one restatement result"""
    info = {k: got[k] for k in cr.INFO_FIELDS}
    assert info == want["info"], (tag, info, want["info"])
    assert got["ops"].tolist() == want["ops"], (tag, got["ops"].tolist()[:40], want["ops"][:40])
    words = [tuple(int(w[k]) for k in cr.WORD_FIELDS) for w in got["words"]]
    assert words == want["words"], (tag, words[:8], want["words"][:8])


def run(eng, pairs, prefix=False, check_padding=True):
    """pairs: [(pred codes, ref codes)] through qv_correct in ONE call; every row against the restatement"""
    info, ops, words = eng.correct_raw([p for p, _ in pairs], [r for _, r in pairs], prefix)
    rows = eng._corrections(info, ops, words)
    for b, ((p, r), got) in enumerate(zip(pairs, rows)):
        same(got, cr.correct(p, r, prefix, max_pred=eng.max_transcript), (b, len(p), len(r), prefix))
        if check_padding:
            assert (ops[b, got["n_ops"]:] == 0xFF).all() and words[b, got["n_words"]:].tobytes() == bytes(words[b, got["n_words"]:].nbytes), b
            assert (info[b]["reserved"] == 0).all()
    return rows


# ------------------------------------------------------------------ 1. explicit texts
def test_every_fixture_pair(engine, cases):
    """the reference's own alignments: the device returns the op codes of align_phonemes' columns (the host test holds the
    restatement to the fixture; here the device is held to both)"""
    rng = np.random.default_rng(5)
    for s in range(0, len(cases), 64):
        chunk = cases[s: s + 64]
        pairs = [(spaced(rng, c["pred"], int(rng.integers(0, 4))), spaced(rng, c["ref"], int(rng.integers(0, 6)))) for c in chunk]
        rows = run(engine, pairs)
        for c, got in zip(chunk, rows):
            ops = [0 if a == b else 1 if a is not None and b is not None else 2 if b is None else 3 for a, b in c["alignment"]]
            assert got["ops"].tolist() == ops and got["distance"] == len(c["errors"]), c["name"]


def test_degenerate_rows_and_tie_probes(engine):
    a, b = 5, 9
    verse = engine.tables.span_codes(engine.tables.verse_index(2, 255), 1).tolist()
    pairs = [([a], [a]), ([a], [b]), ([a, 0, b], []), ([], [a, b]), ([], []), ([0, 0], [a]), ([a], [0]),
             ([a, b], [b, a]), ([a, b], [a, a, b]), ([b, a], [a, b]), ([a, a, b], [a, b]),
             ([63] * 40, verse), ([63, 0, 63], [63, 63]),
             ([a, b], [a, 0, 0, b]), ([0, a, b, 0], [0, a, 0, b, 0])]       # runs of spaces: words without symbols
    rows = run(engine, pairs)
    assert [r["flags"] for r in rows[:7]] == [0, 0, cr.NO_TARGET, cr.NO_TRANSCRIPT, cr.NO_TARGET | cr.NO_TRANSCRIPT,
                                              cr.NO_TRANSCRIPT, cr.NO_TARGET]
    assert rows[0]["ops"].tolist() == [0] and rows[1]["ops"].tolist() == [1]
    assert all(r["n_ops"] == 0 and r["n_ref"] == 0 and r["n_pred"] == 0 and len(r["words"]) == 0 for r in rows[2:7])
    assert rows[7]["ops"].tolist() == [1, 1]                      # ab / ba: S before D and I (the other probes: test_correct_host.py)
    assert rows[11]["n_match"] == 0 and rows[11]["n_sub"] == 40   # 63 never equals a table code ...
    assert rows[12]["ops"].tolist() == [0, 0]                     # ... and is an ordinary symbol against itself
    assert rows[13]["n_words"] == 3 and rows[14]["n_words"] == 4


def size_grid(rng, n_rows=64):
    sizes = [(n, m) for n in GRID for m in GRID]
    pick = [sizes[i] for i in rng.permutation(len(sizes))[:n_rows - len(GRID)]] + [(g, g) for g in GRID]
    pairs = []
    for n, m in pick:
        ref = rng.integers(1, 4, n).tolist()
        pred = rng.integers(1, 4, m).tolist()
        if n == m:                                                # a recitation with a few slips, not noise
            pred = list(ref)
            for at in rng.integers(0, n, 3):
                pred[int(at)] = int(rng.integers(1, 4))
        pairs.append((spaced(rng, pred, 3), spaced(rng, ref, min(n // 3, 40))))
    return pairs


@pytest.mark.parametrize("prefix", [False, True])
def test_size_grid(engine, prefix):
    """n and m from the sizes where the sweep changes shape, a 3-symbol alphabet (ties everywhere), one call of 64 rows"""
    pairs = size_grid(np.random.default_rng(11))
    assert len(pairs) == 64 and {len(cr.strip(r)[0]) for _, r in pairs} == set(GRID)
    rows = run(engine, pairs, prefix)
    if prefix:
        assert any(r["n_ref_used"] < r["n_ref"] for r in rows) and any(r["flags"] & cr.LAST_WORD_OPEN for r in rows)


@pytest.mark.parametrize("window", [1024, 2048])
def test_caps(engine, wide, window):
    eng = engine if window == 1024 else wide
    assert eng.max_transcript == window
    rng = np.random.default_rng(window)
    ref = rng.integers(1, 4, cr.MAX_REF).tolist()
    pred = rng.integers(1, 4, window).tolist()
    near = list(ref[:window])
    for at in rng.integers(0, len(near), 25):
        near[int(at)] = 3
    ok = ([1, 2, 0, 3], [1, 2, 0, 2])
    # m = window + 1: a row of its own with the default window; with the wide one such a text is above QV_CORRECT_MAX_RAW and
    # refused before anything runs (test_argument_errors), so the longest text there is the window itself
    over = (pred + [2], ref) if window == 1024 else (pred, ref[:-1] + [0, 0, 1])
    pairs = [ok, (pred, spaced(rng, ref, 287)), (near, spaced(rng, ref, 100)), (pred, ref + [1]), ok, over, ok,
             (pred, spaced(rng, ref, 288)), ok]
    for prefix in (False, True):
        rows = run(eng, pairs, prefix)
        assert [r["flags"] & cr.TOO_LONG for r in rows] == [0, 0, 0, 4, 0, 4 if window == 1024 else 0, 0, 4, 0]
        assert rows[1]["n_ref"] == cr.MAX_REF and rows[1]["n_pred"] == window and rows[1]["n_words"] == cr.MAX_WORDS
        # the neighbours of the flagged rows are untouched (in prefix mode the last symbol is a trailing insertion)
        assert rows[0]["ops"].tolist() == rows[4]["ops"].tolist() == rows[8]["ops"].tolist() == ([0, 0, 3] if prefix else [0, 0, 1])


def test_rounds_of_64_rows():
    eng = make_engine(max_batch=128)
    try:
        rng = np.random.default_rng(3)
        pairs = [(spaced(rng, rng.integers(1, 4, int(rng.integers(1, 90))), 2), spaced(rng, rng.integers(1, 4, int(rng.integers(1, 90))), 5))
                 for _ in range(65)]
        run(eng, pairs)
        run(eng, pairs[:64] + pairs[:1] * 64, prefix=True)        # two full rounds
    finally:
        eng.close()


def test_prefix_of_a_verse(engine):
    """a recitation that stops after word k of 2:255: nothing is wrong, k words touched, the last word closed"""
    tb = engine.tables
    ref = tb.span_codes(tb.verse_index(2, 255), 1).tolist()
    ends = [i for i, c in enumerate(ref) if c == 0]
    pairs = [(ref[:ends[k]], ref) for k in (0, 6, 20)] + [(ref[:ends[5] + 3], ref)]     # ... and two symbols into word 7
    rows = run(engine, pairs, prefix=True)
    assert [(r["distance"], r["words_touched"], r["flags"]) for r in rows] == [(0, 1, 0), (0, 7, 0), (0, 21, 0), (0, 7, cr.LAST_WORD_OPEN)]
    full = run(engine, pairs)
    assert all(r["n_ref_used"] == r["n_ref"] and r["n_del"] == r["n_ref"] - r["n_pred"] for r in full)


def test_batch_position_invariance(engine):
    rng = np.random.default_rng(17)
    ref = spaced(rng, rng.integers(1, 4, 300), 40)
    pred = spaced(rng, rng.integers(1, 4, 280), 3)
    filler = ([1, 2, 3], [1, 3])
    pairs = [filler] * 64
    for at in (0, 31, 63):
        pairs[at] = (pred, ref)
    for prefix in (False, True):
        info, ops, words = engine.correct_raw([p for p, _ in pairs], [r for _, r in pairs], prefix)
        for at in (31, 63):
            assert info[at].tobytes() == info[0].tobytes() and ops[at].tobytes() == ops[0].tobytes()
            assert words[at].tobytes() == words[0].tobytes()
        same(engine._corrections(info, ops, words)[0], cr.correct(pred, ref, prefix), prefix)


# ------------------------------------------------------------------ 2. through a batch
def word_groups(tb, ids):
    """token indices per word, as words.words_from_alignment groups them"""
    groups = []
    for i, tok in enumerate(ids):
        if not groups or (int(tok) != 0 and tb.piece_surface[int(tok)].startswith(" ")):
            groups.append([])
        groups[-1].append(i)
    return groups


def batch_rows(eng):
    """[(kind, start, span, token ids, dropped word | None, the text these tokens decode to is the one the row was built from)]
    (2:285 and 2:255 carry marks the normaliser drops: their rows differ from the table's text and are only held to the
    restatement)"""
    tb = eng.tables
    spells = lambda ids, codes: tb.encode(eng.transcript_of(ids)).tolist() == codes  # noqa: E731
    rows = []
    for s, a, sp in [(1, 6, 2), (2, 285, 1), (67, 1, 1), (93, 1, 3), (97, 1, 2), (103, 1, 3), (94, 1, 4), (99, 1, 3), (36, 1, 4), (2, 255, 1)]:
        v = tb.verse_index(s, a)
        ids = tb.token_ids(v, sp).tolist()
        ref = tb.span_codes(v, sp).tolist()
        groups = word_groups(tb, ids)
        assert len(groups) == ref.count(0) + 1, (s, a, sp)
        rows.append(("intact", v, sp, ids, None, spells(ids, ref)))
        # a dropped word whose symbols can only be deleted where they stood (the restatement says so before the device is asked)
        ends = [-1] + [i for i, c in enumerate(ref) if c == 0] + [len(ref)]
        for k in range(2, len(groups) - 1):
            pred = ref[: ends[k]] + ref[ends[k + 1]:]
            w = cr.correct(pred, ref)["words"]
            if w[k][5] == cr.DEL and w[k][3] == w[k][0] and all(x[5] == 0 for i, x in enumerate(w) if i != k):
                left = [t for g in groups[:k] + groups[k + 1:] for t in (ids[i] for i in g)]
                rows.append(("dropped", v, sp, left, k, spells(left, pred)))
                break
        swapped = list(ids)
        at = len(ids) // 2
        swapped[at] = ids[at - 1] if ids[at - 1] != ids[at] else ids[at - 2]
        rows.append(("swapped", v, sp, swapped, None, False))
    rows.append(("empty", -1, 0, [], None, False))
    return rows


def check_batch(eng):
    from offline_tarteel_amd.engine import CORRECT_NO_TARGET

    tb = eng.tables
    rows = batch_rows(eng)
    assert sum(r[0] == "dropped" and r[5] for r in rows) >= 4 and sum(r[0] == "intact" and r[5] for r in rows) >= 6
    lps = []
    for k, (kind, v, sp, ids, _, _) in enumerate(rows):
        T = max(2 * len(ids) + 2, 8)
        lg = synth_logits(ids, T, seed=100 + k, noise=0.5 if ids else 0.0, boost=12.0 if ids else 0.0, rep=1)
        lps.append(torch.log_softmax(torch.from_numpy(lg), -1))
    t_max = max(x.shape[0] for x in lps)
    assert t_max <= 376
    dev = torch.full((len(lps), t_max, 1025), -50.0)
    for b, x in enumerate(lps):
        dev[b, : x.shape[0]] = x
    dev = dev.cuda().contiguous()
    res = eng.decode_retrieve_rerank(dev, [x.shape[0] for x in lps])
    got = eng.correct_results(batch=len(rows))
    got_p = eng.correct_results(batch=len(rows), prefix=True)
    codes = eng.transcript_codes(batch=len(rows))
    with_c = eng.decode_retrieve_rerank(dev, [x.shape[0] for x in lps], correct=True)
    checked = {"intact": 0, "dropped": 0, "swapped": 0}
    for b, (kind, v, sp, ids, k, exact) in enumerate(rows):
        pred = codes[b]["codes"].tolist()
        st, n_ay = got[b]["start_verse"], got[b]["span"]
        if not res[b]["surah"]:
            assert kind == "empty" and got[b]["flags"] & CORRECT_NO_TARGET and got[b]["n_ops"] == 0, (b, kind)
            same(got[b], cr.correct(pred, []), (b, kind))
            continue
        assert kind != "empty" and tb.key_of(st, n_ay) == (res[b]["surah"], res[b]["ayah"], res[b]["ayah_end"]), (b, kind)
        ref = tb.span_codes(st, n_ay).tolist()
        same(got[b], cr.correct(pred, ref, start_verse=st, span=n_ay, max_pred=eng.max_transcript), (b, kind))
        same(got_p[b], cr.correct(pred, ref, True, start_verse=st, span=n_ay, max_pred=eng.max_transcript), (b, kind, "prefix"))
        assert {x: y for x, y in with_c[b].items() if x != "correction"} == res[b]
        c = with_c[b]["correction"]
        assert c["ops"].tolist() == got[b]["ops"].tolist() and c["pred_codes"].tolist() == pred and c["ref_codes"].tolist() == ref
        if (st, n_ay) != (v, sp):
            continue                                              # (another text won: the row is still the restatement's)
        if kind == "intact" and exact:
            assert got[b]["distance"] == 0 and all(int(w["type"]) == 0 for w in got[b]["words"]), (b, kind)
        if kind == "dropped" and exact:
            types = [int(w["type"]) for w in got[b]["words"]]
            assert types[k] == cr.DEL and sum(types) == cr.DEL and got[b]["n_del"] == got[b]["distance"] > 0, (b, k, types)
        if kind == "swapped":
            assert got[b]["distance"] > 0
        checked[kind] += exact or kind == "swapped"
    print("rows held to their recipe:", checked, "sources:", sorted({str(r["source"]) for r in res}))
    assert checked["intact"] >= 6 and checked["dropped"] >= 3 and checked["swapped"] >= 5, checked
    return {res[b]["source"] for b in range(len(rows))}


def test_through_a_batch(engine):
    """the default knobs: rows that pass the text gate and rows the CTC rerank decides, in one batch"""
    assert {"text", "ctc"} <= check_batch(engine)


def test_through_a_batch_wide_window(wide):
    check_batch(wide)


def test_behind_the_forward_on_a_model_engine():
    """random weights recognise nothing: the rows are mostly NO_TARGET, but the entry runs behind the forward on the
    context's own bookkeeping, and whatever a row holds is the restatement's"""
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=True, seed=7, max_batch=4, max_samples=48000)
    try:
        audio = torch.from_numpy(synth_audio(3, 48000)).cuda()
        res = eng.predict_batch(audio, [48000, 30000, 40000])
        got = eng.correct_results(batch=3, texts=True)
        for b in range(3):
            ref = eng.tables.span_codes(got[b]["start_verse"], got[b]["span"]).tolist() if res[b]["surah"] else []
            assert got[b]["ref_codes"].tolist() == ref
            want = cr.correct(got[b]["pred_codes"].tolist(), ref, start_verse=got[b]["start_verse"] if ref else -1, span=got[b]["span"] if ref else 0)
            same(got[b], want, b)
            if not res[b]["surah"]:
                assert got[b]["flags"] & cr.NO_TARGET
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. errors
def test_argument_errors():
    from offline_tarteel_amd.engine import CORRECT_INFO_DTYPE, CORRECT_WORD_DTYPE, QvError

    eng = make_engine()
    try:
        pitch = cr.MAX_REF + eng.max_transcript
        info, ops, words = np.zeros(65, CORRECT_INFO_DTYPE), np.zeros((65, pitch), np.uint8), np.zeros((65, cr.MAX_WORDS), CORRECT_WORD_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        codes = np.ones(65 * 4 + cr.MAX_RAW + 8, np.uint8)
        off = (np.arange(66) * 4).astype(np.int32)

        def explicit(rows=2, flags=0, pc=codes, po=off, rc=codes, ro=off, i=info, o=ops, op=pitch, w=words, wp=cr.MAX_WORDS):
            return eng.lib.qv_correct(eng.h, p(pc), p(po), p(rc), p(ro), rows, flags, p(i), p(o), op, p(w), wp, None)

        def results(ctx=0, batch=1, flags=0, i=info, o=ops, op=pitch, w=words, wp=cr.MAX_WORDS):
            return eng.lib.qv_correct_results_ctx(eng.h, ctx, batch, flags, p(i), p(o), op, p(w), wp)

        long_off = off.copy()
        long_off[2:] += cr.MAX_RAW - 3                           # text 1 has 2,049 codes
        assert explicit() == 0 and int(info[0]["n_match"]) == 4
        assert explicit(o=None, w=None) == 0 and explicit(flags=1) == 0
        for bad in (dict(rows=0), dict(flags=2), dict(flags=-1), dict(pc=None), dict(po=None), dict(rc=None), dict(ro=None), dict(i=None),
                    dict(op=pitch - 1), dict(wp=cr.MAX_WORDS - 1), dict(po=long_off), dict(ro=long_off), dict(po=off[::-1].copy())):
            assert explicit(**bad) == 1, bad
            assert explicit() == 0
        long_off[2:] -= 1                                         # 2,048 codes are accepted (and flagged: above the window)
        assert explicit(po=long_off) == 0 and int(info[1]["flags"]) == cr.TOO_LONG and int(info[0]["flags"]) == 0
        assert explicit(rows=65) == 4                             # QV_ERR_CAPACITY
        assert explicit() == 0
        assert results() == 1                                     # the context holds no batch yet
        lp = torch.full((3, 8, 1025), -50.0)
        lp[:, :, 1024] = 0.0
        eng.decode_retrieve_rerank(lp.cuda().contiguous(), [8, 8, 8])
        assert results(batch=3) == 0 and results(batch=3, flags=1) == 0 and results(batch=3, o=None, w=None) == 0
        assert all(int(x) & cr.NO_TARGET for x in info[:3]["flags"])
        for bad in (dict(ctx=-1), dict(ctx=1), dict(batch=0), dict(batch=4), dict(flags=2), dict(i=None), dict(op=pitch - 1),
                    dict(wp=cr.MAX_WORDS - 1)):
            assert results(**bad) == 1, bad
            assert results(batch=3) == 0
        assert results(batch=65) == 4
        assert explicit() == 0 and results(batch=3) == 0          # the explicit form leaves the context's batch alone
        with pytest.raises(QvError):
            eng.correct(["x" * 2049], ["y"])
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. the plugin
def test_plugin_corrections(tmp_path, monkeypatch):
    """predict_batch(paths, corrections=True) on the small synthetic WAV corpus of the plugin tests (seeded random weights;
    verse-shaped log-probs injected where a verse has to be recognised): "correction" is correction.fold of the engine's
    own rows; without the option the dicts are what they were"""
    from offline_tarteel_amd import correction, plugin

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
        with_c = plugin.predict_batch(paths, corrections=True)
        eng = plugin._engine
        for a, b in zip(plain, with_c):
            assert {k: v for k, v in b.items() if k != "correction"} == a
            if not a["surah"]:
                assert b["correction"]["errors"] == [] and b["correction"]["flags"] & cr.NO_TARGET
        tb = eng.tables
        T = 24
        refs = [(112, 2), (112, 1), (112, 3)]
        ids = [tb.token_ids(tb.verse_index(s, a), 1).tolist() for s, a in refs]
        ids[1] = ids[1][:-1]                                       # 112:1 without its last token
        lp = torch.stack([torch.log_softmax(torch.from_numpy(synth_logits(x, T, seed=9 + k, noise=1.0, boost=8.0, rep=1)), -1)
                          for k, x in enumerate(ids)]).cuda().contiguous()
        eng.inject_logprobs(lp, [T] * 3)
        plain = plugin.predict_batch(paths)
        seen = plugin.predict_batch(paths, corrections=True)
        rows = eng.correct_results(batch=3, texts=True)
        both = plugin.predict_batch(paths, words=True, corrections=True)
        words_only = plugin.predict_batch(paths, words=True)
        pre = plugin.predict_batch(paths, corrections=True, prefix=True)
        rows_p = eng.correct_results(batch=3, prefix=True, texts=True)
        monkeypatch.setattr(plugin, "_CORRECTIONS", True)
        one = plugin.predict(paths[1])          # (a clip with at least T frames; a batch of one reads injected row 0)
        eng.inject_logprobs(None)
        assert one["correction"] == seen[0]["correction"]
        assert any(d["surah"] for d in seen) and any(d["correction"]["errors"] for d in seen)
        for b, (a, d, w, wo, pp) in enumerate(zip(plain, seen, both, words_only, pre)):
            assert {k: v for k, v in d.items() if k != "correction"} == a
            assert d["correction"] == correction.fold(tb, rows[b]) == w["correction"]
            assert pp["correction"] == correction.fold(tb, rows_p[b])
            assert [{k: v for k, v in x.items() if k != "status"} for x in w["words"]] == wo["words"]
            if not d["surah"]:
                continue
            c = d["correction"]
            want = cr.correct(rows[b]["pred_codes"].tolist(), rows[b]["ref_codes"].tolist())
            assert c["distance"] == want["info"]["distance"] and len(c["errors"]) == sum(1 for x in want["words"] if x[5])
            status = {(e["ayah"], e["word"]): e["error_type"] for e in c["errors"]}
            assert w["words"] and all(x["status"] == status.get((x["ayah"], x["word"]), "ok") for x in w["words"])
            assert sum(x["status"] != "ok" for x in w["words"]) == len(status)
            for e in c["errors"]:
                assert d["ayah"] <= e["ayah"] <= d["ayah_end"] and e["word"] >= 1
                assert e["error_type"] in ("substitution", "deletion", "insertion") and e["text"]
    finally:
        if plugin._engine is not None:
            plugin._engine.close()
        monkeypatch.setattr(plugin, "_engine", None)
