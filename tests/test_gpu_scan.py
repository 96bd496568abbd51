"""Exhaustive CTC scan (csrc/qv_scan.hip: k_ctc_scan, k_scan_select; include/qverse.h qv_scan_logprobs / qv_scan_batch) on the
MI355X.

What every case is held to:
 (a) loss_out is BIT-equal to qv_debug_ctc_loss (the parent commit's kernel, one recursion per target) on the same targets:
     every key where a row has at most 3,000 of them, else a seeded sample of 512 plus every target of more than 256 states;
     every key that is not feasible holds +inf;
 (b) |loss - float64 torch| <= 1e-3 for T <= 126, the project's CTC bound (tests/test_gpu_postlogits.py).  For T = 376 and
     T = 766 that absolute bound does not hold for torch's own float32 either (1.0e-2 on losses near 5.4e3 at T = 766): there
     the gap of qv_debug_ctc_loss to float64 on the same targets, measured on the MI355X, is the yardstick -- LONG_GAP below --
     and the scan must stay within twice that (by (a) it has the same gap);
 (c) the entries equal tests/scan_ref.py::rank applied to the device's own loss_out, exactly, in every field, and n_feasible
     / n_recursions equal the counts made from the tables (tests/test_scan_host.py pins those against qv_scan_stats);
 (d) the planted verse is entry 0.
Log-probs: log_softmax of seeded continuous noise with the greedy path of one verse boosted, so the top is separated."""
import ctypes as C

import numpy as np
import pytest
import torch

import scan_ref as R
from synth import BLANK, VOCAB, frame_path, synth_audio

pytestmark = pytest.mark.gpu

SHORT_TOL = 1e-3
# measured on the MI355X: max |qv_debug_ctc_loss - float64 torch| over the case's targets and log-probs -- T = 376, surah 65
# (33 targets, losses up to 1,963): 2.892e-3; T = 766, surah 65 (56 targets, losses up to 4,017): 9.868e-3
LONG_GAP = {376: 2.892e-3, 766: 9.868e-3}


def make_lp(tables, verse, span, T, seed, boost=12.0):
    """(boost 12 over unit noise on 1,025 classes: the path's frames cost about 0.01 each, so no longer verse that shares the
    planted one's first tokens overtakes it under the division by L)"""
    lg = np.random.default_rng(seed).standard_normal((T, VOCAB)).astype(np.float32)
    if T:
        lg[np.arange(T), frame_path(tables.token_ids(verse, span), T, 2)] += np.float32(boost)
    x = lg.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))).astype(np.float32)


def batch_of(lps, t_max=None):
    t_max = t_max or max(max(len(x) for x in lps), 1)
    out = np.full((len(lps), t_max, VOCAB), np.nan, np.float32)      # rows t >= t[b] are never read: NaN would show
    for b, x in enumerate(lps):
        out[b, : len(x)] = x
    return torch.from_numpy(out).cuda().contiguous(), [len(x) for x in lps]


@pytest.fixture(scope="module")
def eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=4, max_samples=16000 * 61 + 4000)   # 766 frames
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(eng):
    return eng.tables


@pytest.fixture(scope="module")
def chains(tables):
    return R.chain_ids(tables)


def check_row(eng, tables, chains, lp_dev, b, T, info, ent, losses, k, max_span, penalty, surahs, planted, tag, f64_tol):
    """one row of a scan against (a) .. (d); returns the measured gaps"""
    key, v, sp, L = R.keys(tables, T, max_span, surahs)
    want = R.stats(tables, chains, T, max_span, surahs)
    assert (int(info["n_feasible"]), int(info["n_recursions"]), int(info["t_frames"])) == (want["n_feasible"], want["n_recursions"], T), tag
    assert int(info["n_entries"]) == min(k, len(key)), tag
    row = losses[b].cpu().numpy()
    # everything that is not a feasible key holds +inf
    rest = np.ones(len(row), bool)
    rest[key] = False
    assert np.all(np.isposinf(row[rest])) and np.all(np.isfinite(row[key])), tag
    gaps = {}
    if len(key):
        # (a) bit-equality with the parent's kernel
        if len(key) <= 3000:
            pick = np.arange(len(key))
        else:
            pick = np.union1d(np.random.default_rng(5).choice(len(key), 512, replace=False), np.flatnonzero(2 * L + 1 > 256))
        ids = [tables.token_ids(int(v[i]), int(sp[i])) for i in pick]
        dbg = eng.debug_ctc_loss(lp_dev[b, :T], ids)
        assert dbg.tobytes() == row[key[pick]].tobytes(), (tag, int(np.sum(dbg != row[key[pick]])))
        # (b) against float64
        f64 = R.losses64(lp_dev[b, :T].cpu().numpy(), tables, key[pick])
        gaps = {"scan": float(np.abs(row[key[pick]].astype(np.float64) - f64).max()),
                "debug": float(np.abs(dbg.astype(np.float64) - f64).max()), "max_loss": float(f64.max()), "n": len(pick)}
        print(f"{tag}: {len(key)} keys, {len(pick)} compared, max loss {gaps['max_loss']:.1f}, |scan - f64| {gaps['scan']:.3e}, "
              f"|qv_debug_ctc_loss - f64| {gaps['debug']:.3e}, bound {f64_tol:.3e}")
        assert gaps["scan"] <= f64_tol, (tag, gaps)
    # (c) the entries are the restatement's ranking of the device's own losses
    top = R.rank(row[key], L, sp, penalty, k)
    norm, fin = R.finals(row[key], L, sp, penalty)
    got = ent[: len(top)]
    for name, arr in (("start_verse", v[top]), ("span", sp[top]), ("surah", np.asarray(tables.surah)[v[top]]),
                      ("ayah", np.asarray(tables.ayah)[v[top]]), ("ayah_end", np.asarray(tables.ayah)[v[top]].astype(np.int64) + sp[top] - 1),
                      ("n_tokens", L[top])):
        assert got[name].tolist() == np.asarray(arr).astype(np.int64).tolist(), (tag, name)
    assert got["loss"].tobytes() == row[key][top].tobytes() and got["norm"].tobytes() == norm[top].tobytes(), tag
    assert got["final_score"].tobytes() == fin[top].tobytes(), tag
    assert not ent[len(top):].tobytes().strip(b"\0"), tag                # entries past n_entries are zeroed
    # (d)
    if planted is not None:
        assert (int(ent[0]["start_verse"]), int(ent[0]["span"])) == planted, tag
    return gaps


def test_whole_table_on_a_ragged_batch_with_an_empty_row(eng, tables, chains):
    v33, v17 = tables.verse_index(112, 1), tables.verse_index(1, 1)
    assert 3 * len(tables.token_ids(v33, 1)) <= 33 and 3 * len(tables.token_ids(v17, 1)) <= 17
    lps = [make_lp(tables, v33, 1, 33, 11), make_lp(tables, v17, 1, 17, 12), make_lp(tables, 0, 1, 0, 13)]
    dev, t = batch_of(lps, 33)
    assert t == [33, 17, 0]
    info, ent, losses = eng.scan_raw(dev, t, k=5, max_span=6, span_penalty=0.5, return_losses=True)
    assert info["n_feasible"].tolist() == [len(R.keys(tables, T)[0]) for T in t] and info["n_feasible"][2] == 0 < info["n_feasible"][1]
    for b, planted in enumerate(((v33, 1), (v17, 1), None)):
        check_row(eng, tables, chains, dev, b, t[b], info[b], ent[b], losses, 5, 6, 0.5, None, planted, ("ragged", b), SHORT_TOL)
    assert int(info[2]["n_entries"]) == 0 and int(info[2]["n_recursions"]) == 0
    # the bits of a row do not depend on the batch it travels in, nor on whether the losses are asked for
    one, t1 = batch_of([lps[1]])
    info1, ent1, _ = eng.scan_raw(one, t1, k=5, max_span=6, span_penalty=0.5)
    assert info1[0].tobytes() == info[1].tobytes() and ent1[0].tobytes() == ent[1].tobytes()
    # the dict form
    rows = eng.scan_logprobs(dev, t, k=5, span_penalty=0.5, return_losses=True)
    assert [r["n_feasible"] for r in rows] == info["n_feasible"].tolist() and rows[2]["candidates"] == []
    first = rows[0]["candidates"][0]
    assert (first["surah"], first["ayah"], first["ayah_end"], first["span"]) == (112, 1, 1, 1)
    assert first["final_score"] == float(ent[0, 0]["final_score"]) and torch.equal(rows[0]["losses"], losses[0])
    # span_penalty None: the engine's CTC_DIRECT_SPAN_PENALTY
    assert eng.scan_raw(dev, t, k=5)[1].tobytes() == eng.scan_raw(dev, t, k=5, span_penalty=float(eng.cfg.span_penalty))[1].tobytes()


@pytest.mark.parametrize("T, surahs, verse, span", [(126, [1, 36, 112, 113, 114], (36, 1), 2), (376, [65], (65, 2), 1)])
def test_every_wave_width(eng, tables, chains, T, surahs, verse, span):
    """targets of 2 .. 62 tokens at T = 126 (ctc_wave2<1, 2>), up to 187 at T = 376 (<3, 4, 6>); spans read out as prefixes"""
    v = tables.verse_index(*verse)
    key, _, _, L = R.keys(tables, T, 6, surahs)
    if T == 126:
        assert len(key) == 279 and (L.min(), L.max()) == (2, 62)
    else:
        assert 2 * L.max() + 1 > 256 and np.any((2 * L + 1 > 128) & (2 * L + 1 <= 192)) and np.any((2 * L + 1 > 192) & (2 * L + 1 <= 256))
    dev, t = batch_of([make_lp(tables, v, span, T, 20 + T)])
    for max_span in (6, 2):
        info, ent, losses = eng.scan_raw(dev, t, k=8, max_span=max_span, span_penalty=0.5, surahs=surahs, return_losses=True)
        check_row(eng, tables, chains, dev, 0, T, info[0], ent[0], losses, 8, max_span, 0.5, surahs, (v, span), (T, max_span),
                  SHORT_TOL if T <= 126 else 2 * LONG_GAP[T])


def test_long_targets(eng, tables, chains):
    """T = 766, surah 65: 56 keys, 12 of more than 256 tokens, the longest 371 -- the wide wave programs, up to 743 states"""
    T, surahs = 766, [65]
    key, _, _, L = R.keys(tables, T, 6, surahs)
    assert len(key) == 56 and int((L > 256).sum()) == 12 and L.max() == 371 and np.any((2 * L + 1 > 384) & (2 * L + 1 <= 512))
    v = tables.verse_index(65, 1)
    dev, t = batch_of([make_lp(tables, v, 2, T, 31)])
    info, ent, losses = eng.scan_raw(dev, t, k=32, max_span=6, span_penalty=0.5, surahs=surahs, return_losses=True)
    check_row(eng, tables, chains, dev, 0, T, info[0], ent[0], losses, 32, 6, 0.5, surahs, (v, 2), "long", 2 * LONG_GAP[T])


def test_ties_go_to_the_smaller_verse_and_k_clips(eng, tables, chains):
    """surahs 55 and 77 repeat a verse 31 and 10 times: identical targets, bit-identical losses, exact ties"""
    T, surahs = 96, [55, 77]
    v = tables.verse_index(55, 13)
    same = [u for u in range(tables.n_verses) if int(tables.surah[u]) == 55 and
            np.array_equal(tables.token_ids(u, 1), tables.token_ids(v, 1))]
    assert same[0] == v and len(same) == 31 and 3 * len(tables.token_ids(v, 1)) <= T
    dev, t = batch_of([make_lp(tables, v, 1, T, 41)])
    for penalty in (0.0, 0.5):
        info, ent, losses = eng.scan_raw(dev, t, k=32, max_span=6, span_penalty=penalty, surahs=surahs, return_losses=True)
        check_row(eng, tables, chains, dev, 0, T, info[0], ent[0], losses, 32, 6, penalty, surahs, (v, 1), ("ties", penalty), SHORT_TOL)
        assert ent["start_verse"][0, :31].tolist() == same and len(set(ent["final_score"][0, :31].tolist())) == 1
    # k above the number of feasible keys: all of them, the rest zeroed
    info, ent, losses = eng.scan_raw(dev, [9], k=32, max_span=6, span_penalty=0.5, surahs=surahs, return_losses=True)
    n = len(R.keys(tables, 9, 6, surahs)[0])
    assert 0 < n < 32 and int(info[0]["n_entries"]) == n
    check_row(eng, tables, chains, dev, 0, 9, info[0], ent[0], losses, 32, 6, 0.5, surahs, None, "clip", SHORT_TOL)


def test_masks_are_per_row(eng, tables, chains):
    v = tables.verse_index(114, 1)
    lp = make_lp(tables, v, 1, 64, 51)
    dev, t = batch_of([lp, lp, lp])
    masks = [[114], [1, 2], None]
    info, ent, losses = eng.scan_raw(dev, t, k=4, max_span=6, span_penalty=0.5, surahs=masks, return_losses=True)
    for b, (m, planted) in enumerate(zip(masks, ((v, 1), None, (v, 1)))):
        check_row(eng, tables, chains, dev, b, 64, info[b], ent[b], losses, 4, 6, 0.5, m, planted, ("mask", b), SHORT_TOL)
    assert set(ent["surah"][1].tolist()) <= {1, 2} and int(info[0]["n_feasible"]) < int(info[1]["n_feasible"]) < int(info[2]["n_feasible"])
    # a key scored under two masks has one loss
    k114 = R.keys(tables, 64, 6, [114])[0]
    assert torch.equal(losses[0, k114], losses[2, k114])
    # one list of surah numbers applies to every row
    same = eng.scan_raw(dev, t, k=4, span_penalty=0.5, surahs=[114])[1]
    assert same[1].tobytes() == same[0].tobytes() == ent[0].tobytes()


def test_bad_arguments_are_refused(eng, tables):
    dev, frames = batch_of([make_lp(tables, 0, 1, 20, 61), make_lp(tables, 1, 1, 12, 62)])
    B, t_max = 2, dev.shape[1]
    info = np.zeros(B, dtype=[("a", "<i4", 4)])
    ent = np.zeros((B, 32), dtype=[("a", "u1", 40)])
    t = np.asarray(frames, np.int32)
    mask = np.full((B, 4), 0xFFFFFFFF, np.uint32)
    zero = mask.copy()
    zero[1] = 0
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    lpp = C.c_void_p(dev.data_ptr())

    def call(lp=lpp, t_=t, batch=B, tm=t_max, span=6, pen=0.5, k=5, mask_=None, info_=info, ent_=ent):
        return eng.lib.qv_scan_logprobs(eng.h, lp, p(t_), batch, tm, span, pen, k, p(mask_), p(info_), p(ent_), None, eng._stream())

    assert call() == 0 and call(k=32) == 0 and call(k=1, span=1) == 0 and call(mask_=mask) == 0
    for bad in (dict(lp=None), dict(t_=None), dict(info_=None), dict(ent_=None), dict(batch=0), dict(tm=0), dict(span=0), dict(span=7),
                dict(k=0), dict(k=33), dict(mask_=zero), dict(t_=np.asarray([frames[0], t_max + 1], np.int32)),
                dict(t_=np.asarray([-1, frames[1]], np.int32))):
        assert call(**bad) == 1, bad                                   # QV_ERR_ARG
        assert eng.lib.qv_last_error(eng.h)
    wide = np.zeros(5, np.int32)
    assert call(t_=wide, batch=5, info_=np.zeros(5, info.dtype), ent_=np.zeros((5, 32), ent.dtype)) == 4   # QV_ERR_CAPACITY
    assert call(tm=769) == 4                                           # 766 + 2 frames: the engine's capacity
    assert eng.lib.qv_scan_logprobs(None, lpp, p(t), B, t_max, 6, 0.5, 5, None, p(info), p(ent), None, None) == 1
    with pytest.raises(ValueError):
        eng.scan_logprobs(dev, frames, surahs=[0])
    assert call() == 0                                                 # and the engine still works


def test_scan_batch_and_the_opt_in_fallback(tables, monkeypatch):
    from offline_tarteel_amd import plugin
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=64000)
    try:
        audio = torch.from_numpy(synth_audio(2, 32000)).cuda()
        lens = [32000, 24000]
        # the scan behind the forward is the scan of the forward's log-probs
        rows = e.scan_batch(audio, lens, k=3, surahs=[[112, 113, 114], None])
        lp, T = e.forward(audio, lens)
        assert rows == e.scan_logprobs(lp.contiguous(), T, k=3, surahs=[[112, 113, 114], None])
        assert [r["t_frames"] for r in rows] == list(T) and rows[0]["candidates"] and rows[0]["candidates"][0]["surah"] in (112, 113, 114)

        monkeypatch.setattr(plugin, "_engine", e)
        monkeypatch.delenv("QVERSE_SCAN_FALLBACK", raising=False)
        monkeypatch.delenv("QVERSE_TRIE_FALLBACK", raising=False)
        base = plugin._finish(e, e.predict_batch(audio, lens), True, False, None)
        assert plugin.predict_device(audio, lens) == base and not plugin.scan_fallback_enabled()
        # set: rows that have a prediction stay as they are
        monkeypatch.setenv("QVERSE_SCAN_FALLBACK", "1")
        with_pred = [r for r in base if r["surah"]]
        assert plugin.scan_fallback_enabled() and [r for r in plugin.predict_device(audio, lens) if r["surah"]] == with_pred
        # ... and a row without one is given to the scan.  Injected: the batch comes back with two empty transcripts; the
        # log-probs the scan sees spell 1:1 for row 0 and are too short for any verse for row 1
        real = e.predict_batch(audio, lens)
        empty = [dict(r, surah=0, ayah=0, ayah_end=None, score=0.0, source=None, flags=1, transcript="", greedy_ids=[]) for r in real]
        spelled = {0: make_lp(tables, 0, 1, 40, 71), 1: make_lp(tables, 0, 1, 2, 72)}
        asked, beamed = [], []

        def scan_batch(rows_, ln, **kw):
            asked.append((tuple(rows_.shape), list(ln)))
            return [e.scan_logprobs(*batch_of([spelled[i]]), **kw)[0] for i in range(len(ln))]

        def beam_batch(rows_, ln, **kw):
            beamed.append(list(ln))
            return [{"hypotheses": []} for _ in ln]

        monkeypatch.setattr(e, "predict_batch", lambda *a, **kw: [dict(r) for r in empty])
        monkeypatch.setattr(e, "scan_batch", scan_batch)
        monkeypatch.setattr(e, "beam_batch", beam_batch)
        got = plugin.predict_device(audio, lens)
        assert asked == [((2, 32000), lens)] and not beamed
        want = e.scan_logprobs(*batch_of([spelled[0]]), k=1)[0]["candidates"][0]
        assert (want["surah"], want["ayah"], want["ayah_end"]) == (1, 1, 1)
        assert got[0] == {"surah": 1, "ayah": 1, "ayah_end": 1, "score": round(float(np.exp(-np.float64(want["norm"]))), 4),
                          "transcript": "", "source": "scan", "candidates": []}   # (the empty row's own keys stay, as on the trie route)
        assert 0.0 < got[0]["score"] <= 1.0
        assert got[1] == plugin._empty("")                              # nothing feasible: still no prediction
        # with the trie route set as well the scan runs first and only the rows it left empty go on
        monkeypatch.setenv("QVERSE_TRIE_FALLBACK", "1")
        assert plugin.predict_device(audio, lens) == got and beamed == [[lens[1]]]
        monkeypatch.delenv("QVERSE_TRIE_FALLBACK")
        monkeypatch.delenv("QVERSE_SCAN_FALLBACK")
        assert plugin.predict_device(audio, lens) == [plugin._empty(""), plugin._empty("")] and len(asked) == 2
    finally:
        e.close()
    e = Engine(device=0, with_model=False, max_batch=2, max_samples=32000)
    try:
        with pytest.raises(Exception, match=r"\(5\)"):                # QV_ERR_NO_MODEL
            e.scan_batch(audio, lens)
    finally:
        e.close()
