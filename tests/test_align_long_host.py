"""The host side of the long CTC alignment (include/qverse.h, "word and verse timings for recordings of any length"): the
plan behind the C ABI (csrc/qv_align_long_plan.h), the targets of a run of ayat (Tables.range_token_ids), the folding of an
alignment into verses (words.verses_from_alignment), the binding.  No GPU."""

import ctypes as C

import numpy as np
import pytest

import align_long_ref as A
import align_ref
import long_ref

ERR_ARG, ERR_CAPACITY = 1, 4


@pytest.fixture(scope="module")
def lib():
    import offline_tarteel_amd.engine as E

    return E.load_library()


@pytest.fixture(scope="module")
def tables():
    import offline_tarteel_amd
    from offline_tarteel_amd.tables import Tables

    return Tables(offline_tarteel_amd.TABLES_PATH)


def plan_call(lib, n_samples, n_tokens, max_samples, window=0, margin=-1):
    n = np.asarray(n_samples, np.int64)
    lt = np.asarray(n_tokens, np.int32)
    nw, nbytes = C.c_int32(-5), C.c_int64(-5)
    rc = lib.qv_align_long_plan(n.ctypes.data_as(C.c_void_p), lt.ctypes.data_as(C.c_void_p), len(n), max_samples, window, margin,
                                C.byref(nw), C.byref(nbytes))
    return rc, nw.value, nbytes.value


# ------------------------------------------------------------------ the plan ------------------------------------------------

def test_plan_agrees_with_the_restated_rule_and_the_header_formula(lib):
    cases = [((211000,), (40,), 48000, 0, -1), ((48001, 47360, 130003), (1, 0, 383), 48000, 37 * 1280, 6),
             ((100000,), (2047,), 48000, 37 * 1280, 18), ((9600000, 1280 * 5000), (2048, 4095), 480000, 0, -1),
             ((1280 * 20000,), (4096,), 976000, 0, -1), ((1280 * 112500,), (14403,), 976000, 0, -1),
             ((1280 * 17000, 1280 * 17000 + 5), (8191, 8192), 976000, 0, 0), ((1280 * 17000,), (16383,), 976000, 0, -1),
             ((1280 * 300,), (16384,), 976000, 0, -1)]
    for n, lt, mx, window, margin in cases:
        rc, nw, nbytes = plan_call(lib, n, lt, mx, window, margin)
        plans = [long_ref.plan(v, mx, window, margin) for v in n]
        assert rc == 0 and nw == sum(p.n_windows for p in plans), (n, lt)
        assert nbytes == A.workspace_bytes([p.t_total for p in plans], lt), (n, lt)
    # the formula, spelt out once: 2L + 1 = 28,807 states -> 32 per thread, 901 threads -> 960; 112,501 frames (2.5 hours)
    rc, nw, nbytes = plan_call(lib, (1280 * 112500,), (14403,), 976000)
    assert A.ns_of(14403) == 32 and A.threads_of(14403) == 960
    assert nbytes == ((112501 * 1025 * 4 + 15) & ~15) + 112501 * 960 * 32 // 4 and 1.2e9 < nbytes < 1.4e9
    # too long a target has no back-pointers: the kept rows alone
    assert plan_call(lib, (1280 * 300,), (16384,), 976000)[2] == (301 * 1025 * 4 + 15) & ~15
    assert [A.ns_of(v) for v in (0, 1, 2047, 2048, 4095, 4096, 8191, 8192, 16383, 16384)] == [0, 4, 4, 8, 8, 16, 16, 32, 32, 0]
    assert [A.threads_of(v) for v in (1, 31, 32, 2047, 2048, 16383)] == [64, 64, 64, 1024, 576, 1024]


def test_plan_refuses_what_the_calls_refuse(lib):
    top = long_ref.HOP * long_ref.MAX_FRAMES - 1
    rc, nw, nbytes = plan_call(lib, (top, top), (A.MAX_TOKENS, A.MAX_TOKENS), 976000)
    assert rc == ERR_CAPACITY and nbytes == A.workspace_bytes([long_ref.MAX_FRAMES] * 2, [A.MAX_TOKENS] * 2) > A.MAX_BYTES
    assert plan_call(lib, (top,), (A.MAX_TOKENS,), 976000)[0] == 0                    # one such row fits: 3.2 GB
    assert plan_call(lib, (top + 1,), (5,), 976000) == (ERR_CAPACITY, -5, -5)          # above QV_LONG_MAX_FRAMES: nothing written
    assert plan_call(lib, (100000,), (5,), 48000, 37 * 1280, 19) == (ERR_ARG, -5, -5)  # H < 1
    assert plan_call(lib, (100000,), (5,), 48000, 1000, -1)[0] == ERR_ARG              # not a multiple of 1280
    assert plan_call(lib, (100000,), (-1,), 48000)[0] == ERR_ARG
    assert plan_call(lib, (-1,), (5,), 48000)[0] == ERR_ARG
    n, lt = np.array([100000], np.int64), np.array([5], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.qv_align_long_plan(p(n), p(lt), 0, 48000, 0, -1, None, None) == ERR_ARG  # rows < 1
    assert lib.qv_align_long_plan(None, p(lt), 1, 48000, 0, -1, None, None) == ERR_ARG
    assert lib.qv_align_long_plan(p(n), None, 1, 48000, 0, -1, None, None) == ERR_ARG
    assert lib.qv_align_long_plan(p(n), p(lt), 1, 48000, 0, -1, None, None) == 0        # the outputs are optional


# ------------------------------------------------------------------ targets of a run of ayat --------------------------------

def test_range_token_ids_over_every_surah(tables):
    t = tables
    sizes = []
    for su in range(114):
        start, count = int(t.s["surah_start"][su]), int(t.s["surah_len"][su])
        ids, ends = t.range_token_ids(start, count)
        assert ids.dtype == np.uint16 and len(ends) == count and int(ends[-1]) == len(ids)
        assert (np.diff(np.concatenate(([0], ends))) > 0).all()                        # strictly increasing: no empty verse
        assert int(ids.max()) < 1024
        sizes.append(len(ids))
    assert sorted(sizes)[-5:] == [7110, 8021, 8078, 8937, 14403] and sizes[1] == 14403 <= A.MAX_TOKENS
    # a pair of ayat without a bismillah: the table's own two-ayah token list
    start = t.verse_index(2, 2)
    ids, ends = t.range_token_ids(start, 2)
    assert ids.tolist() == t.token_ids(start, 2).tolist() and ends.tolist() == [len(t.token_ids(start, 1)), len(ids)]
    assert ids[: ends[0]].tolist() == t.token_ids(start, 1).tolist()
    # ... and one WITH a bismillah in its first ayah: the span text strips it, the range keeps it
    start = t.verse_index(2, 1)
    assert int(t.s["nobsm_nw"][start]) > 0
    assert t.range_token_ids(start, 2)[0].tolist() != t.token_ids(start, 2).tolist()
    assert t.range_token_ids(start, 0)[0].tolist() == [] and len(t.range_token_ids(start, 0)[1]) == 0


# ------------------------------------------------------------------ folding -------------------------------------------------

def test_verses_from_alignment_on_a_hand_made_alignment(tables):
    from offline_tarteel_amd.words import FRAME_SECONDS, verses_from_alignment, words_from_alignment

    t = tables
    start = t.verse_index(2, 2)
    verses = [start, start + 1, start + 2]
    ids, ends = t.range_token_ids(start, 3)
    n = len(ids)
    # token i occupies frames 3 + 4i .. 3 + 4i + (i % 3): one to three frames, a gap behind each
    first = 3 + 4 * np.arange(n)
    last = first + np.arange(n) % 3
    logp = -(np.arange(n) % 7 + 1) / 8.0
    al = {"ids": ids.astype(np.int32), "first": first.astype(np.int32), "last": last.astype(np.int32), "logp": logp.astype(np.float32),
          "flags": 0}
    out = verses_from_alignment(t, verses, ends, al)
    assert [(v["surah"], v["ayah"]) for v in out] == [(2, 2), (2, 3), (2, 4)]
    lo = 0
    for v, hi in zip(out, ends.tolist()):
        want = words_from_alignment(t, t.verse_index(v["surah"], v["ayah"]), 1, {k: al[k][lo:hi] for k in ("ids", "first", "last", "logp")})
        assert v["words"] == want and len(want) == int(t.s["clean_nw"][t.verse_index(v["surah"], v["ayah"])])
        assert v["start"] == want[0]["start"] == first[lo] * FRAME_SECONDS and v["end"] == want[-1]["end"] == (last[hi - 1] + 1) * FRAME_SECONDS
        assert [w["word"] for w in want] == list(range(1, len(want) + 1)) and {w["ayah"] for w in want} == {v["ayah"]}
        fr = (last[lo:hi] - first[lo:hi] + 1).astype(np.float64)
        assert abs(v["logp"] - float((logp[lo:hi] * fr).sum() / fr.sum())) < 1e-6
        lo = hi
    # every token once: the words' texts, concatenated, are the texts of the three verses
    text = " ".join(w["text"] for v in out for w in v["words"])
    assert text == " ".join(t.ids_to_text(t.token_ids(x, 1)).strip() for x in verses)
    assert verses_from_alignment(t, verses, ends, dict(al, flags=align_ref.INFEASIBLE)) == []
    assert verses_from_alignment(t, verses, ends, {"ids": ids[:0], "first": first[:0], "last": last[:0], "logp": logp[:0], "flags": 0}) == []
    assert verses_from_alignment(t, verses, ends, None) == []


# ------------------------------------------------------------------ the binding ---------------------------------------------

def test_binding():
    import offline_tarteel_amd.engine as E

    assert {"qv_align_long_plan", "qv_align_windows", "qv_align_long"} <= set(E.exported_symbols())
    lib = E.load_library()
    assert all(hasattr(lib, s) for s in ("qv_align_long_plan", "qv_align_windows", "qv_align_long"))
    assert C.sizeof(E.QvAlignLongInfo) == 24 == E.ALIGN_LONG_INFO_DTYPE.itemsize
    assert [f[0] for f in E.QvAlignLongInfo._fields_] == list(E.ALIGN_LONG_INFO_DTYPE.names)
    assert E.ALIGN_LONG_MAX_TOKENS == A.MAX_TOKENS == 16383 and E.ALIGN_LONG_MAX_BYTES == A.MAX_BYTES == 1 << 32
    for name in ("align_windows_raw", "align_windows", "align_long_raw", "align_long", "align_long_plan"):
        assert callable(getattr(E.Engine, name))


# ------------------------------------------------------------------ the restatement itself ----------------------------------

@pytest.mark.parametrize("L,T,rep", align_ref.PLANTED[:5])
def test_the_long_restatement_equals_the_short_one(L, T, rep):
    ids, lp = align_ref.planted_case(L, T, rep)
    want, got = align_ref.viterbi(lp, ids), A.viterbi(lp, ids)
    assert got["flags"] == want["flags"] == 0 and got["score"].tobytes() == want["score"].tobytes()
    assert got["first"].tolist() == want["first"].tolist() and got["last"].tolist() == want["last"].tolist()
    assert (got["path"] == want["path"]).all() and np.allclose(got["logp"], want["logp"], rtol=T * 2.0 ** -23, atol=0)


def test_the_long_restatement_packs_its_back_pointers_without_changing_a_bit(monkeypatch):
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1024, size=60)
    ids[5] = ids[4]
    lp = (np.round(rng.standard_normal((150, 1025)) * 2) / 4 - 3).astype(np.float32)
    a = A.viterbi(lp, ids, ties=True)
    assert len(a["tie01"]) and len(a["tie12"])
    monkeypatch.setattr(A, "PACK_ABOVE", 0)
    b = A.viterbi(lp, ids)
    assert (a["path"] == b["path"]).all() and a["score"].tobytes() == b["score"].tobytes()
    assert a["first"].tolist() == b["first"].tolist() and a["logp"].tobytes() == b["logp"].tobytes()
