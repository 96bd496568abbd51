"""The premises of tests/test_gpu_decode.py, checked without a GPU: every builder of tests/decode_cases.py produces what it
says (winners, positions, lengths, frame counts), the per-piece code route the kernel takes equals the text route of the
reference on every case, and the cases have the power to tell a subtly wrong decode from a right one -- shown with two
deliberately wrong HOST restatements, never a kernel."""

import numpy as np
import pytest

import decode_cases as D
from synth import BLANK, VOCAB


@pytest.fixture(scope="module")
def pc(oracle):
    return D.Pieces(oracle)


@pytest.fixture(scope="module")
def tables():
    from offline_tarteel_amd import TABLES_PATH
    from offline_tarteel_amd.tables import Tables

    return Tables(TABLES_PATH)


@pytest.fixture(scope="module")
def cases(oracle):
    return D.build_cases(oracle)


@pytest.fixture(scope="module")
def refs(oracle, tables, cases):
    return {name: D.reference_of(oracle, tables.encode, lp, T) for name, lp, T in cases}


def test_vocabulary_material_is_what_the_builders_assume(oracle, pc, tables):
    assert pc.codes[D.UNK].tolist() == [0, 63, 0] and oracle.piece_surface[D.UNK] == " ⁇ "
    assert pc.codes[D.SPACE].tolist() == [0] and oracle.piece_surface[D.SPACE] == " "
    assert tuple(i for i in range(1024) if pc.len[i] == 0) == D.EMPTY_PIECES
    assert sum(1 for i in range(1024) if pc.len[i] and pc.codes[i][0] == 0) == 534
    assert pc.len[:1024].min() == 0 and pc.len[:1024].max() == 9 and pc.len[BLANK] == 0
    assert len(pc.fillers) >= 3
    # the raw-overflow row and the 2,049-character text need two distinct pieces of at least 6 codes
    a, b = pc.spaced[0], pc.spaced[1]
    assert a != b and pc.len[a] >= 6 and pc.len[b] >= 6
    # the product's table reader and the oracle's agree on the codes of a text
    s = "".join(oracle.alphabet) + " x⁇"
    assert tables.encode(s).tolist() == oracle.encode(s).tolist()


def test_argmax_frames_have_the_winner_they_name():
    frames = D.argmax_frames()
    tags = [t for t, _, _ in frames]
    assert sum(t.startswith("unique") for t in tags) == 5 + 32 and sum(t.startswith("tie") for t in tags) == 7
    for tag, f, want in frames:
        assert f.dtype == np.float32 and f.shape == (VOCAB,) and not np.isnan(f).any()
        assert int(np.argmax(f)) == want, tag
        assert D.argmax_first(f) == want, tag
        if tag.startswith("unique"):
            assert (f == f.max()).sum() == 1, tag
    # the ties are exact, and the signed zeros compare equal
    for (idx, win), (tag, f, _) in zip(D.TIES, [x for x in frames if x[0].startswith("tie")]):
        assert sorted(np.flatnonzero(f == f.max()).tolist()) == sorted(idx) and win == min(idx), tag
    assert (dict((t, f) for t, f, _ in frames)["all equal"] == np.float32(-6.9324)).all()
    z = dict((t, f) for t, f, _ in frames)["-0.0 at 3, +0.0 at 700"]
    assert np.signbit(z[3]) and not np.signbit(z[700]) and z[3] == z[700] == 0 and (np.delete(z, [3, 700]) < 0).all()
    z = dict((t, f) for t, f, _ in frames)["+0.0 at 3, -0.0 at 2"]
    assert np.signbit(z[2]) and not np.signbit(z[3]) and (np.delete(z, [2, 3]) < 0).all()
    # the -inf rows
    one = np.full(VOCAB, -np.inf, np.float32)
    one[77] = -0.25
    assert D.argmax_first(one) == int(np.argmax(one)) == 77
    assert D.argmax_first(np.full(VOCAB, -np.inf, np.float32)) == int(np.argmax(np.full(VOCAB, -np.inf, np.float32))) == 0


def test_ordinary_frames_are_decided_by_the_boost():
    ids = [0, 5, BLANK, 1023, 5, 5, BLANK]
    lp = D.frames_of(ids, 3)
    assert lp.dtype == np.float32 and lp.argmax(-1).tolist() == ids
    top2 = np.sort(lp, axis=-1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] >= float(D.BOOST) - 2 * D.NOISE_BOUND - 1e-3).all()
    assert np.allclose(np.exp(lp.astype(np.float64)).sum(-1), 1.0, atol=1e-5)


def test_no_case_feeds_what_the_kernels_cannot_take(cases):
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names)
    for name, lp, T in cases:
        assert lp.dtype == np.float32 and lp.shape == (T, VOCAB) and not np.isnan(lp).any(), name
        assert 0 <= T <= D.T_FULL, name
        assert not lp.flags.writeable
    assert set(D.LONG_TEXT_CASES) <= set(names)


def test_the_argmax_rows_show_every_frames_winner(cases, refs):
    by = {n: (lp, T) for n, lp, T in cases}
    frames = D.argmax_frames()
    lp, T = by["argmax unique"]
    want = [w for t, _, w in frames if t.startswith("unique")]
    assert lp.argmax(-1).tolist() == want and refs["argmax unique"]["ids"] == [w for w in want if w != BLANK]
    assert all(a != b for a, b in zip(want, want[1:]))            # no two neighbours merge
    lp, T = by["argmax ties"]
    want = [w for t, _, w in frames if not t.startswith("unique")]
    assert lp.argmax(-1).tolist()[::2] == want and set(lp.argmax(-1).tolist()[1::2]) == {BLANK}
    assert refs["argmax ties"]["ids"] == want == [5, 5, 63, 6, 0, 1023, 960, 0, 3, 2]
    assert refs["-inf but one"]["ids"] == [int(np.argmax(by["-inf but one"][0][0]))] and by["-inf but one"][1] == 1
    assert refs["-inf everywhere"]["ids"] == [0] and refs["-inf everywhere"]["codes"].tolist() == [63]


def test_collapse_rows_cross_the_chunk_boundaries(cases, refs, pc):
    by = {n: (lp, T) for n, lp, T in cases}
    f1, f2, f3 = pc.fillers[:3]
    fid = by["merge across 63|64 and 127|128"][0].argmax(-1)
    assert fid[63] == fid[64] == f1 and fid[127] == fid[128] == f2 and refs["merge across 63|64 and 127|128"]["ids"] == [f1, f2]
    for s in (62, 63):
        name = f"id blank id from {s} and {s + 64}"
        fid = by[name][0].argmax(-1)
        assert fid[s: s + 3].tolist() == [f1, BLANK, f1] and fid[s + 64: s + 67].tolist() == [f2, BLANK, f2]
        assert refs[name]["ids"] == [f3, f1, f1, f2, f2, f3]
    assert by["T=1 token"][1] == 1 and refs["T=1 token"]["ids"] == [f2]
    assert by["T=1 blank"][1] == 1 and refs["T=1 blank"]["ids"] == [] and refs["T=1 blank"]["text"] == ""
    assert by["T=0"][1] == 0 and refs["T=0"]["ids"] == []
    assert len(refs["65 tokens"]["ids"]) == 65 and len(refs["129 tokens"]["ids"]) == 129
    lp, T = by["T=768"]
    fid = lp.argmax(-1)
    assert T == D.T_FULL == 768 and fid[767] != BLANK and fid[767] != fid[766]     # the last frame of the row is a token of its own
    assert 0 < len(refs["T=768"]["text"]) <= 1024


def test_expansion_rows_hold_what_they_name(cases, refs, pc):
    by = {n: (lp, T) for n, lp, T in cases}
    r = refs["only empty pieces"]
    assert len(r["ids"]) == 5 and r["text"] == "" and D.expected_flags(r, pc, 1024) == 1
    assert refs["only id 10"]["ids"] == [D.SPACE] and refs["only id 10"]["text"] == ""
    r = refs["id 10 leading trailing doubled"]
    assert r["ids"][0] == r["ids"][-1] == D.SPACE and r["ids"][2:4] == [D.SPACE, D.SPACE] and r["words"] == 3
    assert "  " not in r["text"] and r["text"] == r["text"].strip()
    r = refs["id 0 start middle end doubled"]
    assert r["ids"][0] == r["ids"][-1] == D.UNK and r["ids"][5:7] == [D.UNK, D.UNK]
    assert r["codes"].tolist().count(63) == 5 and r["codes"][0] == 63 and r["codes"][-1] == 63 and r["words"] == 8
    r = refs["empty piece between letters"]
    assert len(r["text"]) == 3 and " " not in r["text"] and r["words"] == 1 and len(r["ids"]) == 6
    r = refs["leading-space piece after id 10"]
    raw = pc.raw(r["ids"])
    assert raw[1] == 0 and raw[2] == 0 and "  " not in r["text"] and r["words"] == 3
    # the space runs sit where the whitespace pass changes chunk
    r = refs["space runs across raw 63|64 and 127|128"]
    raw = pc.raw(r["ids"])
    assert raw[62] != 0 and raw[63] == raw[64] == 0 and raw[65] != 0
    assert raw[125] != 0 and raw[126] == raw[127] == raw[128] == 0 and raw[129] != 0
    assert "  " not in r["text"] and r["words"] == 3
    # exact lengths, frame counts, and no blank between different ids
    for n in (1024, 1025, 2048, 2049):
        r, (lp, T) = refs[f"{n} characters"], by[f"{n} characters"]
        assert len(r["text"]) == len(r["codes"]) == n and T <= D.T_TEXT_MAX and len(r["ids"]) == T
        assert len(pc.raw(r["ids"])) <= D.RAW_CAP
        assert D.expected_flags(r, pc, 1024) == (2 if n > 1024 else 0) and D.expected_flags(r, pc, 2048) == (2 if n > 2048 else 0)
    r, (lp, T) = refs["raw overflow"], by["raw overflow"]
    assert T <= D.T_TEXT_MAX and len(pc.raw(r["ids"])) > D.RAW_CAP and len(set(r["ids"])) == 2
    assert D.expected_flags(r, pc, 2048) == 2


def test_per_piece_codes_and_a_collapse_equal_the_text_route(oracle, tables, pc, cases, refs):
    """the kernel's route (argmax, collapse, per-piece codes, whitespace collapse and strip, restated in numpy) against the
    reference's route through the text, on every case and on 300 random id strings"""
    for name, lp, T in cases:
        got, want = D.decode_host(pc, lp, T), refs[name]
        assert got["ids"] == want["ids"], name
        assert got["codes"].tobytes() == want["codes"].tobytes(), name
        assert got["words"] == want["words"], name
    from oracle.oracle import normalize_arabic

    rng = np.random.default_rng(3000)
    for _ in range(300):
        ids = rng.integers(0, 1024, size=int(rng.integers(1, 40))).tolist()
        text = normalize_arabic(oracle.ids_to_text(ids).strip())
        raw = pc.raw(ids)
        keep = [c for i, c in enumerate(raw.tolist()) if c != 0 or (i > 0 and raw[i - 1] != 0 and raw[i + 1:].any())]
        assert bytes(keep) == tables.encode(text).tobytes(), ids


def test_a_last_maximum_argmax_fails_the_tie_frames(pc, cases, refs):
    """power of the tie frames: a restatement that takes the LAST maximum is caught, and by the tie rows only"""
    failed = {name for name, lp, T in cases if D.decode_host(pc, lp, T, argmax=D.argmax_last)["ids"] != refs[name]["ids"]}
    assert failed == {"argmax ties", "-inf everywhere"}
    for tag, f, want in D.argmax_frames():
        if tag.startswith("unique"):
            assert D.argmax_last(f) == want, tag
        else:
            assert D.argmax_last(f) != want, tag


def test_a_collapse_that_forgets_prev_at_chunk_starts_fails_the_straddling_rows(pc, cases, refs):
    """power of the collapse rows: resetting `prev` every 64 frames repeats the token that runs across a chunk boundary"""
    failed = {name for name, lp, T in cases
              if D.decode_host(pc, lp, T, reset_prev_every=64)["ids"] != refs[name]["ids"]}
    assert "merge across 63|64 and 127|128" in failed
    got = D.decode_host(pc, *[(lp, T) for n, lp, T in cases if n == "merge across 63|64 and 127|128"][0], reset_prev_every=64)
    f1, f2 = pc.fillers[:2]
    assert got["ids"] == [f1, f1, f2, f2]
    # rows that do not run a token across a boundary are untouched by the defect
    assert not failed & {"argmax unique", "T=1 token", "only id 10", "id blank id from 62 and 126"}
