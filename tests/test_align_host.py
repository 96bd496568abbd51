"""Forced alignment, host side (no GPU): the numpy restatement the GPU tests compare the device with (tests/align_ref.py)
against brute force and planted paths, the token -> word -> ayah folding (offline-tarteel_amd/words.py), and the exported ABI."""

import numpy as np
import pytest
import torch

import align_ref
from align_ref import PLANTED, planted_case
from synth import frame_path, hash_noise

@pytest.fixture(scope="module")
def tables():
    import offline_tarteel_amd
    from offline_tarteel_amd.tables import Tables

    return Tables(offline_tarteel_amd.TABLES_PATH)


def test_restatement_equals_brute_force_on_tiny_cases():
    """every (L <= 3, T <= 6) with distinct and with repeated tokens: the Viterbi score is the best score over ALL paths"""
    n = 0
    for L in (1, 2, 3):
        for T in range(1, 7):
            for k, ids in enumerate(([5, 9, 700][:L], [7] * L, [7, 7, 9][:L], [9, 7, 7][:L])):
                lp = torch.log_softmax(torch.from_numpy(hash_noise((T, 1025), seed=31 * L + 7 * T + k) * np.float32(2.0)), -1).numpy()
                got = align_ref.viterbi(lp, ids)
                want = align_ref.brute_force_best(lp, ids)
                if want is None:
                    assert got["flags"] == align_ref.INFEASIBLE, (ids, T)
                    continue
                assert got["flags"] == 0 and got["score"] == want, (ids, T, got["score"], want)
                # the reported path is a path with that score
                ext = [1024] * (2 * L + 1)
                ext[1::2] = ids
                acc = np.float32(lp[0, ext[got["path"][0]]])
                for t in range(1, T):
                    acc = np.float32(acc + lp[t, ext[got["path"][t]]])
                assert acc == want
                n += 1
    assert n >= 50


@pytest.mark.parametrize("L,T,rep", PLANTED)
def test_restatement_recovers_a_planted_path(L, T, rep):
    ids, lp = planted_case(L, T, rep)
    r = align_ref.viterbi(lp, ids)
    assert r["flags"] == 0
    want_first = np.arange(L) * (rep + 1)
    assert r["first"].tolist() == want_first.tolist()
    assert r["last"].tolist() == (want_first + rep - 1).tolist()
    # ... which is synth.frame_path itself wherever the path sits in a token state
    fp = frame_path(ids.tolist(), T, rep)
    tok_frames = r["path"] % 2 == 1
    assert (fp[tok_frames] == ids[r["path"][tok_frames] // 2]).all() and (fp[~tok_frames] == 1024).all()


def test_feasibility_and_flags():
    lp6 = torch.log_softmax(torch.from_numpy(hash_noise((6, 1025), seed=3)), -1).numpy()
    assert align_ref.viterbi(lp6[:5], [7, 7, 7, 9])["flags"] == align_ref.INFEASIBLE     # 4 tokens + 2 forced blanks
    r = align_ref.viterbi(lp6, [7, 7, 7, 9])
    assert r["flags"] == 0 and r["path"].tolist() == [1, 2, 3, 4, 5, 7]
    assert align_ref.viterbi(lp6, [])["flags"] == align_ref.NO_TARGET
    assert align_ref.viterbi(lp6, [1] * 384)["flags"] == align_ref.TOO_LONG


def test_ties_go_to_the_smaller_step():
    """constant log-probs: every path has the same score.  A back-pointer prefers 'stay', so walking back from the final
    state the path stays there as long as that state was reachable: it ENTERS every state as early as possible"""
    lp = np.full((8, 1025), np.float32(-2.0))
    r = align_ref.viterbi(lp, [3, 4])
    assert r["flags"] == 0 and r["score"] == np.float32(-16.0)
    assert r["path"].tolist() == [1, 3, 4, 4, 4, 4, 4, 4]
    assert (r["first"].tolist(), r["last"].tolist()) == ([0, 1], [0, 1])


# ---------------------------------------------------------------- words
def _fake_alignment(ids, frames_per_token=2):
    L = len(ids)
    first = np.arange(L) * (frames_per_token + 1)
    return {"ids": np.asarray(ids), "first": first, "last": first + frames_per_token - 1,
            "logp": -np.arange(1, L + 1, dtype=np.float32) / 8, "flags": 0}


def test_word_and_ayah_counts_over_the_whole_table(tables):
    """word starts (a piece whose surface begins with a space, id != 0) per token list = the table's word counts, for all
    35,717 lists; every list begins with a word start; the ayah split of words_from_alignment adds up"""
    from offline_tarteel_amd.words import ayah_word_counts, words_from_alignment

    starts = np.array([s.startswith(" ") for s in tables.piece_surface])
    starts[0] = False
    tok, off = tables.s["tok"], tables.s["tok_off"]
    n_lists = 0
    for v in range(tables.n_verses):
        for span in range(1, 7):
            ids = tok[off[v * 6 + span - 1]: off[v * 6 + span]]
            if not len(ids):
                continue
            n_lists += 1
            assert starts[ids[0]], (v, span)
            assert int(starts[ids].sum()) == sum(ayah_word_counts(tables, v, span)), (v, span)
    assert n_lists == 35717
    for v, span in ((0, 1), (0, 6), (7, 3), (1, 2), (6230, 2), (293, 4)):   # 7: al-Baqara 1 (bismillah stripped in a span)
        ids = tables.token_ids(v, span)
        words = words_from_alignment(tables, v, span, _fake_alignment(ids))
        counts = ayah_word_counts(tables, v, span)
        assert len(words) == sum(counts)
        a0 = int(tables.ayah[v])
        assert [sum(1 for w in words if w["ayah"] == a0 + j) for j in range(span)] == counts
        for j in range(span):
            assert [w["word"] for w in words if w["ayah"] == a0 + j] == list(range(1, counts[j] + 1))


def test_word_times_are_monotone_and_do_not_overlap(tables):
    from offline_tarteel_amd.words import words_from_alignment

    ids = tables.token_ids(tables.verse_index(2, 255), 1)
    al = _fake_alignment(ids, 3)
    words = words_from_alignment(tables, tables.verse_index(2, 255), 1, al)
    assert words[0]["start"] == 0.0
    for w in words:
        assert w["end"] > w["start"]
    for a, b in zip(words, words[1:]):
        assert b["start"] >= a["end"]
    assert words[-1]["end"] == pytest.approx((int(al["last"][-1]) + 1) * 0.08)
    # (this verse has <unk> pieces, whose surface ' ⁇ ' carries its own spaces: compare modulo runs of spaces)
    assert 0 in ids.tolist()
    assert " ".join(w["text"] for w in words).split() == tables.ids_to_text(ids).split()


def test_hand_written_three_word_case(tables):
    from offline_tarteel_amd.words import words_from_alignment

    sp = [i for i, s in enumerate(tables.piece_surface) if i and s.startswith(" ") and len(s) > 1]
    cont = [i for i, s in enumerate(tables.piece_surface) if i and i < 1024 and s and not s.startswith(" ")]
    a, b, c, x, y = sp[0], sp[1], sp[2], cont[0], cont[1]
    ids = [a, x, 0, b, c, y]                      # word 1 = a x <unk>, word 2 = b, word 3 = c y
    al = {"ids": ids, "first": [0, 2, 5, 9, 12, 20], "last": [1, 3, 5, 10, 12, 24],
          "logp": [-1.0, -2.0, -4.0, -0.5, -0.25, -1.0], "flags": 0}
    words = words_from_alignment(tables, None, 0, al)
    ps = tables.piece_surface
    assert [w["text"] for w in words] == [(ps[a] + ps[x] + ps[0]).strip(), ps[b].strip(), (ps[c] + ps[y]).strip()]
    assert "⁇" in words[0]["text"]
    assert [w["word"] for w in words] == [1, 2, 3] and all(w["ayah"] is None for w in words)
    assert [w["start"] for w in words] == pytest.approx([0.0, 0.72, 0.96])
    assert [w["end"] for w in words] == pytest.approx([0.48, 0.88, 2.0])
    # frame-weighted: (2 * -1 + 2 * -2 + 1 * -4) / 5, -0.5, (1 * -0.25 + 5 * -1) / 6
    assert [w["logp"] for w in words] == pytest.approx([-2.0, -0.5, -5.25 / 6])
    # a flagged or empty alignment has no words
    assert words_from_alignment(tables, None, 0, dict(al, flags=4)) == []
    assert words_from_alignment(tables, 0, 1, {"ids": [], "first": [], "last": [], "logp": [], "flags": 0}) == []


def test_alignment_symbols_are_exported_and_bound():
    import ctypes

    import offline_tarteel_amd
    from offline_tarteel_amd import engine as E

    assert {"qv_align", "qv_align_results_ctx"} <= set(E.exported_symbols())
    h = ctypes.CDLL(str(offline_tarteel_amd.LIB_PATH))
    assert hasattr(h, "qv_align") and hasattr(h, "qv_align_results_ctx")
    assert ctypes.sizeof(E.QvAlignInfo) == 32 == E.ALIGN_INFO_DTYPE.itemsize
    hdr = (offline_tarteel_amd.LIB_PATH.parent.parent / "include" / "qverse.h").read_text()
    assert f"#define QV_ALIGN_MAX_TOKENS {E.ALIGN_MAX_TOKENS}" in hdr
