"""Premises of tests/test_gpu_transcribe.py, on the CPU: the numpy restatement of the transcription contract
(tests/transcribe_ref.py) agrees with the oracle's greedy decode on every decode case, and the inputs tell the restatement
from its two deliberately wrong variants (token log-prob at the run's first frame; a sequential sum)."""

import numpy as np
import pytest

import decode_cases as D
import transcribe_ref as R


@pytest.fixture(scope="module")
def cases(oracle):
    return D.build_cases(oracle)


@pytest.fixture(scope="module")
def refs(cases):
    return {name: R.transcribe_ref(lp, T) for name, lp, T in cases}


def test_restated_ids_equal_the_oracles_greedy_ids(oracle, cases, refs):
    for name, lp, T in cases:
        want = oracle.greedy_ids(lp[:T]) if T else []
        assert refs[name]["ids"] == [int(i) for i in want], name


def test_restatement_is_consistent_with_its_definitions(cases, refs):
    seen_empty = seen_inf = False
    for name, lp, T in cases:
        r = refs[name]
        assert r["t_frames"] == T and r["n_tokens"] == len(r["ids"]) == len(r["first"]) == len(r["last"]) == len(r["logp"]), name
        for i, a, e, p in zip(r["ids"], r["first"], r["last"], r["logp"]):
            assert 0 <= a <= e < T and i != R.BLANK, name
            assert (r["fid"][a: e + 1] == i).all(), name
            assert (a == 0 or r["fid"][a - 1] != i) and (e == T - 1 or r["fid"][e + 1] != i), name
            assert p == r["m"][a: e + 1].max(), name
        assert r["flags"] == (0 if r["ids"] else R.FLAG_EMPTY), name
        if not r["ids"]:
            seen_empty = True
            assert r["avg_logprob"] == 0.0 and r["min_token_logprob"] == 0.0, name
        if T == 0:
            assert r["frame_avg_logprob"] == 0.0, name
        if name == "-inf everywhere":
            seen_inf = True
            assert r["ids"] == [0] and np.isneginf(r["logp"][0]) and np.isneginf(r["avg_logprob"]) and np.isneginf(r["frame_avg_logprob"])
    assert seen_empty and seen_inf


def test_the_cases_tell_the_run_maximum_from_the_first_frame(cases, refs):
    """a token that lasts several frames has its best frame somewhere in the run: taking the first frame is a different
    number on at least one case (any multi-frame run of frames_of does it)"""
    differing = 0
    for name, lp, T in cases:
        wrong = R.transcribe_ref(lp, T, logp="first")
        assert wrong["ids"] == refs[name]["ids"], name
        if R.bits32(wrong["logp"]) != R.bits32(refs[name]["logp"]):
            differing += 1
    assert differing >= 1
    # ... and on the full-capacity row (three frames per token) for a good share of the tokens
    full = refs["T=768"]
    wrong = R.transcribe_ref(*next((lp, T) for name, lp, T in cases if name == "T=768"), logp="first")
    assert (np.asarray(wrong["logp"]) != np.asarray(full["logp"])).sum() >= 10


def test_a_constructed_input_tells_the_summation_orders_apart():
    """hash_noise frames are too coarsely quantised for their sums to depend on the order; float32 values spanning 1e-8 .. 40
    in magnitude are not"""
    x = R.order_sensitive_values()
    assert 1e-8 <= np.abs(x).min() < 1e-6 and 10.0 < np.abs(x).max() <= 40.0
    a, b = R.lane_sum(x), R.naive_sum(x)
    assert R.bits64(a) != R.bits64(b)
    assert abs(a - b) <= 1e-9 * abs(a)            # ... in the last bits only
    # the same through the whole restatement: one token per frame, its maximum the constructed value
    lp = np.full((len(x), D.VOCAB), np.float32(-100.0), np.float32)
    lp[np.arange(len(x)), np.arange(len(x)) % 1000] = x
    good, bad = R.transcribe_ref(lp, len(x)), R.transcribe_ref(lp, len(x), total=R.naive_sum)
    assert good["ids"] == bad["ids"] == [i % 1000 for i in range(len(x))]
    assert R.bits64(good["avg_logprob"]) != R.bits64(bad["avg_logprob"])
    assert R.bits64(good["frame_avg_logprob"]) != R.bits64(bad["frame_avg_logprob"])


def test_lane_sum_edge_cases():
    assert R.bits64(R.lane_sum(np.zeros(0, np.float32))) == R.bits64(0.0)
    assert R.bits64(R.lane_sum(np.array([-0.0], np.float32))) == R.bits64(0.0)      # +0.0 + -0.0 = +0.0
    assert np.isneginf(R.lane_sum(np.array([-np.inf, -1.0] * 70, np.float32)))
    x = np.arange(1, 131, dtype=np.float32)                                           # exact in any order
    assert R.lane_sum(x) == R.naive_sum(x) == 131 * 65
