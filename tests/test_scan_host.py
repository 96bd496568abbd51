"""The host side of the exhaustive CTC scan (include/qverse.h, "exhaustive CTC scan"): the launch plan's counts
(csrc/qv_scan_plan.h through qv_scan_stats -- no engine, no GPU) against counts made from Tables in numpy, the argument
errors, the ranking restatement of tests/scan_ref.py (what the GPU tests compare the selection kernel with), and that
restatement against the unmodified reference's brute-force scorer through a committed fixture
(tests/golden/scan_bruteforce.npz, written by tests/golden/gen_scan_golden.py)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scan_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "offline-tarteel_amd" / "csrc"
TABLES = ROOT / "offline-tarteel_amd" / "data" / "qverse_tables.bin"

# float32 CTC loss against float64: the project's bound for clips of up to 126 frames (tests/test_gpu_postlogits.py); the
# fixture has 24 frames and losses below 200.  A score is loss / L with L >= 1.
SCORE_TOL = 1e-3


@pytest.fixture(scope="module")
def tables():
    from offline_tarteel_amd.tables import Tables

    return Tables(TABLES)


@pytest.fixture(scope="module")
def chains(tables):
    return R.chain_ids(tables)


@pytest.fixture(scope="module")
def lib():
    from offline_tarteel_amd.engine import load_library

    return load_library()


def test_plan_header_is_hip_free():
    f = CSRC / "qv_scan_plan.h"
    assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f


def test_stats_equal_the_counts_made_from_the_tables(tables, chains):
    from offline_tarteel_amd.engine import scan_stats

    seen = {}
    for T in (5, 9, 17, 33, 126, 376, 766):
        for max_span in (1, 6):
            for surahs in (None, [65]):
                got = scan_stats(T, max_span, surahs, tables_path=str(TABLES))
                want = R.stats(tables, chains, T, max_span, surahs)
                print(T, max_span, surahs, got)
                assert got == want, (T, max_span, surahs)
                seen[(T, max_span, surahs is None)] = got
    # the table is not empty where it must not be, and prefix sharing does happen
    assert seen[(5, 6, True)]["n_feasible"] > 0 and seen[(766, 6, False)]["n_feasible"] > seen[(766, 1, False)]["n_feasible"] > 0
    assert seen[(766, 6, True)]["n_recursions"] < seen[(766, 6, True)]["n_feasible"]
    assert seen[(126, 1, True)]["n_recursions"] == seen[(126, 1, True)]["n_feasible"]
    # no frames, or fewer than three: nothing is feasible
    for T in (0, 1, 2):
        assert scan_stats(T, 6, None, tables_path=str(TABLES)) == {"n_feasible": 0, "n_recursions": 0, "state_steps": 0}


def test_stats_argument_errors(lib, tmp_path):
    nf = C.c_int32(-1)
    path = str(TABLES).encode()
    ok = (C.c_uint32 * 4)(1, 0, 0, 0)
    zero = (C.c_uint32 * 4)(0, 0, 0, 0)
    assert lib.qv_scan_stats(path, 33, 6, ok, C.byref(nf), None, None) == 0 and nf.value > 0      # output pointers may be NULL
    assert lib.qv_scan_stats(path, 33, 6, None, None, None, None) == 0
    for args in ((None, 33, 6, None), (path, -1, 6, None), (path, 769, 6, None),(path, 33, 0, None), (path, 33, 7, None), (path, 33, 6, zero)):
        assert lib.qv_scan_stats(*args, C.byref(nf), None, None) == 1, args[1:3]
        assert b"qv_scan_stats" in lib.qv_last_error(None)
    assert lib.qv_scan_stats(str(tmp_path / "missing.bin").encode(), 33, 6, None, C.byref(nf), None, None) == 2
    bad = tmp_path / "bad.bin"
    bad.write_bytes(TABLES.read_bytes()[:4096])
    assert lib.qv_scan_stats(str(bad).encode(), 33, 6, None, C.byref(nf), None, None) == 2
    # a mask with a bit above the table's surahs selects nothing there but is no error
    high = (C.c_uint32 * 4)(0, 0, 0, 0x80000000)
    assert lib.qv_scan_stats(path, 766, 6, high, C.byref(nf), None, None) == 0 and nf.value == 0


def test_ranking_restatement():
    rng = np.random.default_rng(7)
    n = 600
    L = rng.integers(1, 60, n)
    span = np.tile(np.arange(1, 7), n // 6)
    losses = (rng.random(n) * 50 + 1).astype(np.float32)
    # planted ties: the same loss and length at three places -- two spans of one verse, and a later verse
    for i in (13, 14, 300):
        losses[i], L[i] = np.float32(0.001), 4             # (every other loss / L is above 1 / 59)
    span[[13, 14, 300]] = 1                                # (equal spans, so the penalty does not separate them)
    top = R.rank(losses, L, span, 0.5, 32)
    assert top[:3].tolist() == [13, 14, 300]               # key ascending = verse, then span
    assert len(top) == 32 and len(set(top.tolist())) == 32
    assert R.rank(losses, L, span, 0.5, 1000).shape == (n,)            # k clips to the number of keys
    # penalty 0.0: a plain stable sort by loss / L in float32
    plain = np.argsort(losses / L.astype(np.float32), kind="stable")
    assert R.rank(losses, L, span, 0.0, n).tolist() == plain.tolist()
    # the penalty is 0.5 per additional ayah, in double
    norm, fin = R.finals(losses, L, span, 0.5)
    assert norm.dtype == np.float32 and fin.dtype == np.float64
    assert np.array_equal(fin, -norm.astype(np.float64) - 0.5 * (span - 1))
    # -0.0 and +0.0 are one score
    z = R.rank(np.array([0.0, 0.0], np.float32), np.array([3, 3]), np.array([1, 1]), 0.0, 2)
    assert z.tolist() == [0, 1]


def test_restatement_against_the_reference_scorer(tables, golden_dir):
    g = np.load(golden_dir / "scan_bruteforce.npz")
    logits, gv, gs, gscore = g["logits"], g["verse"].astype(np.int64), g["span"].astype(np.int64), g["score"]
    assert logits.shape == (1, 24, 1025) and logits.dtype == np.float32
    T = logits.shape[1]
    key, v, sp, L = R.keys(tables, T, 6, [1, 112, 113, 114])
    gkey = gv * 6 + gs - 1
    # the fixture lists every non-empty key of the four surahs once
    lens = R.lengths(tables)
    want_all = np.flatnonzero(np.repeat(R.selected(tables, [1, 112, 113, 114]), 6) & (lens > 0))
    assert sorted(gkey.tolist()) == want_all.tolist()
    # the sentinel: exactly the keys the gate refuses, +inf, behind every scored one
    fin_mask = np.isfinite(gscore)
    assert sorted(gkey[fin_mask].tolist()) == key.tolist() and len(key) > 10
    assert np.all(gscore[~fin_mask] == np.inf) and not fin_mask[fin_mask.sum():].any()
    # the scores: loss / L
    x = logits[0].astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    lp = x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))
    losses = R.losses64(lp, tables, key)
    norm = dict(zip(key.tolist(), (losses / L).tolist()))
    worst = max(abs(norm[k] - s) for k, s in zip(gkey[fin_mask].tolist(), gscore[fin_mask].tolist()))
    print(f"worst |loss / L - reference score| {worst:.3e}")
    assert worst <= SCORE_TOL
    # the order: the restatement's ranking at penalty 0.0 is the reference's list wherever two scores differ by more than
    # the tolerance of either
    order = key[R.rank(losses.astype(np.float32), L, sp, 0.0, len(key))]
    ref_order = gkey[fin_mask]
    ref_score = dict(zip(gkey.tolist(), gscore.tolist()))
    for a, b in zip(order.tolist(), ref_order.tolist()):
        assert a == b or abs(ref_score[a] - ref_score[b]) <= 2 * SCORE_TOL, (a, b)
    # the planted verse (surah 112 ayah 1) leads both, clearly
    assert order[0] == ref_order[0] == tables.verse_index(112, 1) * 6
    assert gscore[1] - gscore[0] > 100 * SCORE_TOL


def test_symbols_are_exported(lib):
    from offline_tarteel_amd.engine import exported_symbols

    for s in ("qv_scan_stats", "qv_scan_logprobs", "qv_scan_batch", "qv_scan_kernel_times"):
        assert s in exported_symbols() and hasattr(lib, s), s
