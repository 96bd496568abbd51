"""The trie of the verse-constrained beam search (csrc/qv_trie_host.h) is pure host logic, and so is the definition of the
search.  tools/trie_check.cpp builds the trie from the committed tables for S = 1, 2, 3, 6 under AddressSanitizer + UBSan,
checks its invariants and prints statistics and array checksums, which are held here to the measured table and to the numpy
builder of tests/beam_ref.py.  The restatement of the search in beam_ref -- what the GPU tests compare the kernel with -- is
pinned independently of the code under test: against torch's CTC loss on one-sequence tries and against a brute-force sum
over all frame labellings on a small vocabulary."""
import itertools
import math
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import beam_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "offline-tarteel_amd" / "csrc"
TABLES = ROOT / "offline-tarteel_amd" / "data" / "qverse_tables.bin"

# S: (nodes, ends, max depth); the root has 185 children, every other node at most 96, at most 31 ends sit on one node
STATS = {1: (161465, 6236, 298), 2: (343929, 12358, 385), 3: (523170, 18366, 441), 6: (1046039, 35717, 673)}

# float64 round-off only: the gaps observed are 7.1e-15 (CTC loss; totals of magnitude up to 40) and 1.8e-15 (brute force;
# magnitude up to 12); asserted with a 10x margin
CTC_BOUND = 7.1e-14
BRUTE_BOUND = 1.8e-14


@pytest.fixture(scope="module")
def check_out(tmp_path_factory):
    src = ROOT / "tools" / "trie_check.cpp"
    for f in (src, CSRC / "qv_trie_host.h"):   # no HIP in or behind them
        assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # the sanitizer runtimes are linked INTO the executable, so it runs in whatever environment the suite runs in
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = tmp_path_factory.mktemp("trie") / "trie_check"
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         *static_rt, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    p = subprocess.run([str(exe), str(TABLES)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    return p.stdout


@pytest.fixture(scope="module")
def tables():
    from offline_tarteel_amd.tables import Tables

    return Tables(TABLES)


@pytest.fixture(scope="module")
def tries(tables):
    return {S: R.Trie.from_tables(tables, S) for S in (1, 3)}


def test_invariants_hold_and_the_statistics_are_the_measured_ones(check_out):
    assert "trie holds" in check_out and "refusals hold" in check_out
    stats = {int(m[0]): tuple(map(int, m[1:])) for m in re.findall(
        r"^stats S (\d) nodes (\d+) ends (\d+) max_depth (\d+) root_children (\d+) max_children (\d+) inner_children (\d+) max_ends (\d+)$",
        check_out, re.M)}
    assert sorted(stats) == [1, 2, 3, 6]
    for S, (nodes, ends, depth) in STATS.items():
        assert stats[S] == (nodes, ends, depth, 185, 185, 96, 31), S


def test_array_checksums_equal_the_numpy_builder(check_out, tries):
    sums = {int(m[0]): dict(zip(("rec", "parent", "depth", "end_off", "ends", "below_count", "below_first"), map(int, m[1:])))
            for m in re.findall(r"^sums S (\d) rec (\d+) parent (\d+) depth (\d+) end_off (\d+) ends (\d+) below_count (\d+) below_first (\d+)$",
                                check_out, re.M)}
    assert sorted(sums) == [1, 2, 3, 6]
    for S in (1, 3):
        t = tries[S]
        assert (t.n, t.n_ends(), t.max_depth, t.max_children) == (*STATS[S], 185)
        assert t.checksums() == sums[S], S


def test_numpy_builder_numbers_breadth_first_and_lists_every_sequence(tables, tries):
    t = tries[3]
    assert (np.diff(t.depth.astype(np.int64)) >= 0).all() and (t.depth[t.parent[1:]] + 1 == t.depth[1:]).all()
    kids = t.first_child[0] + np.arange(t.n_child[0])
    assert t.first_child[0] == 1 and (np.diff(t.tok[kids].astype(np.int64)) > 0).all() and int(t.below_count[0]) == t.n_ends()
    for v, sp in ((0, 1), (0, 3), (6, 1), (261, 1), (6230, 2), (6235, 1)):
        ids = tables.token_ids(v, sp)
        if len(ids) == 0:
            continue
        n = t.walk(ids)
        assert n > 0 and (v, sp) in t.ends_of(n) and t.tokens_of(n) == ids.tolist() and int(t.depth[n]) == len(ids)
    assert t.walk([1023, 1023, 1023]) == -1


def test_trie_stats_through_the_library_need_no_gpu():
    import ctypes as C

    import offline_tarteel_amd.engine as E

    assert {"qv_trie_stats", "qv_trie_node_tokens", "qv_beam_decode", "qv_beam_batch"} <= set(E.exported_symbols())
    for S, (nodes, ends, depth) in STATS.items():
        assert E.trie_stats(S) == {"nodes": nodes, "ends": ends, "max_depth": depth, "max_children": 185}
    lib = E.load_library()
    assert lib.qv_trie_stats(str(TABLES).encode(), 3, None, None, None, None) == 0          # the outputs are optional
    out = C.c_int32(-5)
    for bad in (0, 7, -1):
        assert lib.qv_trie_stats(str(TABLES).encode(), bad, C.byref(out), None, None, None) == 1
    assert lib.qv_trie_stats(None, 3, C.byref(out), None, None, None) == 1
    assert lib.qv_trie_stats(b"/nonexistent/qverse_tables.bin", 3, C.byref(out), None, None, None) == 2
    assert out.value == -5                                                                    # a refused call writes nothing
    with pytest.raises(E.QvError):
        E.trie_stats(9)
    assert E.BEAM_MAX == 64 and C.sizeof(E.QvBeamEntry) == 72


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


@pytest.mark.parametrize("seq", [[3], [2, 2], [1, 4, 4, 0, 2, 5, 1]], ids=["L=1", "L=2 repeated", "L=7"])
def test_one_sequence_trie_scores_the_ctc_likelihood(seq):
    """with W >= L + 1 nothing is pruned and the end node's total is the CTC log-likelihood: -F.ctc_loss in float64"""
    import torch
    import torch.nn.functional as F

    V, blank, L = 7, 6, len(seq)
    trie = R.Trie([np.asarray(seq)], [(0, 1)])
    assert trie.n == L + 1 and trie.walk(seq) == L
    worst = 0.0
    t_min = L + sum(a == b for a, b in zip(seq, seq[1:]))          # the shortest feasible input
    for T in (t_min, 2 * L + 1, 16):
        lp = log_softmax64(np.random.default_rng(100 * L + T).standard_normal((T, V)) * 2.0)
        r = R.beam_search(trie, lp, L + 1, blank)
        got = {n: tot for n, tot, _, _ in r["hyps"]}
        want = -float(F.ctc_loss(torch.from_numpy(lp).unsqueeze(1), torch.tensor([seq]), torch.tensor([T]), torch.tensor([L]),
                                 blank=blank, reduction="sum", zero_infinity=False))
        assert r["prune_margin"] == math.inf and math.isfinite(want)
        print(f"one sequence L={L} T={T}: |beam - ctc| = {abs(got[L] - want):.3e}")
        worst = max(worst, abs(got[L] - want))
    assert worst <= CTC_BOUND, worst


def collapse(lab, blank):
    out, prev = [], None
    for k in lab:
        if k != prev and k != blank:
            out.append(k)
        prev = k
    return tuple(out)


def test_small_vocabulary_equals_the_brute_force_sum_over_all_labellings():
    """4 tokens + blank, T = 5, W = 64 (no pruning): every node's total is the log of the summed probability of all 5^5 frame
    labellings that collapse to the node's sequence"""
    V, blank, T = 5, 4, 5
    seqs = [[0], [0, 0], [0, 1], [0, 1, 1, 2], [1], [1, 0, 1, 0, 1], [2, 3], [2, 3, 3], [3, 3, 3], [3, 2, 1, 0], [2, 0, 2]]
    trie = R.Trie([np.asarray(s) for s in seqs], [(i, 1) for i in range(len(seqs))])
    assert trie.n <= 64
    lp = log_softmax64(np.random.default_rng(5).standard_normal((T, V)) * 1.5)
    mass = {}
    for lab in itertools.product(range(V), repeat=T):
        key = collapse(lab, blank)
        mass[key] = mass.get(key, 0.0) + math.exp(sum(lp[t, k] for t, k in enumerate(lab)))
    r = R.beam_search(trie, lp, 64, blank)
    assert r["prune_margin"] == math.inf
    got = {tuple(trie.tokens_of(n)): tot for n, tot, _, _ in r["hyps"]}
    reachable = {tuple(trie.tokens_of(n)) for n in range(trie.n)} & set(mass)
    assert set(got) == reachable and {(), (0, 0), (1, 0, 1, 0, 1)} <= set(got) and (0, 1, 1, 2) in got
    worst = max(abs(got[k] - math.log(mass[k])) for k in reachable)
    print(f"brute force: {len(reachable)} nodes, worst |beam - log mass| = {worst:.3e}")
    assert worst <= BRUTE_BOUND, worst
    # the order of the result: total descending, ties to the smaller node
    keys = [(-tot, n) for n, tot, _, _ in r["hyps"]]
    assert keys == sorted(keys)


def test_pruning_margins_and_candidate_count_are_reported(tables, tries):
    trie = tries[1]
    ids = tables.token_ids(0, 1).tolist()
    lp = np.full((3 * len(ids), 1025), -20.0)
    for t in range(lp.shape[0]):
        lp[t, ids[t // 3] if t % 3 < 2 else 1024] = -1e-3
    r = R.beam_search(trie, lp, 4, 1024)
    assert r["hyps"][0][0] == trie.walk(ids) and r["max_candidates"] >= 1 + 185 and r["prune_margin"] == 0.0   # equal log-probs: exact ties
    assert 0 <= r["final_gap"] < math.inf and len(r["hyps"]) == 4
    assert R.beam_search(trie, lp[:0], 4, 1024)["hyps"] == [(0, 0.0, 0.0, -math.inf)]
    f = R.entry_fields(trie, tables, r["hyps"][0][0])
    assert (f["surah"], f["ayah"], f["ayah_end"], f["flags"], f["n_tokens"]) == (1, 1, 1, 1, len(ids)) and f["n_ends"] >= 1
