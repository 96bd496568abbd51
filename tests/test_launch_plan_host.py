"""The kernel switches (csrc/qv_switches.h: one table, one snapshot) and the launch plans (csrc/qv_launch_plan.h: GEMM tile
policy, run lengths of k_sub01 / k_sub35, attention dispatch) are pure host logic.  tools/launch_plan_check.cpp checks the
precedence of every switch (default, environment, override, override -1), pins plans that can be derived by hand, and prints
the plans over a grid that is compared here with a restatement of the rules.  Built with the host compiler under
AddressSanitizer + UBSan and run as a plain executable; the environment it reads is set through subprocess's env= only."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "offline-tarteel_amd" / "csrc"

# every environment variable the library reads: name -> (parse rule, default).  "digit": atoi if the first character is a
# digit, else ignored; "atoi": atoi of whatever is set; "one": first character == '1'
ENV_ROWS = {
    "QVERSE_LOGMEL": ("digit", 2), "QVERSE_ORT_SUB": ("digit", 1), "QVERSE_SPANS": ("digit", 1), "QVERSE_FWD_GRAPH": ("digit", 1),
    "QVERSE_CTC": ("digit", 1), "QVERSE_SUB_RUN": ("digit", 0),
    "QVERSE_ATT_OLD": ("one", 0), "QVERSE_ATT_HPB": ("one", 0), "QVERSE_ATT_TILED": ("one", 0), "QVERSE_ATT_X": ("one", 0),
    "QVERSE_GEMM_T256": ("atoi", 1), "QVERSE_GEMM_BM": ("atoi", 1), "QVERSE_GEMM_NST": ("atoi", 0), "QVERSE_GEMM_NARROW": ("atoi", -1),
    "QVERSE_GEMM_LD": ("atoi", 1), "QVERSE_GEMM_MINTILES": ("atoi", 0), "QVERSE_GEMM_MINTILES_LONGK": ("atoi", 0),
    "QVERSE_DEBUG_TAPS": ("one", 0), "QVERSE_SUB_UNFUSED": ("one", 0), "QVERSE_SUB35_UNFUSED": ("one", 0),
    "QVERSE_POST_GRAPH": ("atoi", 0), "QVERSE_CU_PARTITION": ("atoi", 0),
}
DEV_HOOK_ROWS = {"QVERSE_SKIP": ("atoi", 0), "QVERSE_DUP": ("atoi", 0)}   # rows of a -DQV_DEV_HOOKS build only
ATT_ROW = 8   # the attention variant: no variable of its own, its environment value comes from the four QVERSE_ATT_* flags


def c_atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def expected(rows, env):
    """switch values by variable name, and the attention variant, for a process started with `env`"""
    out = {}
    for name, (rule, dflt) in rows.items():
        s = env.get(name)
        if s is None:
            out[name] = dflt
        elif rule == "digit":
            out[name] = c_atoi(s) if s[:1].isdigit() else dflt
        elif rule == "atoi":
            out[name] = c_atoi(s)
        else:
            out[name] = int(s[:1] == "1")
    att = 2 if out["QVERSE_ATT_OLD"] else 1 if out["QVERSE_ATT_HPB"] else 0 if out["QVERSE_ATT_TILED"] else 5 if out["QVERSE_ATT_X"] else 3
    return out, att


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    src = ROOT / "tools" / "launch_plan_check.cpp"
    for f in (src, CSRC / "qv_switches.h", CSRC / "qv_launch_plan.h", CSRC / "qv_limits.h"):   # no HIP in or behind them
        assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # the sanitizer runtimes are linked INTO the executable, so it runs in whatever environment the suite runs in
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exes = {}
    for flavour, defs in (("product", []), ("dev_hooks", ["-DQV_DEV_HOOKS"])):
        exe = tmp_path_factory.mktemp("launch_plan") / f"launch_plan_check_{flavour}"
        cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                             *static_rt, *defs, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
        assert cc.returncode == 0, cc.stderr
        exes[flavour] = exe
    return exes


def run(exe, mode, env=None):
    base = {k: v for k, v in os.environ.items() if not k.startswith(("QVERSE_", "QV_"))}
    p = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=120, env={**base, **(env or {})})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    return p.stdout


def switch_values(stdout):
    rows = [(int(i), name, int(v)) for i, name, v in re.findall(r"^switch (\d+) (\S+) (-?\d+)$", stdout, re.M)]
    assert [i for i, _, _ in rows] == list(range(len(rows)))
    return rows


@pytest.mark.parametrize("flavour", ["product", "dev_hooks"])
def test_switch_precedence_and_parsing(check_exe, flavour):
    rows = {**ENV_ROWS, **(DEV_HOOK_ROWS if flavour == "dev_hooks" else {})}
    all_set = {name: "1" if rule == "one" else "3" for name, (rule, _) in rows.items()}
    envs = [
        {},                                                        # the defaults
        all_set,                                                   # every variable set
        {name: "0" for name in rows},
        {"QVERSE_LOGMEL": "x", "QVERSE_GEMM_T256": "x"},           # ignored / atoi("x") = 0
        {"QVERSE_SUB_RUN": "-1", "QVERSE_GEMM_NARROW": "-1", "QVERSE_CTC": " 0", "QVERSE_GEMM_BM": " 2", "QVERSE_DEBUG_TAPS": "11", "QVERSE_SUB_UNFUSED": "01",
         "QVERSE_POST_GRAPH": "yes", "QVERSE_GEMM_MINTILES": "12abc", "QVERSE_SPANS": "0x"},
        # the attention flags: OLD > HPB > TILED > X, and only '1' counts
        {"QVERSE_ATT_HPB": "1", "QVERSE_ATT_TILED": "1", "QVERSE_ATT_X": "1"},
        {"QVERSE_ATT_TILED": "1", "QVERSE_ATT_X": "1"},
        {"QVERSE_ATT_X": "1"},
        {"QVERSE_ATT_OLD": "2", "QVERSE_ATT_HPB": "true", "QVERSE_ATT_X": "1"},
        {"QVERSE_ATT_OLD": "0", "QVERSE_ATT_HPB": "1", "QVERSE_ATT_X": "1"},
    ]
    seen_att = set()
    for env in envs:
        out = run(check_exe[flavour], "switches", env)
        assert "switches hold" in out
        want, att = expected(rows, env)
        got = switch_values(out)
        assert {name for _, name, _ in got if name != "-"} == set(rows)          # the table covers every variable, once
        assert len([1 for _, name, _ in got if name != "-"]) == len(rows)
        for i, name, v in got:
            if name != "-":
                assert v == want[name], (env, name, v, want[name])
            else:
                assert v == (att if i == ATT_ROW else 0), (env, i, v)            # (rows 6 and 7: no variable, default 0)
        seen_att.add(att)
    assert seen_att == {0, 1, 2, 3, 5}
    want, att = expected(rows, envs[3])
    assert want["QVERSE_LOGMEL"] == 2 and want["QVERSE_GEMM_T256"] == 0 and expected(rows, all_set)[1] == 2


def test_hand_derived_plans(check_exe):
    assert "pins hold" in run(check_exe["product"], "pins")
    # pins do not read the environment: the same under switches that would change every plan
    assert "pins hold" in run(check_exe["product"], "pins", {"QVERSE_GEMM_T256": "2", "QVERSE_SUB_RUN": "1", "QVERSE_ATT_OLD": "1"})


def gemm_plan_codes(M, N, K, w4, has_bias, glu, in_flight, t256, bm_mode, e_nst, e_narrow, e_ld, e_min, e_min_longk):
    """gemm_plan (qv_gemm.hip's policy as of the commit that moved it into qv_launch_plan.h), restated on arrays"""
    narrow = N % 128 != 0
    narrow = narrow | (w4 & ~narrow & ((N // 128) * ((M + 127) // 128) < 400))
    narrow = np.where((e_narrow >= 0) & (N % 128 == 0) & ~glu, e_narrow != 0, narrow)
    tiles = (N // np.where(narrow, 64, 128)) * ((M + 127) // 128)
    nst = np.where(tiles >= 400, 2, np.where(K // 64 >= 16, 4, 3))
    nst = np.where(narrow & (nst > 3), 3, nst)
    nst = np.where((e_nst >= 2) & (e_nst <= np.where(narrow, 3, 4)), e_nst, nst)
    nst = np.where(e_ld == 1, 0, nst)
    allowed = (t256 > 0) & (N % 256 == 0) & has_bias & ~(w4 & ((K % 128 != 0) | (K > 4096)))
    tiles256 = (N // 256) * ((M + 255) // 256)
    busy = in_flight >= 3
    min_tiles = np.where(e_min > 0, e_min, np.where(in_flight >= 4, 1, np.where(busy, 128, 160)))
    min_tiles_longk = np.where(e_min_longk > 0, e_min_longk, np.where(busy, 1, 160))
    wide = allowed & ((t256 >= 2) | (tiles256 >= np.where(K >= 2048, min_tiles_longk, min_tiles)))
    tiles192 = (N // 256) * ((M + 191) // 192)
    cost256, cost192 = (tiles256 + 255) // 256 * 256, (tiles192 + 255) // 256 * 192
    bm192 = wide & (bm_mode > 0) & ((bm_mode >= 3) | (((bm_mode == 2) | ~busy) & (cost192 * 108 <= cost256 * 100)))
    return wide.astype(np.int64) | narrow.astype(np.int64) << 1 | nst << 2 | bm192.astype(np.int64) << 5


def gemm_kernel_codes(plan, w, glu):
    """gemm_kernel restated: the k_gemm instantiation behind a plan code (weights: 0 f16, 1 int4, 2 int8, 3 A8W8)"""
    narrow, nst = (plan >> 1 & 1) != 0, plan >> 2 & 7
    fixed = w >= 2                                     # int8 / A8W8: 128-wide, register staging, whatever the plan says
    bn64 = narrow & ~glu & ~fixed
    ld = ((nst == 0) | fixed).astype(np.int64)
    knst = np.where(ld == 1, 2, np.where(bn64, np.minimum(nst, 3), nst))
    return bn64.astype(np.int64) | (knst - 2) << 1 | ld << 3


def run_lengths(batch, frames, forced, per_step, longest_auto, forced_runs, round_blocks, cost_of_run):
    """sub01_run_tiles / sub35_run_steps restated on a [batch][frames] grid"""
    n = (frames + per_step - 1) // per_step
    if forced in forced_runs:
        best = np.full(np.broadcast(batch, n).shape, forced_runs[forced])
    else:
        runs = np.arange(1, longest_auto + 1)[:, None, None]
        cost = (batch * ((n + runs - 1) // runs) + round_blocks - 1) // round_blocks * cost_of_run(runs)
        best = 1 + np.argmin(cost, axis=0)   # the first of equal costs, as the loop's `cost < best_cost`
    return np.where(best < n, best, np.maximum(n, 1))


def test_plans_over_a_grid_equal_the_restated_rules(check_exe):
    out = run(check_exe["product"], "sweep")
    axis = {name: [int(x) for x in vals.split()] for name, vals in re.findall(r"^gemm (\w+): ([-\d ]+)$", out, re.M) if name != "env"}
    envs = [[int(x) for x in vals.split()] for vals in re.findall(r"^gemm env: ([-\d ]+)$", out, re.M)]
    # the grid is the one the rules were to be held on
    assert axis["M"][0] == 1 and axis["M"][-1] == 50000 and {255, 256, 257} <= set(axis["M"]) and sum(m % 192 == 0 for m in axis["M"]) >= 5
    assert len(set(np.diff(axis["M"]).tolist())) > 10                       # uneven steps
    assert {256, 512, 1024, 1536, 2048} <= set(axis["N"]) and axis["K"] == [256, 512, 2048, 2560] and axis["weights"] == [0, 1, 2, 3]
    assert axis["in_flight"] == [0, 1, 2, 3, 4, 5] and axis["t256"] == [0, 1, 2] and axis["bm"] == [0, 1, 2, 3] and set(axis["bias_glu"]) == {2, 0, 3}
    assert envs[0] == [0, -1, 1, 0, 0]                                      # nothing set: the table's defaults
    for col in range(5):                                                    # ... and every variable set somewhere
        assert any(e[col] != envs[0][col] for e in envs[1:]), col
    M, N, K, W, BG, F, T, B, E = np.meshgrid(*(np.array(axis[k]) for k in ("M", "N", "K", "weights", "bias_glu", "in_flight", "t256", "bm")),
                                             np.arange(len(envs)), indexing="ij")
    env = np.array(envs)[E]
    want = gemm_plan_codes(M, N, K, W == 1, (BG & 2) != 0, (BG & 1) != 0, F, T, B, *(env[..., i] for i in range(5))).ravel()
    got = np.frombuffer(re.search(r"^gemm plans: (\S+)$", out, re.M).group(1).encode(), dtype=np.uint8).astype(np.int64) - ord("0")
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(np.unravel_index(i, M.shape), int(got[i]), int(want[i])) for i in bad[:5]]
    # the grid reaches wide and 128-wide and narrow tiles (a wide plan keeps the width of its fall-back), every stage count, both tile heights
    assert set((got & 3).tolist()) == {0, 1, 2, 3} and set((got >> 2 & 7).tolist()) == {0, 2, 3, 4} and set((got >> 5).tolist()) == {0, 1}
    # ... and the kernel behind every plan: 64- and 128-wide register staging, direct loads with 2 / 3 stages at both widths and 4 at 128
    kern = np.frombuffer(re.search(r"^plan kernels: (\S+)$", out, re.M).group(1).encode(), dtype=np.uint8).astype(np.int64) - ord("0")
    want_kern = gemm_kernel_codes(want, W.ravel(), ((BG & 1) != 0).ravel())
    bad = np.flatnonzero(kern != want_kern)
    assert kern.shape == want.shape and bad.size == 0, [(np.unravel_index(i, M.shape), int(kern[i]), int(want_kern[i])) for i in bad[:5]]
    assert set(kern.tolist()) == {8, 9, 0, 1, 2, 3, 4}
    fixed = W.ravel() >= 2
    assert set(kern[fixed].tolist()) == {8} and set(kern[((BG & 1) != 0).ravel()].tolist()) <= {8, 0, 2, 4}   # int8 / A8W8: one kernel; GLU: never narrow

    lines = re.findall(r"^(sub01|sub35) batch 1\.\.(\d+) t\d 1\.\.(\d+) forced (\d): (\S+)$", out, re.M)
    assert [(k, int(f)) for k, _, _, f, _ in lines] == [("sub01", f) for f in range(5)] + [("sub35", f) for f in range(4)]
    for kernel, nb, nt, forced, codes in lines:
        nb, nt = int(nb), int(nt)
        assert nb == 256 and nt >= (1526 if kernel == "sub01" else 763)    # 61 s, the longest clip an engine accepts
        batch, frames = np.arange(1, nb + 1)[:, None], np.arange(1, nt + 1)[None, :]
        if kernel == "sub01":   # SUB_TT = 4 frames a tile; 512 blocks a round; a run costs 2 tiles + 1; forced 3 / 4 = 16 / 4 tiles
            want = run_lengths(batch, frames, int(forced), 4, 4, {1: 1, 2: 2, 3: 16, 4: 4}, 512, lambda run: 2 * run + 1)
        else:                   # S35_TC = 3 frames a step; 256 blocks a round; a run costs its steps + 1; forced 3 = 16 steps
            want = run_lengths(batch, frames, int(forced), 3, 16, {1: 1, 2: 2, 3: 16}, 256, lambda run: run + 1)
        got = (np.frombuffer(codes.encode(), dtype=np.uint8).astype(np.int64) - ord("a") + 1).reshape(nb, nt)
        assert np.array_equal(got, want), (kernel, forced, np.argwhere(got != want)[:5])
