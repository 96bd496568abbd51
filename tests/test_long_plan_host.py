"""The rule by which a recording of any length is cut into windows (csrc/qv_long_plan.h) is pure host logic.
tools/long_plan_check.cpp holds n / 1280 + 1 to the forward's own frame arithmetic, checks the plan's invariants over a grid
of (n, Kw, M) -- the ownership ranges tile [0, T), every owned frame is a valid frame of its window, the last window's frames
plus its offset are T -- and the refusals, and prints every plan; the plans are compared here with tests/long_ref.py, the
restatement the GPU tests cut and stitch by.  Built with the host compiler under AddressSanitizer + UBSan and run as a plain
executable."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import long_ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "offline-tarteel_amd" / "csrc"


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    src = ROOT / "tools" / "long_plan_check.cpp"
    for f in (src, CSRC / "qv_long_plan.h"):   # no HIP in or behind them
        assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # the sanitizer runtimes are linked INTO the executable, so it runs in whatever environment the suite runs in
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = tmp_path_factory.mktemp("long_plan") / "long_plan_check"
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         *static_rt, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    return exe


def run(exe, mode):
    p = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    return p.stdout


def test_frames_are_n_over_1280_plus_one(check_exe):
    assert "frames hold" in run(check_exe, "frames")
    assert all(long_ref.frames(n) == n // 1280 + 1 for n in (0, 1279, 1280, 48000, 200000))


def test_bad_arguments_are_refused(check_exe):
    assert "refusals hold" in run(check_exe, "refused")
    W = 37 * 1280
    for bad in ((-1, 48000, W, 6), (100000, 48000, W + 1, 6), (100000, 48000, 1000, 6), (100000, 48000, W + 1280, 6),
                (100000, 1279, 0, 0), (100000, 48000, W, 19), (100000, 48000, 2560, 1), (100000, 48000, W, -2)):
        with pytest.raises(long_ref.BadPlan):
            long_ref.plan(*bad)
    with pytest.raises(long_ref.TooLong):
        long_ref.plan(1280 * 262144, 48000, W, 6)
    assert long_ref.plan(1280 * 262144 - 1, 48000, W, 6).t_total == 262144 and long_ref.plan(100000, 48000, W, 18).h == 1


def test_the_library_exports_the_plan_and_it_needs_no_gpu():
    """qv_long_plan through the built library: the header's rule behind the C ABI, with QV_ERR_ARG / QV_ERR_CAPACITY"""
    import ctypes as C

    import offline_tarteel_amd.engine as E

    assert {"qv_long_plan", "qv_transcribe_long", "qv_transcribe_windows", "qv_long_kernel_times"} <= set(E.exported_symbols())
    lib = E.load_library()
    out = [C.c_int32(-5) for _ in range(4)]
    for n, mx, window, margin in ((211000, 48000, 0, -1), (48001, 48000, 37 * 1280, 6), (47360, 48000, 0, 0), (100000, 48000, 37 * 1280, 18),
                                  (9600000, 480000, 0, -1), (1280 * 262144 - 1, 976000, 0, -1)):
        assert lib.qv_long_plan(n, mx, window, margin, *map(C.byref, out)) == 0
        p = long_ref.plan(n, mx, window, margin)
        assert [v.value for v in out] == [p.n_windows, p.t_total, p.kw, p.m], (n, mx, window, margin)
    assert lib.qv_long_plan(9600000, 480000, 0, -1, None, None, None, None) == 0            # the outputs are optional
    before = [v.value for v in out]
    assert lib.qv_long_plan(100000, 48000, 37 * 1280, 19, *map(C.byref, out)) == 1           # H < 1
    assert lib.qv_long_plan(100000, 48000, 1000, -1, *map(C.byref, out)) == 1                # not a multiple of 1280
    assert lib.qv_long_plan(1280 * 262144, 48000, 0, -1, *map(C.byref, out)) == 4            # above QV_LONG_MAX_FRAMES
    assert [v.value for v in out] == before                                                  # a refused call writes nothing
    assert E.QV_LONG_MAX_FRAMES == long_ref.MAX_FRAMES and E.QV_LONG_HOP == long_ref.HOP and C.sizeof(E.QvLongInfo) == 48


def test_window_and_margin_from_the_environment_are_read_once(monkeypatch):
    import offline_tarteel_amd.engine as E

    monkeypatch.setattr(E, "_long_env", None)
    monkeypatch.setenv("QVERSE_LONG_WINDOW_S", "20")
    monkeypatch.setenv("QVERSE_LONG_MARGIN_S", "2.0")
    assert E.long_env() == (20.0, 2.0)
    monkeypatch.setenv("QVERSE_LONG_WINDOW_S", "25")                       # read once: a later change is not seen
    assert E.long_env() == (20.0, 2.0)
    args = E.Engine._long_args
    assert args(None, None, None) == (320000 // 1280 * 1280, 25)           # 20 s: 250 frames; 2 s: 25 frames
    assert args(None, 2.96, 0.48) == (37 * 1280, 6) and args(None, 3.0, 0.0) == (37 * 1280, 0)   # the call's own values win
    with pytest.raises(E.QvError):
        args(None, 0.05, None)                                             # shorter than one frame
    monkeypatch.setattr(E, "_long_env", None)
    monkeypatch.delenv("QVERSE_LONG_WINDOW_S")
    monkeypatch.delenv("QVERSE_LONG_MARGIN_S")
    assert E.long_env() == (None, None) and args(None, None, None) == (0, -1)                    # the library's defaults
    monkeypatch.setattr(E, "_long_env", None)


def test_plans_over_a_grid_tile_the_frames_and_equal_the_restated_rule(check_exe):
    out = run(check_exe, "grid")
    assert re.search(r"^grid holds \d+$", out, re.M)
    plans = [tuple(map(int, g)) for g in re.findall(r"^plan (\d+) (\d+) (-?\d+): (\d+) (\d+) (\d+) (\d+)$", out, re.M)]
    assert len(plans) > 1000
    # the grid is the one the rule was to be held on
    kws = {w // 1280 for _, w, *_ in plans}
    assert {1, 37, 762} <= kws
    assert any(kw - 2 * m == 1 and nw > 1 for _, _, _, nw, _, kw, m in plans)                  # Kw - 2M = 1
    assert any(m == 0 and nw > 1 for _, _, _, nw, _, _, m in plans) and any(mm == -1 for _, _, mm, *_ in plans)
    for d in (-1, 0, 1, 1279):
        assert any(n == w + d and w == 37 * 1280 for n, w, *_ in plans), d                     # n = window - 1, window, + 1, + 1279
    assert max(t for *_, t, _, _ in plans) == 262144
    for n, window, margin, nw, t, kw, m in plans:
        p = long_ref.plan(n, window, window, margin)
        assert (p.n_windows, p.t_total, p.kw, p.m) == (nw, t, kw, m), (n, window, margin)
        if nw > 3000:       # (the invariants below were checked by the program for every plan; restated here on the smaller ones)
            continue
        edge = 0
        for w, (start, ln, fwd, lo, hi) in enumerate(p.windows()):
            assert lo == edge < hi and start % 1280 == 0 and 0 <= lo - w * p.h and hi - w * p.h <= long_ref.frames(ln), (n, window, margin, w)
            assert long_ref.frames(fwd) == long_ref.frames(ln) and (fwd == ln or (w > 0 and ln < 400 and fwd == 400 and p.m == 0))
            edge = hi
        assert edge == t == long_ref.frames(p.length(nw - 1)) + (nw - 1) * p.h
