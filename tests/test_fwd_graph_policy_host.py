"""The forward-graph replacement policy (csrc/qv_graph_policy.h: which forwards of a context replay a graph, capture one or
run as plain launches) is pure host logic: tools/fwd_graph_policy_check.cpp asserts each of its rules on hand-written key
sequences and replays the order of test_gpu_forward.py::test_forward_graph_replay_equals_the_plain_launches against the
bounds that test holds.  Built here with the host compiler under AddressSanitizer + UBSan and run as a plain executable."""
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_forward_graph_policy_rules_hold(tmp_path):
    src = ROOT / "tools" / "fwd_graph_policy_check.cpp"
    header = ROOT / "offline-tarteel_amd" / "csrc" / "qv_graph_policy.h"
    for f in (src, header):   # the policy header alone, and no HIP behind it
        assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "fwd_graph_policy_check"
    # the sanitizer runtimes are linked INTO the executable, so it runs in whatever environment the suite runs in
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         *static_rt, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"replay order: (\d+) forwards, (\d+) captures \((\d+) \+ (\d+)\), (\d+) graph launches", p.stdout)
    assert m, p.stdout
    n, captures, launches = int(m.group(1)), int(m.group(2)), int(m.group(5))
    assert 8 < captures <= 14 and launches >= n // 2, p.stdout   # the bounds the GPU test holds
    assert (n, captures, launches) == (66, 10, 52), p.stdout      # and what today's policy gives for that order
    assert "all rules hold" in p.stdout
