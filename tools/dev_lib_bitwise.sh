#!/bin/bash
# dev: the log-probs of a ragged seeded batch from two library builds, compared bitwise (tools/ab_forward.py)
#   bash tools/dev_lib_bitwise.sh A/libqverse.so B/libqverse.so [--variant N] [--precision P] [--gemm-tiles T] [--gemm-tile-height H] [--frames T ...]
set -u
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$R"
A=$1 B=$2
shift 2
rm -f /tmp/lp_a.pt /tmp/lp_b.pt
QVERSE_LIB=$R/$A timeout -k 10 120 python tools/ab_forward.py /tmp/lp_a.pt "$@" > /tmp/lp_a.log 2>&1 &&
QVERSE_LIB=$R/$B timeout -k 10 120 python tools/ab_forward.py /tmp/lp_b.pt "$@" > /tmp/lp_b.log 2>&1 ||
    { echo "bitwise: a forward run FAILED (status $?; /tmp/lp_a.log, /tmp/lp_b.log)"; exit 1; }   # nothing more runs on the GPU
python - <<'PY'
import sys
import torch
a, b = torch.load("/tmp/lp_a.pt"), torch.load("/tmp/lp_b.pt")
same = torch.equal(a["lp"], b["lp"])
print("bitwise:", "identical" if same else f"DIFFERS, max |d| {float((a['lp'] - b['lp']).abs().max()):g}")
sys.exit(0 if same else 1)
PY
